// The one reader of a surrogate container's roles table (mrbf_ps_problem, include/mrbf.h) and what the descent entry points build on
// it: mrbf_ps_step_problem, mrbf_sd_criticality, mrbf_sd_step, mrbf_sd_iterate_batch, mrbf_normal_step, mrbf_normal_step_batch.  Host
// code without a HIP include and without a context, so that tools/descent_problem_check.cpp can drive it as a plain C++ program: the
// caller describes the models (d, k, n per slot and start), a defect comes back by value, and the entry point maps its class to its
// own return code in front of its own name.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mrbf.h"

namespace mrbf {
namespace descent {

// ---- what the reader is told
struct SlotShape {
    bool present;  // false: the handle is NULL
    int d, k;      // variables, outputs
    int64_t n;     // centres
};
struct Shape {
    int n_slots = 0;
    int64_t n_starts = 1;
    const SlotShape *slots = nullptr;  // start-major n_starts x n_slots; start 0 gives every slot's output count
    const int32_t *roles = nullptr;    // one entry per output of every slot, in slot order
    int n_objectives = 0, n_lin_eq = 0, n_lin_ineq = 0;
    bool lin_eq_given = false, lin_ineq_given = false;  // A and b of the block are both there
    int d = -1;          // the number of variables where the entry point is told it (the normal step), else -1: slot 0's
    bool batch = false;  // the messages name the start
};
enum class Centres { UNCHECKED, EVERY_SLOT, CONSTRAINED_SLOTS };  // which slots must have centres
struct Needs {
    bool objectives;  // false: the objective rows are ignored, whatever the table says of them (the normal step)
    Centres centres;
};

struct Defect {
    enum Class { NONE = 0, PROBLEM, MODELS, ROLE } cls = NONE;
    int index = -1;  // ROLE: the entry of the table (-1: an objective position that no entry takes); MODELS: the slot
    std::string msg;
    explicit operator bool() const { return cls != NONE; }
};
inline Defect defect(Defect::Class cls, int index, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    Defect D;
    D.cls = cls, D.index = index, D.msg = buf;
    return D;
}

// ---- what the reader gives
struct Entry {
    int slot, col;
};
struct Row {
    int slot, col;
    bool eq;
};
enum class Slots { USED, CONSTRAINED, OBJECTIVE };
// where the evaluations of the chosen slots lie: slot j's Jacobians (sites x k_j x d) at jac[j], its values (sites x k_j) at val[j]
struct Offsets {
    std::vector<int64_t> jac, val;
    int64_t jtot = 0, vtot = 0;
};
struct Layout {
    int d = 0;
    std::vector<int> k;                // outputs of every slot
    std::vector<Entry> obj;            // objective position l is output obj[l].col of slot obj[l].slot
    std::vector<Row> rows;             // the modelled constraint rows in the table's order
    std::vector<char> has_obj, has_con;  // per slot
    int n_lin_eq = 0, n_lin_ineq = 0;
    int n_nl = 0, meq = 0, min = 0;    // modelled rows; equality / inequality rows, the linear ones included

    bool chosen(int j, Slots which) const {
        return which == Slots::USED ? (has_obj[j] || has_con[j]) : (which == Slots::CONSTRAINED ? has_con[j] != 0 : has_obj[j] != 0);
    }
    Offsets offsets(int64_t sites, Slots which) const {
        Offsets o;
        o.jac.assign(k.size(), 0), o.val.assign(k.size(), 0);
        for (size_t j = 0; j < k.size(); ++j) {
            if (!chosen((int)j, which)) continue;
            o.jac[j] = o.jtot, o.val[j] = o.vtot;
            o.jtot += sites * k[j] * d, o.vtot += sites * k[j];
        }
        return o;
    }
};

inline Defect read(const Shape &S, const Needs &needs, Layout &L) {
    const int nm = S.n_slots, nobj = needs.objectives ? S.n_objectives : 0;
    if (nm < 0 || (nm > 0 && (!S.slots || !S.roles))) return defect(Defect::PROBLEM, -1, "models need handles and a roles table");
    if (needs.objectives && nobj < 1) return defect(Defect::PROBLEM, -1, "%d objectives", S.n_objectives);
    if (S.n_lin_eq < 0 || S.n_lin_ineq < 0) return defect(Defect::PROBLEM, -1, "negative constraint count");
    if ((S.n_lin_eq && !S.lin_eq_given) || (S.n_lin_ineq && !S.lin_ineq_given))
        return defect(Defect::PROBLEM, -1, "linear constraint matrices are NULL");
    // ---- start 0's slots give d and every slot's output count
    const char *of0 = S.batch ? " of start 0" : "";
    L.d = S.d >= 0 ? S.d : (nm > 0 && S.slots[0].present ? S.slots[0].d : 0);
    L.k.assign(nm, 0);
    for (int j = 0; j < nm; ++j) {
        const SlotShape &M = S.slots[j];
        if (!M.present) return defect(Defect::MODELS, j, "model %d%s is NULL", j, of0);
        if (M.d != L.d) return defect(Defect::MODELS, j, "model %d%s has %d variables, model 0 has %d", j, of0, M.d, L.d);
        L.k[j] = M.k;
    }
    // ---- the table
    L.obj.assign(nobj, Entry{-1, -1});
    L.rows.clear();
    L.has_obj.assign(nm, 0), L.has_con.assign(nm, 0);
    for (int j = 0, e = 0; j < nm; ++j)
        for (int c = 0; c < L.k[j]; ++c, ++e) {
            const int role = S.roles[e];
            if (role >= 0) {
                if (!needs.objectives) continue;
                if (role >= nobj || L.obj[role].slot >= 0)
                    return defect(Defect::ROLE, e, "roles[%d] = %d is not a (new) objective position", e, role);
                L.obj[role] = Entry{j, c};
                L.has_obj[j] = 1;
            } else if (role == MRBF_ROLE_EQ || role == MRBF_ROLE_INEQ) {
                L.rows.push_back(Row{j, c, role == MRBF_ROLE_EQ});
                L.has_con[j] = 1;
            } else if (role != MRBF_ROLE_NONE) {
                return defect(Defect::ROLE, e, "roles[%d] = %d is not a role", e, role);
            }
        }
    for (int l = 0; l < nobj; ++l)
        if (L.obj[l].slot < 0) return defect(Defect::ROLE, -1, "objective %d is not an output of any model", l);
    // ---- every start's slots agree with start 0's; the slots that will be evaluated have centres
    for (int64_t p = 0; p < S.n_starts; ++p)
        for (int j = 0; j < nm; ++j) {
            const SlotShape &M = S.slots[p * nm + j];
            if (!M.present) return defect(Defect::MODELS, j, "model %d of start %lld is NULL", j, (long long)p);
            if (M.d != L.d || M.k != L.k[j])
                return defect(Defect::MODELS, j, "model %d of start %lld is %d variables x %d outputs, %s %d x %d", j, (long long)p, M.d, M.k,
                              S.d >= 0 ? "expected" : "start 0 has", L.d, L.k[j]);
            const bool needs_n = needs.centres == Centres::EVERY_SLOT || (needs.centres == Centres::CONSTRAINED_SLOTS && L.has_con[j]);
            if (needs_n && M.n == 0) return defect(Defect::MODELS, j, "model %d of start %lld has no centres", j, (long long)p);
        }
    L.n_lin_eq = S.n_lin_eq, L.n_lin_ineq = S.n_lin_ineq;
    L.n_nl = (int)L.rows.size();
    L.meq = S.n_lin_eq, L.min = S.n_lin_ineq;
    for (const Row &r : L.rows) ++(r.eq ? L.meq : L.min);
    return Defect();
}

// ---- one row of the LPs' right-hand sides, as the assembly kernels of sd_lp.hip and normal_lp.hip read it: one workgroup per row and
// start, the Jacobians / values of the evaluation kernels as they lie
struct RowSrc {
    int kind;      // 0 objective row (Jacobian at the first site), 1 linear row, 2 modelled constraint row
    int dst;       // objective position / row of A_eq or A_ineq
    int eq;        // 1: equality block
    int stride;    // rows of the model (k_j): the Jacobian is k_j x d column-major per site
    int64_t jac;   // offset of the row's first entry in the Jacobian buffer (site 0; site 1 follows after k_j d)
    int64_t val;   // offset of the row's value at site 0 / index of the linear row
};
// the sources in the kernels' order: [objective rows,] linear equalities, modelled equalities, linear inequalities, modelled
// inequalities; `at` = the offsets of the evaluations the rows are taken from.  Returns the number of rows.
inline int fill_sources(const Layout &L, const Offsets &at, bool objectives, RowSrc *src) {
    int r = 0;
    if (objectives)
        for (size_t l = 0; l < L.obj.size(); ++l) {
            const Entry &o = L.obj[l];
            src[r++] = RowSrc{0, (int)l, 0, L.k[o.slot], at.jac[o.slot] + o.col, at.val[o.slot] + o.col};
        }
    for (int eq = 1; eq >= 0; --eq) {
        const int nlin = eq ? L.n_lin_eq : L.n_lin_ineq;
        for (int i = 0; i < nlin; ++i) src[r++] = RowSrc{1, i, eq, 1, 0, (eq ? 0 : L.n_lin_eq) + i};
        int dst = nlin;
        for (const Row &m : L.rows)
            if (m.eq == (eq != 0)) src[r++] = RowSrc{2, dst++, eq, L.k[m.slot], at.jac[m.slot] + m.col, at.val[m.slot] + m.col};
    }
    return r;
}

}  // namespace descent
}  // namespace mrbf
