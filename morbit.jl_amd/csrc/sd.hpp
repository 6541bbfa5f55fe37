// What the steepest-descent entry points share: the direction LP's launcher and the row assembly of sd_lp.hip, the step-size, trial-row
// and Armijo kernels of sd_step.hip.  Every kernel takes the start on a grid dimension and per-start strides, so that a single call
// (mrbf_sd_criticality, mrbf_sd_step) is the batch of one of mrbf_sd_iterate_batch (sd_batch.hip) through the same code.
#pragma once
#include "common.hpp"

namespace mrbf {
namespace sd {

constexpr int THREADS = 256;
constexpr int MAXM = 64;
constexpr int MAXD = 4096;

// ---- get_criticality's right-hand sides: one workgroup per LP row and start (RowSrc and its filler: descent_problem.hpp); kind 0 rows read
// the Jacobian at x_n, kind 2 rows the Jacobian at x and the value at x_n
using descent::RowSrc;
struct AsmArgs {
    int n, k, rows, meq, min;
    int64_t sJ, sV, sx;  // per-start strides of J, of V, of xn / x; G, A_eq, b_eq, A_ineq, b_ineq lie in the consecutive per-LP blocks of launch()
    const double *J, *V, *xn, *x, *Alin, *blin;  // Alin / blin: the one MOP's linear rows, shared by the starts
    double *G, *Aeq, *beq, *Ain, *bin;
    RowSrc src[MAXM];
};
int launch_assemble(mrbf_ctx *ctx, const AsmArgs &a, int64_t n_starts);

// all device pointers; LPs in chunks so that the per-LP workspace stays below 256 MB.  LP p reads x at x + p x_stride and its bounds at
// lb / ub + p bound_stride (0: one box for every LP); everything else lies in consecutive per-LP blocks.
int launch(mrbf_ctx *ctx, int64_t n_lp, int n, int k, int meq, int min, int normalize, const double *G, const double *x, int64_t x_stride,
           const double *lb, const double *ub, int64_t bound_stride, const double *Aeq, const double *beq, const double *Ain,
           const double *bin, double *d_out, double *omega_out, double *dual_out, int *status_out, int *iters_out);

}  // namespace sd

namespace sdstep {

constexpr int THREADS = 256;
constexpr int MAXK = 64, MAXROWS = 256;  // the limits of mrbf_dispatch_sd_step (d <= 4096, max_loops <= 1024) need no array here

// one constraint row of the stacked problem of descent.jl:279-285: the row acts on the x_n half (linear rows) or on the n = x_n - x
// half (modelled rows); a(t) = A[a_off + t * stride], right-hand side b_lin[b_off] (linear) or -Vc[b_off] (modelled)
struct RowRef {
    int64_t a_off, b_off;
    int32_t stride, modelled;
};
struct ObjSrc {
    int64_t off;     // value of objective l at site p: V[off + p * stride]
    int64_t stride;  // the model's output count
};

// per-start strides (s*): start p reads its arrays at base + p * stride; lb / ub, the linear rows and the rows table are shared
struct StepArgs {
    int d, n_eq, n_in, max_loops;
    double shrink;
    int64_t sx, sdir, sJ, sV;  // of xn / x, of dir, of Jc, of Vc
    const double *delta;       // one per start
    const double *xn, *x, *lb, *ub, *dir;
    const double *Alin, *blin, *Jc, *Vc;
    const RowRef *rows;  // n_eq equality rows (linear, then modelled), then n_in inequality rows (likewise)
    double *steps;       // per start max_loops + 1
    double *out;         // per start [sigma, branch]
};
int launch_stepsize(mrbf_ctx *ctx, const StepArgs &a, int64_t n_starts);
// StepArgs::rows of a container: linear equalities, modelled equalities, linear inequalities, modelled inequalities; `at` = the
// offsets of the one-site evaluations at x of the slots with constraint rows
inline std::vector<RowRef> stacked_rows(const descent::Layout &L, const descent::Offsets &at) {
    std::vector<RowRef> rows;
    for (int eq = 1; eq >= 0; --eq) {
        const int first = eq ? 0 : L.n_lin_eq, nlin = eq ? L.n_lin_eq : L.n_lin_ineq;
        for (int i = first; i < first + nlin; ++i) rows.push_back(RowRef{(int64_t)i * L.d, i, 1, 0});
        // the Jacobian block of a slot is k x d column-major: entry (c, t) at t * k + c
        for (const descent::Row &m : L.rows)
            if (m.eq == (eq != 0)) rows.push_back(RowRef{at.jac[m.slot] + m.col, at.val[m.slot] + m.col, L.k[m.slot], 1});
    }
    return rows;
}
// per start: row 0 = x_n, row 1 + i = x_n + steps[i] * d, i = 0 .. max_loops
int launch_trial(mrbf_ctx *ctx, const double *xn, int64_t sx, const double *dir, int64_t sdir, const double *steps, int d, int max_loops,
                 int64_t n_starts, double *X);

struct ArmijoArgs {
    int d, k, max_loops, strict;
    double const_rhs, min_stepsize_raw, min_step;
    int64_t sV, sdir;     // per-start strides of V and of dir (X, steps, stepout and the outputs follow from d, k and max_loops)
    const double *omega;  // one per start
    const double *V;      // values of the objective models at the L + 2 rows (each model's block: rows x its outputs)
    const double *X;      // the L + 2 trial rows
    const double *dir, *steps, *stepout;
    double *xplus, *mxplus;  // per start d / k
    double *tail;            // per start [omega, step_norm, loops, sigma, branch]
    ObjSrc obj[MAXK];
};
constexpr int ARMIJO_TAIL = 5;  // words per start of ArmijoArgs::tail
int launch_armijo(mrbf_ctx *ctx, const ArmijoArgs &a, int64_t n_starts);
// ArmijoArgs::obj of a container; `at` = the offsets of the objective slots' values at the L + 2 trial rows
inline void fill_objectives(const descent::Layout &L, const descent::Offsets &at, ObjSrc *obj) {
    for (size_t l = 0; l < L.obj.size(); ++l) obj[l] = ObjSrc{at.val[L.obj[l].slot] + L.obj[l].col, L.k[L.obj[l].slot]};
}

}  // namespace sdstep
}  // namespace mrbf
