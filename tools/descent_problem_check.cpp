// Stand-alone host check of the one reader of a container's roles table (morbit.jl_amd/csrc/descent_problem.hpp), which the six descent
// entry points share.  Every case is judged by statements made directly from the table as include/mrbf.h defines it ("one entry per
// output row of every model, concatenated in model order: l >= 0 -> objective l; MRBF_ROLE_EQ / _INEQ -> modelled constraint;
// MRBF_ROLE_NONE -> not used"), not by a second copy of the reader's loop.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror tools/descent_problem_check.cpp -o /tmp/descent_problem_check && /tmp/descent_problem_check
// and once under the sanitizers:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer tools/descent_problem_check.cpp -o /tmp/descent_problem_check && /tmp/descent_problem_check
// The tables: 1 .. 3 slots of 1 .. 3 outputs each, n_objectives 0 .. 3, entries from {NONE, EQ, INEQ, 0 .. n_objectives, -7}, read
// with and without objective rows.  Tables of up to 5 entries are enumerated in full.  With 6 .. 9 entries there are 3 10^8 tables, far
// more than a test of a few seconds can read, and nearly all of them only differ behind their first defective entry: there every table
// is enumerated up to and including its first defective entry, and the entries behind it are filled in two ways (all NONE; the
// alphabet in turn); read without objective rows, where no objective entry can be a defect, one objective entry stands for all of
// them.  `--all` enumerates those in full as well (an hour).  Then the slot defects on every accepted table of up to 4
// entries: a NULL slot, another d, another k in a second start, a slot without centres.
#include <cstdio>
#include <cstring>

#include "../morbit.jl_amd/csrc/descent_problem.hpp"

using namespace mrbf::descent;

static long g_cases = 0, g_accepted = 0;
static int g_failed = 0;
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, case_text()); \
        }                                                                          \
    } while (0)

constexpr int D = 3, UNKNOWN = -7;
constexpr int FULL = 5;  // tables of up to so many entries are enumerated in full

struct Case {
    int ns, k[3], nobj, ne;
    int32_t roles[9];
};
// the case under test, put into words only when a check fails
static const Case *g_case = nullptr;
static bool g_objectives = false;
static void describe(const Case &c, bool objectives) { g_case = &c, g_objectives = objectives; }
static const char *case_text() {
    static char g_what[256];
    const Case &c = *g_case;
    const bool objectives = g_objectives;
    int at = std::snprintf(g_what, sizeof(g_what), "k =");
    for (int j = 0; j < c.ns; ++j) at += std::snprintf(g_what + at, sizeof(g_what) - at, " %d", c.k[j]);
    at += std::snprintf(g_what + at, sizeof(g_what) - at, ", %d objectives%s, roles =", c.nobj, objectives ? "" : " (ignored)");
    for (int e = 0; e < c.ne; ++e) at += std::snprintf(g_what + at, sizeof(g_what) - at, " %d", c.roles[e]);
    return g_what;
}
static bool is_con(int role) { return role == MRBF_ROLE_EQ || role == MRBF_ROLE_INEQ; }
// slot and column of entry e, from the slots' output counts alone
static void where(const Case &c, int e, int *slot, int *col) {
    int j = 0;
    while (e >= c.k[j]) e -= c.k[j++];
    *slot = j, *col = e;
}
static int count_role(const Case &c, int role) {
    int n = 0;
    for (int e = 0; e < c.ne; ++e) n += c.roles[e] == role;
    return n;
}

// the offsets of distinct chosen slots do not overlap and cover exactly the requested sizes; slots not chosen take nothing
static void check_offsets(const Layout &L, int64_t sites, Slots which) {
    const Offsets o = L.offsets(sites, which);
    const int nm = (int)L.k.size();
    int64_t jsum = 0, vsum = 0;
    for (int j = 0; j < nm; ++j) {
        if (!L.chosen(j, which)) continue;
        const int64_t jn = sites * L.k[j] * L.d, vn = sites * L.k[j];
        jsum += jn, vsum += vn;
        CHECK(o.jac[j] >= 0 && o.jac[j] + jn <= o.jtot && o.val[j] >= 0 && o.val[j] + vn <= o.vtot);
        for (int i = 0; i < j; ++i) {
            if (!L.chosen(i, which)) continue;
            CHECK(o.jac[i] + sites * L.k[i] * L.d <= o.jac[j] || o.jac[j] + jn <= o.jac[i]);
            CHECK(o.val[i] + sites * L.k[i] <= o.val[j] || o.val[j] + vn <= o.val[i]);
        }
    }
    CHECK(jsum == o.jtot && vsum == o.vtot);
}

static void check_case(const Case &c, bool objectives, int n_lin_eq, int n_lin_ineq) {
    ++g_cases;
    describe(c, objectives);
    SlotShape slots[3];
    for (int j = 0; j < c.ns; ++j) slots[j] = SlotShape{true, D, c.k[j], 10};
    Shape S;
    S.n_slots = c.ns, S.slots = slots, S.roles = c.roles;
    S.n_objectives = c.nobj, S.n_lin_eq = n_lin_eq, S.n_lin_ineq = n_lin_ineq;
    S.lin_eq_given = S.lin_ineq_given = true;
    static Layout L;
    const Defect def = read(S, Needs{objectives, Centres::EVERY_SLOT}, L);
    // ---- what the table says
    bool valid = !objectives || c.nobj >= 1;
    for (int e = 0; e < c.ne; ++e) {
        const int r = c.roles[e];
        if (r < 0 && r != MRBF_ROLE_NONE && !is_con(r)) valid = false;
        if (objectives && r >= c.nobj) valid = false;
    }
    for (int l = 0; objectives && l < c.nobj; ++l) valid = valid && count_role(c, l) == 1;
    CHECK(valid == !def);
    if (def) {
        CHECK(!def.msg.empty());
        if (objectives && c.nobj < 1) {
            CHECK(def.cls == Defect::PROBLEM);
        } else {
            CHECK(def.cls == Defect::ROLE && def.index >= -1 && def.index < c.ne);
            if (def.cls != Defect::ROLE || def.index < -1 || def.index >= c.ne) return;
            if (def.index >= 0) {
                const int r = c.roles[def.index];
                const bool unknown = r < 0 && r != MRBF_ROLE_NONE && !is_con(r);
                CHECK(unknown || (objectives && r >= 0 && (r >= c.nobj || count_role(c, r) > 1)));
            } else {
                bool missing = false;
                for (int l = 0; l < c.nobj; ++l) missing = missing || count_role(c, l) == 0;
                CHECK(objectives && missing);
            }
        }
        return;
    }
    ++g_accepted;
    // ---- an accepted table: position l is the entry whose role is l; the modelled rows are the EQ / INEQ entries in table order
    CHECK(L.d == D && (int)L.k.size() == c.ns && (int)L.obj.size() == (objectives ? c.nobj : 0));
    for (int j = 0; j < c.ns; ++j) CHECK(L.k[j] == c.k[j]);
    bool has_obj[3] = {false, false, false}, has_con[3] = {false, false, false};
    int n_rows = 0, n_eq = 0;
    for (int e = 0; e < c.ne; ++e) {
        int slot, col;
        where(c, e, &slot, &col);
        const int r = c.roles[e];
        if (objectives && r >= 0) {
            CHECK(L.obj[r].slot == slot && L.obj[r].col == col);
            has_obj[slot] = true;
        }
        if (is_con(r)) {
            CHECK(n_rows < (int)L.rows.size() && L.rows[n_rows].slot == slot && L.rows[n_rows].col == col &&
                  L.rows[n_rows].eq == (r == MRBF_ROLE_EQ));
            ++n_rows, n_eq += r == MRBF_ROLE_EQ;
            has_con[slot] = true;
        }
    }
    CHECK(n_rows == (int)L.rows.size() && L.n_nl == n_rows);
    CHECK(L.meq == n_lin_eq + n_eq && L.min == n_lin_ineq + n_rows - n_eq && L.n_lin_eq == n_lin_eq && L.n_lin_ineq == n_lin_ineq);
    for (int j = 0; j < c.ns; ++j) CHECK((L.has_obj[j] != 0) == has_obj[j] && (L.has_con[j] != 0) == has_con[j]);
    const int64_t site_counts[3] = {1, 2, 7};
    for (int64_t sites : site_counts) {
        check_offsets(L, sites, Slots::USED);
        check_offsets(L, sites, Slots::CONSTRAINED);
        check_offsets(L, sites, Slots::OBJECTIVE);
    }
    // ---- the assembly sources: every row of every block once, each from the entry it stands for
    const Offsets at = L.offsets(2, Slots::USED);
    RowSrc src[9 + 4];
    const int nsrc = fill_sources(L, at, objectives, src);
    CHECK(nsrc == (objectives ? c.nobj : 0) + L.meq + L.min);
    int next[2] = {0, 0}, next_obj = 0, next_mod[2] = {0, 0};
    for (int r = 0; r < nsrc; ++r) {
        const RowSrc &s = src[r];
        if (s.kind == 0) {
            CHECK(objectives && s.dst == next_obj && s.stride == c.k[L.obj[s.dst].slot] && s.jac == at.jac[L.obj[s.dst].slot] + L.obj[s.dst].col &&
                  s.val == at.val[L.obj[s.dst].slot] + L.obj[s.dst].col);
            ++next_obj;
            continue;
        }
        CHECK((s.eq == 0 || s.eq == 1) && s.dst == next[s.eq]);
        ++next[s.eq];
        if (s.kind == 1) {
            CHECK(s.dst < (s.eq ? n_lin_eq : n_lin_ineq) && s.val == (s.eq ? 0 : n_lin_eq) + s.dst);
        } else {
            // the next modelled row of this block, in table order
            int seen = 0, found = -1;
            for (int i = 0; i < (int)L.rows.size() && found < 0; ++i)
                if (L.rows[i].eq == (s.eq == 1) && seen++ == next_mod[s.eq]) found = i;
            CHECK(s.kind == 2 && found >= 0);
            if (found >= 0)
                CHECK(s.stride == c.k[L.rows[found].slot] && s.jac == at.jac[L.rows[found].slot] + L.rows[found].col &&
                      s.val == at.val[L.rows[found].slot] + L.rows[found].col);
            ++next_mod[s.eq];
        }
    }
    CHECK(next[1] == L.meq && next[0] == L.min);
}

// the slot defects, one at a time, on an accepted table
static void check_slot_defects(const Case &c, bool objectives) {
    describe(c, objectives);
    for (int n_starts = 1; n_starts <= 2; ++n_starts)
        for (int p = 0; p < n_starts; ++p)
            for (int j = 0; j < c.ns; ++j)
                for (int what = 0; what < 6; ++what) {
                    ++g_cases;
                    SlotShape slots[6];
                    for (int i = 0; i < n_starts * c.ns; ++i) slots[i] = SlotShape{true, D, c.k[i % c.ns], 10};
                    SlotShape &M = slots[p * c.ns + j];
                    Needs needs{objectives, Centres::EVERY_SLOT};
                    bool expect = true;
                    if (what == 0) M.present = false;
                    if (what == 1) {
                        M.d = D + 1;
                        if (p == 0 && j == 0) continue;  // slot 0 of start 0 gives d: the other slots would be the ones that differ
                    }
                    if (what == 2) {
                        M.k += 1;
                        if (p == 0) continue;  // start 0's k is the table's own shape: another table, not a defect
                    }
                    if (what >= 3) M.n = 0;
                    if (what == 4) needs.centres = Centres::UNCHECKED, expect = false;
                    Shape S;
                    S.n_slots = c.ns, S.n_starts = n_starts, S.slots = slots, S.roles = c.roles, S.n_objectives = c.nobj;
                    S.batch = n_starts > 1;
                    Layout L;
                    if (what == 5) {
                        // only the slots with constraint rows need centres
                        needs.centres = Centres::CONSTRAINED_SLOTS;
                        int e0 = 0;
                        for (int i = 0; i < j; ++i) e0 += c.k[i];
                        expect = false;
                        for (int e = e0; e < e0 + c.k[j]; ++e) expect = expect || is_con(c.roles[e]);
                    }
                    const Defect def = read(S, needs, L);
                    CHECK(expect == !!def);
                    if (def) CHECK(def.cls == Defect::MODELS && def.index == j && !def.msg.empty());
                }
    // the problem's own defects
    SlotShape slots[3];
    for (int j = 0; j < c.ns; ++j) slots[j] = SlotShape{true, D, c.k[j], 10};
    Shape S;
    S.n_slots = c.ns, S.slots = slots, S.roles = c.roles, S.n_objectives = c.nobj;
    Layout L;
    Shape T = S;
    T.n_lin_eq = -1;
    CHECK(read(T, Needs{objectives, Centres::UNCHECKED}, L).cls == Defect::PROBLEM);
    T = S, T.n_lin_ineq = 1;
    CHECK(read(T, Needs{objectives, Centres::UNCHECKED}, L).cls == Defect::PROBLEM);
    T.lin_ineq_given = true;
    CHECK(!read(T, Needs{objectives, Centres::UNCHECKED}, L));
    T = S, T.roles = nullptr;
    CHECK(read(T, Needs{objectives, Centres::UNCHECKED}, L).cls == Defect::PROBLEM);
    T = S, T.d = D + 1;  // the entry point's own d (the normal step)
    CHECK(read(T, Needs{objectives, Centres::UNCHECKED}, L).cls == Defect::MODELS);
}

static bool g_all = false;

static bool entry_defective(const Case &c, int e, bool objectives) {
    const int r = c.roles[e];
    if (r < 0) return r != MRBF_ROLE_NONE && !is_con(r);
    if (!objectives) return false;
    if (r >= c.nobj) return true;
    for (int i = 0; i < e; ++i)
        if (c.roles[i] == r) return true;
    return false;
}

static void enumerate(Case &c, int e, const int32_t *alphabet, int na, bool objectives) {
    if (e == c.ne) {
        check_case(c, objectives, (c.ne + c.nobj) % 3, c.ne % 2);
        if (c.ne <= 4) {
            // (check_case has said whether the reader accepts it; ask again here rather than keep state)
            SlotShape slots[3];
            for (int j = 0; j < c.ns; ++j) slots[j] = SlotShape{true, D, c.k[j], 10};
            Shape S;
            S.n_slots = c.ns, S.slots = slots, S.roles = c.roles, S.n_objectives = c.nobj;
            Layout L;
            if (!read(S, Needs{objectives, Centres::UNCHECKED}, L)) check_slot_defects(c, objectives);
        }
        return;
    }
    for (int a = 0; a < na; ++a) {
        c.roles[e] = alphabet[a];
        if (!g_all && c.ne > FULL && entry_defective(c, e, objectives)) {
            // the first defective entry of a long table: the entries behind it in two ways
            for (int i = e + 1; i < c.ne; ++i) c.roles[i] = MRBF_ROLE_NONE;
            check_case(c, objectives, 1, 0);
            for (int i = e + 1; i < c.ne; ++i) c.roles[i] = alphabet[(i + a) % na];
            check_case(c, objectives, 0, 2);
            continue;
        }
        enumerate(c, e + 1, alphabet, na, objectives);
    }
}

int main(int argc, char **argv) {
    g_all = argc > 1 && std::strcmp(argv[1], "--all") == 0;
    for (int objectives = 1; objectives >= 0; --objectives)
        for (int nobj = 0; nobj <= 3; ++nobj) {
            int32_t alphabet[9];
            int na = 0;
            alphabet[na++] = MRBF_ROLE_NONE, alphabet[na++] = MRBF_ROLE_EQ, alphabet[na++] = MRBF_ROLE_INEQ, alphabet[na++] = UNKNOWN;
            for (int l = 0; l <= nobj; ++l) alphabet[na++] = l;
            for (int ns = 1; ns <= 3; ++ns)
                for (int shape = 0; shape < 27; ++shape) {
                    Case c;
                    c.ns = ns, c.nobj = nobj, c.ne = 0;
                    c.k[0] = 1 + shape % 3, c.k[1] = 1 + shape / 3 % 3, c.k[2] = 1 + shape / 9;
                    if ((ns < 3 && c.k[2] != 1) || (ns < 2 && c.k[1] != 1)) continue;  // the slots that are not there: once
                    for (int j = 0; j < ns; ++j) c.ne += c.k[j];
                    if (!g_all && !objectives && c.ne > FULL) {
                        // read without objective rows no non-negative entry is a defect: one of them stands for all, at one n_objectives
                        if (nobj == 1) enumerate(c, 0, alphabet, 5, false);
                        continue;
                    }
                    enumerate(c, 0, alphabet, na, objectives != 0);
                }
        }
    if (g_failed) std::printf("descent_problem_check: %d check(s) FAILED\n", g_failed);
    else std::printf("descent_problem_check: ok (%ld cases, %ld accepted%s)\n", g_cases, g_accepted, g_all ? ", every table in full" : "");
    return g_failed ? 1 : 0;
}
