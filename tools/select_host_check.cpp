// Stand-alone host check of the host logic of the two batched selection calls that have no database behind them: the affine filter's
// pick loop (morbit.jl_amd/csrc/affine_host.hpp) and round 4 for small starts (morbit.jl_amd/csrc/round4_host.hpp) -- the validation
// of a batch's jobs, the counts, the routing and the layout of each call's arena.  Every case is judged by statements made directly
// from the headers' comments and from include/mrbf.h, not by a second call of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/select_host_check.cpp -o /tmp/select_host_check && /tmp/select_host_check
// Enumerated: batches of 1 .. 4 starts (a stride through the combinations of the larger ones), d in {1, 2, 8}, mc in {0, 1, 9}, j0 in
// {0, 1, d}, max_picks in {0, 1, d + 3}, poly_deg in {-1, 0, 1}, n0 in {q - 1, q, q + 3}, max_points in {default, n0, n0 + 1}; every
// defect in every position, alone, before a later job's defect and before a later defect of the same job; the caps of the affine batch;
// every limit of round 4's small range at the limit and one beyond; the arena limit reached by adding one start.
#include <cstdio>
#include <cstring>
#include <string>

#include "../morbit.jl_amd/csrc/affine_host.hpp"
#include "../morbit.jl_amd/csrc/round4_host.hpp"

using namespace mrbf;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static double g_mem[4];        // something for the pointers of a job to point at: never read
static int64_t g_picks[4];
static int32_t g_acc[4];
static size_t up(size_t b) { return (b + 255) / 256 * 256; }  // "every piece a multiple of 256 bytes"
static bool names(const Defect &D, size_t p, const char *field) {
    char job[32];
    std::snprintf(job, sizeof(job), "jobs[%zu]", p);
    return D.msg.find(job) != std::string::npos && D.msg.find(field) != std::string::npos;
}
// the pieces `at` (n of them, then the end) are in order, 256-byte multiples, each with room for `need`
static void check_pieces(const size_t *at, const size_t *need, int n) {
    for (int i = 0; i < n; ++i) CHECK(at[i] % 256 == 0 && at[i] + need[i] <= at[i + 1]);
    CHECK(at[n] % 256 == 0);
}

// ---------------------------------------------------------------------------------------------------------------- the affine batch
static mrbf_affine_job affine_job(int64_t mc, int j0, int max_picks) {
    mrbf_affine_job jb;
    std::memset(&jb, 0, sizeof(jb));
    jb.mc = mc, jb.j0 = j0, jb.max_picks = max_picks, jb.pivot_val = 0.5;
    jb.shifted = g_mem, jb.Q0 = g_mem, jb.picked_out = g_picks;
    return jb;
}

// "want[p] = mc > 0 ? min(max_picks, d - j0) : 0", "T = max want[p]", "ngrp_max = max ceil(mc / AFF_G) over the starts with want[p] > 0";
// the arena "state | picks | hv | descriptors | Q | Zs | val | C | S", "state and picks come back in one copy", "descriptors and start
// bases go up in one"
static void check_affine_valid() {
    const size_t desc = 88;
    for (int d : {1, 2, 8})
        for (int ns = 1; ns <= 4; ++ns) {
            long total = 1;
            for (int i = 0; i < ns; ++i) total *= 27;
            for (long code = 0; code < total; code += (ns == 4 ? 7 : 1)) {
                mrbf_affine_job jobs[4];
                const int64_t mcs[] = {0, 1, 9};
                const int j0s[] = {0, 1, d}, mps[] = {0, 1, d + 3};
                long c = code;
                for (int p = 0; p < ns; ++p, c /= 27) jobs[p] = affine_job(mcs[c % 3], j0s[c / 3 % 3], mps[c / 9 % 3]);
                const affine::Plan P = affine::plan(ns, d, jobs, desc, 5);
                ++g_cases;
                CHECK(P.bad.code == 0 && P.bad.msg.empty());
                int T = 0;
                int64_t ngrp = 0, sum = 0;
                for (int p = 0; p < ns; ++p) {
                    const int want = jobs[p].mc > 0 ? std::min(jobs[p].max_picks, d - jobs[p].j0) : 0;
                    CHECK(P.want[(size_t)p] == want);
                    T = std::max(T, want);
                    if (want > 0) ngrp = std::max(ngrp, (jobs[p].mc + 7) / 8);
                    sum += jobs[p].mc;
                }
                CHECK(P.T == T && P.ngrp_max == ngrp && P.mc_sum == sum);
                const affine::Plan &L = P;
                const size_t N = (size_t)ns, D = (size_t)d, M = (size_t)std::max<int64_t>(sum, 1);
                CHECK(L.hvn == 2 * D + 8);
                const size_t at[] = {L.oState, L.oPicks, L.oHv, L.oDesc, L.oQ, L.oZs, L.oVal, L.oC, L.oS, L.A.total};
                const size_t need[] = {N * 16, N * D * 8, N * (2 * D + 8) * 8, N * desc, N * D * D * 8, N * D * D * 8, M * 8, M * D * 8, M * D * 8};
                CHECK(at[0] == 0);
                check_pieces(at, need, 9);
                CHECK(L.A.back_at == L.oState && L.A.back_end == L.oHv && L.A.back_bytes() == L.oHv - L.oState);
                CHECK(L.A.up_at == L.oDesc && L.A.up_end == L.oZs && L.A.upload_bytes() == L.oZs - L.oDesc);
            }
        }
}

// "an invalid field of a job is an invalid `jobs` (-5)"; the first defect in job order wins, within a job the first of: mc, j0, Q0,
// max_picks, shifted, picked_out
static const char *affine_break(mrbf_affine_job &jb, int kind, int d) {
    switch (kind) {
        case 0: jb.mc = -1; return ".mc";
        case 1: jb.mc = ((int64_t)1 << 26) + 1; return ".mc";
        case 2: jb.j0 = -1; return ".j0";
        case 3: jb.j0 = d + 1; return ".j0";
        case 4: jb.j0 = 1, jb.Q0 = nullptr; return ".Q0";
        case 5: jb.max_picks = -1; return ".max_picks";
        case 6: jb.shifted = nullptr; return ".shifted";
        default: jb.picked_out = nullptr; return ".picked_out";
    }
}
static void check_affine_defects() {
    const int kinds = 8;
    const size_t desc = 88;
    for (int d : {1, 2, 8})
        for (int ns = 1; ns <= 4; ++ns)
            for (int at = 0; at < ns; ++at)
                for (int kind = 0; kind < kinds; ++kind)
                    for (int later_at = at; later_at < ns; ++later_at)
                        for (int later = -1; later < kinds; ++later) {
                            // a second defect: a later kind of the same job (kinds are numbered in the order of the checks; the two
                            // defects of one field exclude each other), or any kind of a later job; -1: none
                            if (later_at == at && later >= 0 && (later <= kind || (kind == 0 && later == 1) || ((kind == 2 || kind == 3) && later <= 4))) continue;
                            if (later_at > at && later < 0) continue;
                            mrbf_affine_job jobs[4];
                            for (int p = 0; p < ns; ++p) jobs[p] = affine_job(9, 0, 1);
                            const char *field = affine_break(jobs[at], kind, d);
                            if (later >= 0) affine_break(jobs[later_at], later, d);
                            const affine::Plan P = affine::plan(ns, d, jobs, desc, 5);
                            ++g_cases;
                            CHECK(P.bad.code == -5);
                            CHECK(names(P.bad, (size_t)at, field));
                        }
    // "At most 2^26 candidates in all": a start of 2^26 alone and two of 2^25 are inside, one more candidate anywhere is not -- and that
    // is reported as -5 too, behind the field checks of the job at which the sum passes the cap
    const int64_t cap = (int64_t)1 << 26;
    mrbf_affine_job jobs[3] = {affine_job(cap, 0, 1), affine_job(0, 0, 1), affine_job(0, 0, 1)};
    CHECK(affine::plan(1, 2, jobs, 88, 5).bad.code == 0 && affine::plan(3, 2, jobs, 88, 5).bad.code == 0);
    jobs[2].mc = 1;
    CHECK(affine::plan(3, 2, jobs, 88, 5).bad.code == -5 && affine::plan(2, 2, jobs, 88, 5).bad.code == 0);
    jobs[2].shifted = nullptr;  // the third job's own field defect comes first
    CHECK(names(affine::plan(3, 2, jobs, 88, 5).bad, 2, ".shifted"));
    jobs[0].mc = jobs[1].mc = cap / 2, jobs[2] = affine_job(0, 0, 1);
    CHECK(affine::plan(3, 2, jobs, 88, 5).bad.code == 0 && affine::plan(3, 2, jobs, 88, 5).mc_sum == cap);
    jobs[1].mc = cap / 2 + 1;
    CHECK(affine::plan(3, 2, jobs, 88, 5).bad.code == -5 && affine::plan(1, 2, jobs, 88, 5).bad.code == 0);
    g_cases += 8;
}

// -------------------------------------------------------------------------------------------------------------------------- round 4
static mrbf_round4_job round4_job(int64_t n0, int64_t mc, int poly_deg, int max_points) {
    mrbf_round4_job jb;
    std::memset(&jb, 0, sizeof(jb));
    jb.n0 = n0, jb.mc = mc, jb.poly_deg = poly_deg, jb.max_points = max_points, jb.kernel_id = 1, jb.a = 1.0, jb.b = 0.5;
    jb.theta_pivot_cholesky = 1e-7;
    jb.start_sites = g_mem, jb.cand_sites = g_mem, jb.accepted_out = g_acc;
    return jb;
}
// what the header says of one start: the tail's terms, "cap = min(mc, max_points - n0)" with "max_points <= 0: (d + 1)(d + 2) / 2", and
// its route while it is inside the small range and the arena has room
struct Expect {
    int q, route;
    int64_t cap;
};
static Expect expect_of(const mrbf_round4_job &jb, int d) {
    Expect e;
    e.q = jb.poly_deg < 0 ? 0 : (jb.poly_deg == 0 ? 1 : d + 1);
    const int64_t mp = jb.max_points <= 0 ? (int64_t)(d + 1) * (d + 2) / 2 : jb.max_points;
    e.cap = std::min<int64_t>(jb.mc, mp - jb.n0);
    e.route = jb.n0 < e.q ? r4s::SINGLE : ((jb.mc == 0 || e.cap <= 0) ? r4s::DONE : r4s::BATCHED);
    return e;
}
// the slices of a BATCHED start: "X0 | Xc | XcT | Ginv | Phi00 | T | Lam | U | RK | RH", "Ginv and T at least one", "without a tail
// (q = 0) ... RH is RK"; returns the end of the start's slices
static size_t check_slices(const r4s::Start &st, const mrbf_round4_job &jb, int d, const Expect &e, size_t begin) {
    const size_t n0 = (size_t)jb.n0, mc = (size_t)jb.mc, D = (size_t)d, Q = (size_t)e.q, C = (size_t)e.cap;
    const size_t rk_end = st.RK + up(C * mc * 8);
    CHECK((st.RH == st.RK) == (e.q == 0));
    if (e.q > 0) CHECK(st.RH >= rk_end);
    const size_t end = e.q > 0 ? st.RH + up(C * mc * 8) : rk_end;
    const size_t at[] = {st.X0, st.Xc, st.XcT, st.Ginv, st.Phi00, st.T, st.Lam, st.U, st.RK, end};
    const size_t need[] = {n0 * D * 8, mc * D * 8, mc * D * 8, std::max<size_t>(Q * Q, 1) * 8, n0 * n0 * 8, std::max<size_t>(Q * mc, 1) * 8,
                           n0 * mc * 8, n0 * mc * 8, C * mc * 8};
    CHECK(at[0] >= begin);
    check_pieces(at, need, 9);
    CHECK(st.RH % 256 == 0);
    return end;
}
// the whole plan of a valid batch inside the small range
static void check_round4_plan(const r4s::Plan &P, int ns, int d, const mrbf_round4_job *jobs, size_t desc) {
    ++g_cases;
    CHECK(P.bad.code == 0 && P.bad.msg.empty());
    size_t nb = 0, end = 0;
    int cap_max = 0, q_max = 0;
    int64_t mc_max = 0, n0_max = 0;
    for (int p = 0; p < ns; ++p) {
        const Expect e = expect_of(jobs[p], d);
        const r4s::Start &st = P.st[(size_t)p];
        CHECK(st.q == e.q && st.route == e.route);
        if (e.route != r4s::BATCHED) continue;
        CHECK(st.cap == e.cap);
        end = check_slices(st, jobs[p], d, e, end);  // the starts' slices follow each other in job order: disjoint
        ++nb;
        cap_max = std::max(cap_max, (int)e.cap), q_max = std::max(q_max, e.q);
        mc_max = std::max(mc_max, jobs[p].mc), n0_max = std::max(n0_max, jobs[p].n0);
    }
    CHECK(P.nb == nb && P.cap_max == cap_max && P.q_max == q_max && P.mc_max == mc_max && P.n0_max == n0_max);
    CHECK(P.ostride == (size_t)cap_max + 2);  // "ostride = cap_max + 2": count, flag, list
    // "output words (the read-back) | descriptors (the upload) | the starts' slices"
    const size_t at[] = {P.oOut, P.oDesc, P.oSlices, P.A.total};
    const size_t need[] = {nb * P.ostride * 4, nb * desc, end};
    CHECK(at[0] == 0);
    check_pieces(at, need, 3);
    CHECK(P.A.back_at == P.oOut && P.A.back_end == P.oDesc && P.A.up_at == P.oDesc && P.A.up_end == P.oSlices);
    CHECK(end <= r4s::R4S_ARENA_MAX);
}

static void check_round4_valid() {
    const size_t desc = 152;
    for (int d : {1, 2, 8})
        for (int ns = 1; ns <= 4; ++ns) {
            long total = 1;
            for (int i = 0; i < ns; ++i) total *= 81;
            const long step = ns == 1 ? 1 : (ns == 2 ? 1 : (ns == 3 ? 5 : 401));
            for (long code = 0; code < total; code += step) {
                mrbf_round4_job jobs[4];
                long c = code;
                for (int p = 0; p < ns; ++p, c /= 81) {
                    const int64_t mcs[] = {0, 1, 9};
                    const int deg = (int)(c / 3 % 3) - 1, q = deg < 0 ? 0 : (deg == 0 ? 1 : d + 1);
                    const int64_t n0s[] = {std::max(q - 1, 1), std::max(q, 1), q + 3};  // either side of n0 = q wherever q - 1 is a valid n0
                    const int64_t n0 = n0s[c / 9 % 3];
                    const int mps[] = {0, (int)n0, (int)n0 + 1};                         // default; cap = 0; cap = 1 (where mc >= 1)
                    jobs[p] = round4_job(n0, mcs[c % 3], deg, mps[c / 27 % 3]);
                }
                check_round4_plan(r4s::plan(ns, d, jobs, desc, 4), ns, d, jobs, desc);
            }
        }
    // the boundaries by name: n0 = q - 1 / q; cap = 0 / 1
    {
        mrbf_round4_job jb = round4_job(8, 9, 1, 0);  // d = 8, degree 1: q = 9
        CHECK(r4s::plan(1, 8, &jb, desc, 4).st[0].route == r4s::SINGLE);
        jb.n0 = 9;
        CHECK(r4s::plan(1, 8, &jb, desc, 4).st[0].route == r4s::BATCHED);
        jb.max_points = 9;
        CHECK(r4s::plan(1, 8, &jb, desc, 4).st[0].route == r4s::DONE);
        jb.max_points = 10;
        CHECK(r4s::plan(1, 8, &jb, desc, 4).st[0].route == r4s::BATCHED && r4s::plan(1, 8, &jb, desc, 4).st[0].cap == 1);
        g_cases += 4;
    }
    // "d <= 128, q <= n0 <= 256, 1 <= mc <= 4096, min(mc, max_points - n0) <= 256": at each limit BATCHED, one beyond SINGLE
    {
        struct Case {
            int d;
            int64_t n0, mc;
            int acc;
            int route;
        };
        const Case cases[] = {{128, 256, 4096, 256, r4s::BATCHED}, {129, 256, 4096, 256, r4s::SINGLE}, {128, 257, 4096, 256, r4s::SINGLE},
                              {128, 256, 4097, 256, r4s::SINGLE},  {128, 256, 4096, 257, r4s::SINGLE}, {128, 256, 257, 257, r4s::SINGLE},
                              {128, 256, 256, 257, r4s::BATCHED}};  // (the last: 257 allowed, 256 candidates: cap = 256)
        for (const Case &c : cases) {
            mrbf_round4_job jb = round4_job(c.n0, c.mc, 1, (int)c.n0 + c.acc);
            const r4s::Plan P = r4s::plan(1, c.d, &jb, desc, 4);
            ++g_cases;
            CHECK(P.bad.code == 0 && P.st[0].route == c.route);
            if (c.route == r4s::BATCHED) check_round4_plan(P, 1, c.d, &jb, desc);
        }
    }
    // "at most 2 GiB of workspace for the batch": with starts of the largest shape, the last start that fits is BATCHED, the next one
    // takes the single call, and a small start behind it still finds room
    {
        const int d = 128;
        const size_t n0 = 256, mc = 4096, q = 129, acc = 256;
        const size_t need = up(n0 * d * 8) + 2 * up(mc * d * 8) + up(q * q * 8) + up(n0 * n0 * 8) + up(q * mc * 8) + 2 * up(n0 * mc * 8) + 2 * up(acc * mc * 8);
        const int fit = (int)(r4s::R4S_ARENA_MAX / need);
        std::vector<mrbf_round4_job> jobs((size_t)fit + 2, round4_job(256, 4096, 1, 512));
        jobs.back() = round4_job(3, 9, -1, 0);
        const r4s::Plan A = r4s::plan(fit, d, jobs.data(), desc, 4), B = r4s::plan(fit + 2, d, jobs.data(), desc, 4);
        g_cases += 2;
        CHECK(A.nb == (size_t)fit && B.nb == (size_t)fit + 1);
        for (int p = 0; p < fit; ++p) CHECK(A.st[(size_t)p].route == r4s::BATCHED && B.st[(size_t)p].route == r4s::BATCHED);
        CHECK(B.st[(size_t)fit].route == r4s::SINGLE && B.st[(size_t)fit + 1].route == r4s::BATCHED);
        CHECK(A.A.total - A.oSlices == (size_t)fit * need && A.A.total - A.oSlices <= r4s::R4S_ARENA_MAX && (size_t)(fit + 1) * need > r4s::R4S_ARENA_MAX);
        // the slices of the small start lie behind those of the last large one
        CHECK(B.st[(size_t)fit + 1].X0 == (size_t)fit * need);
    }
}

// "an invalid field of a job is an invalid `jobs`: -4"; the first defect in job order wins, within a job the first of: n0, mc,
// start_sites, cand_sites, kernel_id, poly_deg, accepted_out
static const char *round4_break(mrbf_round4_job &jb, int kind) {
    switch (kind) {
        case 0: jb.n0 = 0; return ".n0";
        case 1: jb.mc = -1; return ".mc";
        case 2: jb.start_sites = nullptr; return ".start_sites";
        case 3: jb.cand_sites = nullptr; return ".cand_sites";
        case 4: jb.kernel_id = -1; return ".kernel_id";
        case 5: jb.kernel_id = 5; return ".kernel_id";
        case 6: jb.poly_deg = -2; return ".poly_deg";
        case 7: jb.poly_deg = 2; return ".poly_deg";
        default: jb.accepted_out = nullptr; return ".accepted_out";
    }
}
static void check_round4_defects() {
    const int kinds = 9;
    for (int d : {1, 2, 8})
        for (int ns = 1; ns <= 4; ++ns)
            for (int at = 0; at < ns; ++at)
                for (int kind = 0; kind < kinds; ++kind)
                    for (int later_at = at; later_at < ns; ++later_at)
                        for (int later = -1; later < kinds; ++later) {
                            // a second defect: as for the affine batch
                            if (later_at == at && later >= 0 && (later <= kind || (kind == 4 && later == 5) || (kind == 6 && later == 7))) continue;
                            if (later_at > at && later < 0) continue;
                            mrbf_round4_job jobs[4];
                            for (int p = 0; p < ns; ++p) jobs[p] = round4_job(d + 2, 9, 1, d + 7);  // cap = 5
                            const char *field = round4_break(jobs[at], kind);
                            if (later >= 0) round4_break(jobs[later_at], later);
                            const r4s::Plan P = r4s::plan(ns, d, jobs, 152, 4);
                            ++g_cases;
                            CHECK(P.bad.code == -4);
                            CHECK(names(P.bad, (size_t)at, field));
                        }
    // no candidates need no pointer; no site to accept needs no list
    mrbf_round4_job jb = round4_job(3, 0, -1, 0);
    jb.cand_sites = nullptr, jb.accepted_out = nullptr;
    CHECK(r4s::plan(1, 2, &jb, 152, 4).bad.code == 0);
    jb = round4_job(3, 9, -1, 3);
    jb.accepted_out = nullptr;
    CHECK(r4s::plan(1, 2, &jb, 152, 4).bad.code == 0 && r4s::plan(1, 2, &jb, 152, 4).st[0].route == r4s::DONE);
    g_cases += 2;
}

int main() {
    check_affine_valid();
    check_affine_defects();
    check_round4_valid();
    check_round4_defects();
    if (g_failed) {
        std::printf("select_host_check: %d checks FAILED in %ld cases\n", g_failed, g_cases);
        return 1;
    }
    std::printf("select_host_check: ok (%ld cases)\n", g_cases);
    return 0;
}
