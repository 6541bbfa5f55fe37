// Stand-alone host check of the many-start directed-search call's host logic (morbit.jl_amd/csrc/ds_batch_host.hpp): the validation
// behind mrbf_ds_iterate_batch's return codes, the layout of the chain's arena, and the record packing.  Every case is judged by
// statements made directly from the header's text (include/mrbf.h "many-start directed search" and the comments of ds_batch_host.hpp),
// not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/ds_batch_host_check.cpp -o /tmp/ds_batch_host_check && /tmp/ds_batch_host_check
// Enumerated: every defect of a call alone and in pairs (the order of the codes), NULL for each argument, start counts on either side of
// 1 .. 65535 and overflow-sized ones; the layout over n_starts in {1, 2, 5, 33, 64, 65535}, d in {1, 2, 7, 65, 128, 256}, k in {1, 2,
// 3, 16}, max_loops in {0, 6, 117, 1024} and 1 .. 3 models (walked piece by piece in a buffer of its size under AddressSanitizer where
// that buffer is small); the record of every start of a packed read-back.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../morbit.jl_amd/csrc/ds_batch_host.hpp"

using namespace mrbf::dsbatch;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static Call good_call() {
    Call c;
    c.has_ctx = true;
    c.n_starts = 33;
    c.shape = c.models = c.x = c.x_n = c.delta = c.lb = c.ub = c.r = c.opts = true;
    c.d_out = c.x_plus = c.mx_plus = c.records = true;
    c.shrink = 0.75, c.n_models = 2, c.roles = true;
    return c;
}

// defects in the order validate() looks for them: the earlier one wins when two are present
enum Defect { NO_CTX, NO_SHAPE, NO_MODELS, NO_X, NO_XN, NO_DELTA, NO_LB, NO_UB, NO_R, NO_OPTS, NO_DOUT, NO_XPLUS, NO_MXPLUS, NO_RECORDS,
              BAD_SHRINK, NO_ROLES, BAD_STARTS, N_DEFECTS };
static const int CODE[N_DEFECTS] = {-1, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12, -13, -14, -15, -11, -3, -2};

static void apply(Call &c, int defect) {
    switch (defect) {
        case NO_CTX: c.has_ctx = false; break;
        case NO_SHAPE: c.shape = false; break;
        case NO_MODELS: c.models = false; break;
        case NO_X: c.x = false; break;
        case NO_XN: c.x_n = false; break;
        case NO_DELTA: c.delta = false; break;
        case NO_LB: c.lb = false; break;
        case NO_UB: c.ub = false; break;
        case NO_R: c.r = false; break;
        case NO_OPTS: c.opts = false; break;
        case NO_DOUT: c.d_out = false; break;
        case NO_XPLUS: c.x_plus = false; break;
        case NO_MXPLUS: c.mx_plus = false; break;
        case NO_RECORDS: c.records = false; break;
        case BAD_SHRINK: c.shrink = 1.0; break;
        case NO_ROLES: c.roles = false; break;
        case BAD_STARTS: c.n_starts = 0; break;
    }
}

static void check_validate() {
    CHECK(validate(good_call()) == 0);
    for (int a = 0; a < N_DEFECTS; ++a) {
        Call c = good_call();
        apply(c, a);
        ++g_cases;
        CHECK(validate(c) == CODE[a]);
        for (int b = a + 1; b < N_DEFECTS; ++b) {
            Call c2 = good_call();
            apply(c2, a), apply(c2, b);
            ++g_cases;
            CHECK(validate(c2) == CODE[a]);
        }
    }
    // "-1 no context" whatever else is missing
    Call none;
    CHECK(validate(none) == -1);
    // "1 <= n_starts <= 65535"; beyond it, overflow-sized counts included, the table's answer -2 and nothing else is looked at
    CHECK(MAX_STARTS == 65535);
    Call c = good_call();
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)65535}) {
        c.n_starts = n;
        ++g_cases;
        CHECK(validate(c) == 0);
    }
    for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)65536, (int64_t)1 << 31, (int64_t)1 << 40, ((int64_t)1 << 62) + 5,
                      std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
        c.n_starts = n;
        ++g_cases;
        CHECK(validate(c) == -2);
    }
    // "shrink outside (0, 1)": the ends and a NaN
    c = good_call();
    for (double s : {0.0, 1.0, -0.5, 1.5, std::nan("")}) {
        c.shrink = s;
        ++g_cases;
        CHECK(validate(c) == -11);
    }
    c.shrink = 0.5, c.n_models = 0;
    CHECK(validate(c) == -3);
}

// "Every offset is a multiple of 16; [0, up_cnt) is the one upload, [out0, out0 + out_cnt) the one read-back"; nothing overlaps
static void check_layout() {
    for (int64_t N : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)33, (int64_t)64, (int64_t)65535})
        for (int d : {1, 2, 7, 65, 128, 256})
            for (int k : {1, 2, 3, 16})
                for (int loops : {0, 6, 117, 1024})
                    for (int nm = 1; nm <= 3; ++nm) {
                        if (nm > k) continue;  // every model carries at least one objective row here
                        Sizes s;
                        s.n_starts = N, s.d = d, s.k = k, s.max_loops = loops;
                        s.jtot = (size_t)k * d, s.otot = (size_t)(loops + 2) * k;
                        s.desc_dbl = (size_t)2 * N * nm * 23 + 1;  // an odd count: the padding is the layout's
                        s.scratch = (size_t)N * nm * 64 * ((size_t)d + 1);
                        const Layout L = layout(s);
                        ++g_cases;
                        const size_t SN = (size_t)N, sd = (size_t)d, sk = (size_t)k, sl = (size_t)loops;
                        const size_t off[] = {L.pairs, L.delta, L.lb, L.ub, L.r, L.desc, L.J, L.G, L.draw, L.z, L.omega_step, L.steps, L.sig,
                                              L.X, L.VO, L.scratch, L.xp, L.mxp, L.tail, L.dir, L.mult, L.omega, L.dnorm, L.ints, L.total};
                        const size_t need[] = {SN * 2 * sd, SN, sd, sd, SN * sk, s.desc_dbl, SN * s.jtot, SN * sk * sd, SN * sd, SN * sk, SN,
                                               SN * (sl + 1), SN * 2, SN * (sl + 2) * sd, SN * s.otot, s.scratch, SN * sd, SN * sk, SN * TAIL,
                                               SN * sd, SN * sk, SN, SN, ints_doubles(SN)};
                        const int pieces = (int)(sizeof(need) / sizeof(need[0]));
                        CHECK(off[0] == 0);
                        for (int i = 0; i < pieces; ++i) {
                            CHECK(off[i] % 16 == 0);
                            CHECK(off[i] + need[i] <= off[i + 1]);        // in the order listed: no overlap
                            CHECK(off[i + 1] - off[i] < need[i] + 16);    // and no more than the padding in between
                        }
                        CHECK(L.up_cnt == L.J && L.desc + s.desc_dbl <= L.up_cnt);            // the upload ends where the work begins
                        CHECK(L.out0 == L.xp && L.out0 + L.out_cnt == L.total);               // the read-back is the arena's end
                        CHECK(L.scratch + s.scratch <= L.out0);
                        CHECK(ints_doubles(SN) * sizeof(double) >= 3 * SN * sizeof(int32_t));  // status + (iterations, dropped)
                        // walk it: every piece written to its end inside a buffer of exactly L.total doubles
                        if (L.total > ((size_t)1 << 19)) continue;
                        std::vector<double> buf(L.total, 0.0);
                        for (int i = 0; i < pieces; ++i)
                            for (size_t j = 0; j < need[i]; ++j) buf[off[i] + j] += 1.0;
                        bool once = true;
                        for (int i = 0; i < pieces && once; ++i)
                            for (size_t j = 0; j < need[i]; ++j) once = once && buf[off[i] + j] == 1.0;
                        CHECK(once);
                    }
}

// "start p's record from the read-back: the status words of all starts, then (iterations, dropped) per start"; the tail's order is
// [omega_step, step_norm, loops, sigma, branch]
static void check_pack() {
    CHECK(sizeof(mrbf_ds_batch_record) == 64 && TAIL == 5);
    for (size_t N : {(size_t)1, (size_t)5, (size_t)33}) {
        std::vector<int32_t> ints(3 * N);
        std::vector<double> tail(N * TAIL), omega(N), dnorm(N);
        for (size_t p = 0; p < N; ++p) {
            ints[p] = (int32_t)(p % 4), ints[N + 2 * p] = (int32_t)(10 + p), ints[N + 2 * p + 1] = (int32_t)(100 + p);
            tail[p * TAIL + 0] = 0.5 + p, tail[p * TAIL + 1] = 0.25 * (p + 1), tail[p * TAIL + 2] = (double)(p % 7), tail[p * TAIL + 3] = 0.125 + p;
            tail[p * TAIL + 4] = (double)(p % 3);
            omega[p] = p % 4 == 2 ? -std::numeric_limits<double>::infinity() : 1.5 + p;
            dnorm[p] = 2.0 + p;
        }
        for (size_t p = 0; p < N; ++p) {
            mrbf_ds_batch_record R;
            std::memset(&R, 0xff, sizeof(R));
            pack(R, p, N, ints.data(), tail.data(), omega.data(), dnorm.data());
            ++g_cases;
            CHECK(R.ds_status == (int32_t)(p % 4) && R.iterations == (int32_t)(10 + p) && R.dropped == (int32_t)(100 + p));
            CHECK(R.branch == (int32_t)(p % 3) && R.loops == (int32_t)(p % 7) && R.reserved == 0);
            CHECK(R.omega == omega[p] && R.omega_step == 0.5 + p && R.step_norm == 0.25 * (p + 1) && R.sigma == 0.125 + p && R.dnorm == 2.0 + p);
        }
    }
}

int main() {
    check_validate();
    check_layout();
    check_pack();
    std::printf("ds_batch_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("ds_batch_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
