// Stand-alone host check of the local-ideal-point calls' host logic (morbit.jl_amd/csrc/ideal_host.hpp): the validation behind the
// return codes of mrbf_ideal_point_problem / mrbf_ideal_point_batch, the layout of the block the outputs are gathered in, and the
// record packing.  Every case is judged by statements made directly from the header's text (include/mrbf.h "local ideal points" and
// the comments of ideal_host.hpp), not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/ideal_host_check.cpp -o /tmp/ideal_host_check && /tmp/ideal_host_check
// Enumerated: every defect of a call alone and in pairs (the order of the codes), for the single and the batch call; start counts on
// either side of 1 .. 65535 and overflow-sized ones; the layout for d in 1 .. 256, k in 1 .. 8 and n_starts in {1, 2, 5, 9, 64}
// (walked piece by piece in a buffer of its size under AddressSanitizer) and at 65535 starts (arithmetic only); the record of every
// found / refined pattern of 1 .. 8 objectives.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../morbit.jl_amd/csrc/ideal_host.hpp"

using namespace mrbf::ideal;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static Call good_call(bool batch) {
    Call c;
    c.has_ctx = true;
    c.batch = batch;
    c.n_starts = batch ? 33 : 1;
    c.problem = c.models = c.x_n = c.lb = c.ub = c.opts = c.ideal_out = c.info = true;
    c.n_models = 2, c.roles = true;
    return c;
}

// defects in the order validate() looks for them: the earlier one wins when two are present
enum Defect { NO_CTX, NO_PROBLEM, NO_MODELS, NO_XN, NO_LB, NO_UB, NO_OPTS, NO_IDEAL, NO_INFO, NO_ROLES, BAD_STARTS, N_DEFECTS };
// "-4 NULL models (the batch; the single call's handles are the problem's, hence -3)"
static int code(int defect, bool batch) {
    static const int CODE[N_DEFECTS] = {-1, -3, -4, -5, -6, -7, -8, -9, -10, -3, -2};
    return defect == NO_MODELS && !batch ? -3 : CODE[defect];
}

static void apply(Call &c, int defect) {
    switch (defect) {
        case NO_CTX: c.has_ctx = false; break;
        case NO_PROBLEM: c.problem = false; break;
        case NO_MODELS: c.models = false; break;
        case NO_XN: c.x_n = false; break;
        case NO_LB: c.lb = false; break;
        case NO_UB: c.ub = false; break;
        case NO_OPTS: c.opts = false; break;
        case NO_IDEAL: c.ideal_out = false; break;
        case NO_INFO: c.info = false; break;
        case NO_ROLES: c.roles = false; break;
        case BAD_STARTS: c.n_starts = 0; break;
    }
}

static void check_validate() {
    for (bool batch : {false, true}) {
        CHECK(validate(good_call(batch)) == 0);
        // (the single call has no start count: BAD_STARTS is the batch's defect)
        const int nd = batch ? N_DEFECTS : BAD_STARTS;
        for (int a = 0; a < nd; ++a) {
            Call c = good_call(batch);
            apply(c, a);
            ++g_cases;
            CHECK(validate(c) == code(a, batch));
            for (int b = a + 1; b < nd; ++b) {
                Call c2 = good_call(batch);
                apply(c2, a), apply(c2, b);
                ++g_cases;
                CHECK(validate(c2) == code(a, batch));
            }
        }
        // "-1 no context" whatever else is missing
        Call none;
        none.batch = batch;
        CHECK(validate(none) == -1);
        Call c = good_call(batch);
        c.n_models = 0;
        CHECK(validate(c) == -3);
        c.n_models = -4;
        CHECK(validate(c) == -3);
    }
    // "-2 for a start count outside 1 .. MAX_STARTS", overflow-sized counts included; nothing else is looked at behind it
    CHECK(MAX_STARTS == 65535);
    Call c = good_call(true);
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
    // the single call does not read the count
    Call s = good_call(false);
    s.n_starts = 0;
    CHECK(validate(s) == 0);
}

// "[ideal: n_starts x k][mx: n_starts x k][x_ideal: n_starts x k x d]": the pieces in that order, nothing between them, every
// (start, objective) entry inside its piece
static void check_layout() {
    for (int64_t N : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)9, (int64_t)64, (int64_t)65535})
        for (int d = 1; d <= 256; ++d)
            for (int k = 1; k <= 8; ++k) {
                const Layout L = layout(N, d, k);
                ++g_cases;
                const size_t SN = (size_t)N, sd = (size_t)d, sk = (size_t)k;
                CHECK(L.ideal == 0 && L.mx == SN * sk && L.x_ideal == 2 * SN * sk && L.total == SN * sk * (2 + sd));
                CHECK(L.ideal_at(0, 0) == L.ideal && L.mx_at(0, 0) == L.mx && L.x_ideal_at(0, 0) == L.x_ideal);
                CHECK(L.ideal_at(SN - 1, sk - 1) + 1 == L.mx && L.mx_at(SN - 1, sk - 1) + 1 == L.x_ideal);
                CHECK(L.x_ideal_at(SN - 1, sk - 1) + sd == L.total);
                if (N > 64) continue;
                // walk it: every entry written once inside a buffer of exactly L.total doubles
                std::vector<double> buf(L.total, 0.0);
                for (size_t p = 0; p < SN; ++p)
                    for (size_t l = 0; l < sk; ++l) {
                        buf[L.ideal_at(p, l)] += 1.0;
                        buf[L.mx_at(p, l)] += 1.0;
                        for (size_t t = 0; t < sd; ++t) buf[L.x_ideal_at(p, l) + t] += 1.0;
                    }
                bool once = true;
                for (double v : buf) once = once && v == 1.0;
                CHECK(once);
                // a start's k entries are contiguous, the starts follow each other: the piece is the caller's array as it is
                if (SN > 1) CHECK(L.ideal_at(1, 0) == L.ideal_at(0, 0) + sk && L.x_ideal_at(1, 0) == L.x_ideal_at(0, 0) + sk * sd);
            }
}

// "found[l] / refined[l] != 0 -> bit l of the masks"
static void check_pack() {
    CHECK(sizeof(mrbf_ideal_info) == 20 && MAX_OBJECTIVES == 8);
    for (int k = 1; k <= MAX_OBJECTIVES; ++k)
        for (int fm = 0; fm < (1 << k); ++fm)
            for (int rm : {0, fm, fm & 0x55, (1 << k) - 1}) {
                char found[MAX_OBJECTIVES], refined[MAX_OBJECTIVES];
                for (int l = 0; l < k; ++l) found[l] = (char)((fm >> l) & 1), refined[l] = (char)(((rm >> l) & 1) ? 7 : 0);
                mrbf_ideal_info I;
                std::memset(&I, 0xff, sizeof(I));
                pack(I, k, 1000 + k, 17 * k, found, refined);
                ++g_cases;
                CHECK(I.evals_ideal == 1000 + k && I.generations == 17 * k && I.found == fm && I.refined == rm && I.ms_total == 0.f);
            }
}

int main() {
    check_validate();
    check_layout();
    check_pack();
    std::printf("ideal_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("ideal_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
