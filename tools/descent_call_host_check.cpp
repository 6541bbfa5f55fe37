// Stand-alone host check of what the direction calls share (morbit.jl_amd/csrc/descent_call_host.hpp): the rule that cuts a batch into
// launches, the staging layout of the outputs of mrbf_sd_direction, mrbf_normal_direction and mrbf_ds_direction, and the offsets of the
// packed input block of mrbf_sd_criticality, mrbf_normal_step, mrbf_ds_criticality and mrbf_sd_step.  The expected values are the
// formulas these seven calls spelled by hand before the header existed, copied here.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/descent_call_host_check.cpp -o /tmp/dcall_check && /tmp/dcall_check
// Enumerated: n in {0, 1, 2, 5} problems against workspaces of which n - 1, n and n + 1 fit, and one beyond the limit; N in {1, 2, 3, 7}
// and d in {1, 5} with every combination of given / NULL optional outputs and of host / device memory per output; d in {1, 5} with 0 and
// 2 linear rows.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../morbit.jl_amd/csrc/descent_call_host.hpp"

using namespace mrbf::dcall;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

// ---- the three launchers' rules as they stood: sd::launch over nc columns, ns::launch over n variables, ds::chunk over d variables
static int64_t sd_rule(int64_t n_lp, size_t nc) {
    const size_t per = (size_t)nc * (5 * sizeof(double) + sizeof(int));
    return std::max<int64_t>(1, std::min<int64_t>(n_lp, ((size_t)256 << 20) / per));
}
static int64_t ns_rule(int64_t n_lp, size_t n) {
    const size_t per = (size_t)n * (6 * sizeof(double) + sizeof(int));
    return std::max<int64_t>(1, std::min<int64_t>(n_lp, ((size_t)256 << 20) / per));
}
static int64_t ds_rule(int64_t n_qp, size_t d) {
    int64_t fit = (int64_t)(((size_t)256 << 20) / (4 * d * sizeof(double) + d * sizeof(int32_t)));
    if (fit < 1) fit = 1;
    return n_qp < fit ? (n_qp < 1 ? 1 : n_qp) : fit;
}

static void check_chunk() {
    CHECK(WS_LIMIT_BYTES == (size_t)256 << 20);
    const size_t unit[3] = {5 * 8 + 4, 6 * 8 + 4, 4 * 8 + 4};  // bytes per column / variable of the three workspaces
    int64_t (*const rule[3])(int64_t, size_t) = {sd_rule, ns_rule, ds_rule};
    for (int64_t n : {0, 1, 2, 5})
        for (int64_t fit : {n - 1, n, n + 1, (int64_t)0}) {
            if (fit < 0) continue;
            for (int s = 0; s < 3; ++s) {
                // so many columns that exactly `fit` workspaces stay below the limit (fit = 0: one workspace is beyond it)
                const size_t count = fit ? WS_LIMIT_BYTES / (unit[s] * (size_t)fit) : WS_LIMIT_BYTES / unit[s] + 1;
                const size_t per = count * unit[s];
                ++g_cases;
                CHECK((int64_t)(WS_LIMIT_BYTES / per) == fit);
                const int64_t got = chunk(n, per);
                CHECK(got == rule[s](n, count));
                CHECK(got == std::max<int64_t>(1, std::min(n, fit)));
                if (n == 0 || fit == 0) CHECK(got == 1);  // a zero count and a count beyond the limit
            }
        }
    CHECK(chunk(37, 36 * 4096) == 37 && chunk((int64_t)1 << 20, 36 * 4096) == 1820);  // ds_host_check's two shapes
    CHECK(chunk(5, 100, 250) == 2 && chunk(5, 100, 99) == 1);                          // the limit is an argument
}

// ---- outputs.  want[i]: the byte offset the entry point computed by hand for output i (whatever its residency)
static char g_mem[8];  // stands for the caller's buffers: only the addresses are used
static void check_one(std::vector<Out> o, const std::vector<size_t> &want, size_t out_dbl, size_t out_int) {
    ++g_cases;
    const size_t doubles = out_layout(o.data(), o.size());
    CHECK(doubles == out_dbl + (out_int + 1) / 2 + 1);  // the size the three entries asked of their arena slot
    std::vector<char> buf(doubles * sizeof(double), 0);
    for (size_t i = 0; i < o.size(); ++i) {
        const size_t bytes = o[i].count * (o[i].is_int ? 4 : 8);
        if (!o[i].user || o[i].device) {
            CHECK(o[i].at == NONE);  // in place, or not given: no offset
            continue;
        }
        CHECK(o[i].at == want[i]);
        CHECK(o[i].at % (o[i].is_int ? 4 : 8) == 0);
        CHECK(o[i].is_int ? o[i].at >= out_dbl * 8 : o[i].at + bytes <= out_dbl * 8);  // the int region begins at out_dbl
        CHECK(o[i].at + bytes <= buf.size());
        for (size_t b = 0; b < bytes && o[i].at + bytes <= buf.size(); ++b) CHECK(buf[o[i].at + b]++ == 0);  // disjoint
    }
}
// every combination of given / NULL for the outputs in `optional` (a bit mask) and of host / device for each output
static void check_combinations(const std::vector<Out> &all, unsigned optional, const std::vector<size_t> &want, size_t out_dbl, size_t out_int) {
    const unsigned n = (unsigned)all.size();
    for (unsigned given = 0; given < (1u << n); ++given) {
        if ((given | optional) != (1u << n) - 1) continue;  // a required output is always given
        for (unsigned dev = 0; dev < (1u << n); ++dev) {
            std::vector<Out> o = all;
            for (unsigned i = 0; i < n; ++i) {
                o[i].user = (given >> i & 1) ? g_mem : nullptr;
                o[i].device = o[i].user && (dev >> i & 1);
            }
            check_one(o, want, out_dbl, out_int);
        }
    }
}

static void check_outputs() {
    for (size_t N : {1, 2, 3, 7})
        for (size_t d : {1, 5}) {
            const size_t k = 2, m_sd = k + 2, m_ns = 2;
            // mrbf_sd_direction / mrbf_normal_direction: d (n), omega (alpha), dual (optional), status, iterations (optional)
            for (size_t m : {m_sd, m_ns}) {
                const size_t out_dbl = N * d + N + N * m, out_int = 3 * N;
                const std::vector<Out> lp = {{g_mem, N * d, false}, {g_mem, N, false}, {g_mem, N * m, false}, {g_mem, N, true}, {g_mem, 2 * N, true}};
                check_combinations(lp, 1u << 2 | 1u << 4, {0, 8 * (N * d), 8 * (N * d + N), 8 * out_dbl, 8 * out_dbl + 4 * N}, out_dbl, out_int);
            }
            // mrbf_ds_direction: d, z, omega, mult (optional), status, iterations (optional)
            const size_t out_dbl = N * d + 2 * N * k + N, out_int = 3 * N;
            const std::vector<Out> qp = {{g_mem, N * d, false}, {g_mem, N * k, false}, {g_mem, N, false}, {g_mem, N * k, false}, {g_mem, N, true}, {g_mem, 2 * N, true}};
            check_combinations(qp, 1u << 3 | 1u << 5, {0, 8 * (N * d), 8 * (N * d + N * k), 8 * (N * d + N * k + N), 8 * out_dbl, 8 * out_dbl + 4 * N},
                               out_dbl, out_int);
        }
}

// ---- the packed blocks: the pieces in the order each call adds them, against the offsets it spelled as `base + ...`
static void check_pack() {
    for (size_t d : {1, 5})
        for (size_t nlin : {0, 2}) {
            ++g_cases;
            {  // mrbf_sd_criticality: x_n, x, lb, ub, A, b
                Pack p;
                CHECK(p.add(d) == 0 && p.add(d) == d && p.add(d) == 2 * d && p.add(d) == 3 * d);
                CHECK(p.add(nlin * d) == 4 * d && p.add(nlin) == 4 * d + nlin * d && p.total == 4 * d + nlin * (d + 1));
            }
            {  // mrbf_normal_step: x, lb, ub, A, b
                Pack p;
                CHECK(p.add(d) == 0 && p.add(d) == d && p.add(d) == 2 * d);
                CHECK(p.add(nlin * d) == 3 * d && p.add(nlin) == 3 * d + nlin * d && p.total == 3 * d + nlin * (d + 1));
            }
            {  // mrbf_ds_criticality: x_n, lb, ub, r (k entries; the call takes no linear rows)
                const size_t k = 2 + nlin;
                Pack p;
                CHECK(p.add(d) == 0 && p.add(d) == d && p.add(d) == 2 * d && p.add(k) == 3 * d && p.total == 3 * d + k);
            }
            {  // mrbf_sd_step: x_n, x, lb, ub, d, A, b, [delta, omega]
                Pack p;
                CHECK(p.add(d) == 0 && p.add(d) == d && p.add(d) == 2 * d && p.add(d) == 3 * d && p.add(d) == 4 * d);
                CHECK(p.add(nlin * d) == 5 * d && p.add(nlin) == 5 * d + nlin * d && p.add(2) == 5 * d + nlin * d + nlin);
                CHECK(p.total == 5 * d + nlin * (d + 1) + 2);
            }
        }
}

int main() {
    check_chunk();
    check_outputs();
    check_pack();
    std::printf("descent_call_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("descent_call_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
