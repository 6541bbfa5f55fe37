// Stand-alone host check of the directed-search direction QP's host logic (morbit.jl_amd/csrc/ds_host.hpp): the validation behind
// mrbf_ds_direction's return codes, the iteration cap, the per-QP workspace and the rule that cuts a batch into launches, and the LDS
// carve.  Every case is judged by statements made directly from the header's text (include/mrbf.h "directed search" and the comments of
// ds_host.hpp), not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/ds_host_check.cpp -o /tmp/ds_host_check && /tmp/ds_host_check
// Enumerated: every defect of a call alone and in pairs (the order of the codes); the limits of d and k on either side; the chunk rule
// over n_qp in {1 .. 40, 65535, 2^20} and d in {1, 2, 7, 64, 300, 4096}; the carve for every k in 1 .. 16 (walked as the kernel walks
// it, in a buffer of its size under AddressSanitizer).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../morbit.jl_amd/csrc/descent_call_host.hpp"
#include "../morbit.jl_amd/csrc/ds_host.hpp"

using namespace mrbf::ds;
using mrbf::dcall::WS_LIMIT_BYTES;
// QPs per launch, as ds::launch asks for them
static int64_t chunk(int64_t n_qp, int d) { return mrbf::dcall::chunk(n_qp, ws_bytes(d)); }

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
    c.n_qp = 37, c.d = 65, c.k = 3;
    c.G = c.r = c.x = c.lb = c.ub = true;
    c.d_out = c.z_out = c.omega_out = c.status_out = true;
    return c;
}

// defects in the order the header lists the codes; the earlier one wins when two are present
enum Defect { NO_CTX, BAD_NQP, BAD_D, BAD_K, NO_G, NO_R, NO_X, NO_LB, NO_UB, NO_DOUT, NO_ZOUT, NO_OMEGA, NO_STATUS, N_DEFECTS };
static const int CODE[N_DEFECTS] = {-1, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12, -13, -14};

static void apply(Call &c, int defect) {
    switch (defect) {
        case NO_CTX: c.has_ctx = false; break;
        case BAD_NQP: c.n_qp = 0; break;
        case BAD_D: c.d = 0; break;
        case BAD_K: c.k = 17; break;
        case NO_G: c.G = false; break;
        case NO_R: c.r = false; break;
        case NO_X: c.x = false; break;
        case NO_LB: c.lb = false; break;
        case NO_UB: c.ub = false; break;
        case NO_DOUT: c.d_out = false; break;
        case NO_ZOUT: c.z_out = false; break;
        case NO_OMEGA: c.omega_out = false; break;
        case NO_STATUS: c.status_out = false; break;
    }
}

static void check_validate() {
    CHECK(validate(good_call()) == 0);
    for (int a = 0; a < N_DEFECTS; ++a) {
        Call c = good_call();
        apply(c, a);
        ++g_cases;
        CHECK(validate(c) == CODE[a]);
        CHECK(validate(c) != -2);  // "-2 is never returned"
        for (int b = a + 1; b < N_DEFECTS; ++b) {
            Call c2 = good_call();
            apply(c2, a), apply(c2, b);
            ++g_cases;
            CHECK(validate(c2) == CODE[a]);
        }
    }
    // "1 <= d <= 4096, 1 <= k <= 16, n_qp >= 1": the limits on either side
    CHECK(MAXD == 4096 && MAXK == 16 && THREADS == 256);
    Call c = good_call();
    c.d = 1, c.k = 1, c.n_qp = 1;
    CHECK(validate(c) == 0);
    c.d = 4096, c.k = 16, c.n_qp = (int64_t)1 << 40;
    CHECK(validate(c) == 0);
    c.d = 4097;
    CHECK(validate(c) == -4);
    c.d = -1;
    CHECK(validate(c) == -4);
    c.d = 7, c.k = 0;
    CHECK(validate(c) == -5);
    c.k = 3, c.n_qp = -5;
    CHECK(validate(c) == -3);
}

// "Cap 8 (d + k) + 16"
static void check_cap() {
    for (int d : {1, 2, 7, 300, 4096})
        for (int k : {1, 2, 16}) {
            ++g_cases;
            CHECK(iteration_cap(d, k) == 8 * (d + k) + 16);
        }
}

// "4 d doubles (d, p, l, u) and d ints"; "QPs per launch: all of them, unless their workspaces would pass WS_LIMIT_BYTES; at least one"
static void check_workspace() {
    CHECK(WS_LIMIT_BYTES == (size_t)256 << 20);
    std::vector<int64_t> ns;
    for (int64_t v = 1; v <= 40; ++v) ns.push_back(v);
    ns.push_back(65535), ns.push_back((int64_t)1 << 20);
    for (int d : {1, 2, 7, 64, 300, 4096}) {
        CHECK(ws_doubles(d) == (size_t)4 * d && ws_ints(d) == (size_t)d && ws_bytes(d) == (size_t)36 * d);
        for (int64_t n : ns) {
            const int64_t per = chunk(n, d);
            ++g_cases;
            CHECK(per >= 1 && per <= n);
            CHECK((size_t)per * ws_bytes(d) <= WS_LIMIT_BYTES || per == 1);
            if (per < n) CHECK((size_t)(per + 1) * ws_bytes(d) > WS_LIMIT_BYTES);  // cut only where one more would not fit
            if ((size_t)n * ws_bytes(d) <= WS_LIMIT_BYTES) CHECK(per == n);
        }
    }
    CHECK(chunk(37, 4096) == 37);                         // the largest test shape is one launch
    CHECK(chunk((int64_t)1 << 20, 4096) == 1820);         // 256 MiB / (36 x 4096 bytes)
}

// "offsets in bytes, each a multiple of 16"; the pieces do not overlap and the whole stays far below the 64 KiB a workgroup gets by default
static void check_carve() {
    CHECK(NVEC >= 17 && NIVEC == 3 && NISC >= 6 && NDSC >= 2);
    for (int k = 1; k <= MAXK; ++k) {
        const Carve c = carve(k);
        ++g_cases;
        const size_t off[] = {c.M, c.L, c.A, c.vec, c.part, c.ipart, c.ivec, c.isc, c.dsc, c.total};
        const size_t need[] = {(size_t)k * k * 8, (size_t)k * k * 8, (size_t)k * k * 8, (size_t)NVEC * MAXK * 8, (size_t)THREADS * 8,
                               (size_t)THREADS * 4, (size_t)NIVEC * MAXK * 4, (size_t)NISC * 4, (size_t)NDSC * 8};
        for (int i = 0; i < 9; ++i) {
            CHECK(off[i] % 16 == 0);
            CHECK(off[i] + need[i] <= off[i + 1]);
        }
        CHECK(c.M == 0 && c.total % 16 == 0 && c.total <= (size_t)16 * 1024);
        // walk it as the kernel does: every piece written to its end inside a buffer of exactly c.total bytes
        std::vector<char> buf(c.total);
        for (int i = 0; i < 9; ++i) std::memset(buf.data() + off[i], i + 1, need[i]);
        for (int i = 0; i < 9; ++i) CHECK(buf[off[i]] == i + 1 && buf[off[i] + need[i] - 1] == i + 1);
    }
}

int main() {
    check_validate();
    check_cap();
    check_workspace();
    check_carve();
    std::printf("ds_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("ds_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
