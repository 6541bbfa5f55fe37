// Stand-alone host check of the host logic of the directed-search direction QP with constraint rows
// (morbit.jl_amd/csrc/ds_rows_host.hpp): the validation behind mrbf_ds_direction_rows' return codes, the row-kind table, the start
// tolerance's range, the input arena's size, the workspace (ds_host.hpp's) and the LDS carve.  Every case is judged by statements made
// directly from the header's text (include/mrbf.h "directed search with constraint rows" and the comments of ds_rows_host.hpp), not by
// a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/ds_rows_host_check.cpp -o /tmp/ds_rows_host_check && /tmp/ds_rows_host_check
// Enumerated: every defect of a call alone and in pairs (the order of the codes); the limits of d, k and K on either side; NULL rows
// where their count is 0; the kind of every row for every (k, m_eq, m_in) with K <= 16; the carve for every K in 1 .. 16 (walked as the
// kernel walks it, in a buffer of its size under AddressSanitizer).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../morbit.jl_amd/csrc/descent_call_host.hpp"
#include "../morbit.jl_amd/csrc/ds_rows_host.hpp"

using namespace mrbf::ds;
using namespace mrbf::ds::rows;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static rows::Call good_call() {
    rows::Call c;
    c.has_ctx = true;
    c.n_qp = 37, c.d = 65, c.k = 2, c.m_eq = 2, c.m_in = 3;
    c.G = c.r = c.x = c.lb = c.ub = true;
    c.A_eq = c.b_eq = c.A_in = c.b_in = true;
    c.d_out = c.c_out = c.omega_out = c.status_out = true;
    return c;
}

// defects in the order the header lists the codes; the earlier one wins when two are present
enum Defect { NO_CTX, BAD_NQP, BAD_D, BAD_K, BAD_MEQ, BAD_MIN, BAD_ROWS, NO_G, NO_R, NO_X, NO_LB, NO_UB, NO_AEQ, NO_BEQ, NO_AIN, NO_BIN,
              NO_DOUT, NO_COUT, NO_OMEGA, NO_STATUS, N_DEFECTS };
static const int CODE[N_DEFECTS] = {-1, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12, -13, -14, -15, -16, -17, -18, -19, -20, -21};

static void apply(rows::Call &c, int defect) {
    switch (defect) {
        case NO_CTX: c.has_ctx = false; break;
        case BAD_NQP: c.n_qp = 0; break;
        case BAD_D: c.d = 0; break;
        case BAD_K: c.k = 0; break;
        case BAD_MEQ: c.m_eq = -1; break;
        case BAD_MIN: c.m_in = -1; break;
        case BAD_ROWS: c.m_in += 12; break;  // 2 + 2 + 15 rows
        case NO_G: c.G = false; break;
        case NO_R: c.r = false; break;
        case NO_X: c.x = false; break;
        case NO_LB: c.lb = false; break;
        case NO_UB: c.ub = false; break;
        case NO_AEQ: c.A_eq = false; break;
        case NO_BEQ: c.b_eq = false; break;
        case NO_AIN: c.A_in = false; break;
        case NO_BIN: c.b_in = false; break;
        case NO_DOUT: c.d_out = false; break;
        case NO_COUT: c.c_out = false; break;
        case NO_OMEGA: c.omega_out = false; break;
        case NO_STATUS: c.status_out = false; break;
    }
}

static void check_validate() {
    CHECK(rows::validate(good_call()) == 0);
    for (int a = 0; a < N_DEFECTS; ++a) {
        rows::Call c = good_call();
        apply(c, a);
        ++g_cases;
        CHECK(rows::validate(c) == CODE[a]);
        CHECK(rows::validate(c) != -2);  // "-2 is never returned"
        for (int b = a + 1; b < N_DEFECTS; ++b) {
            if (a == BAD_MIN && b == BAD_ROWS) continue;  // b acts on a's field
            rows::Call c2 = good_call();
            apply(c2, a), apply(c2, b);
            ++g_cases;
            CHECK(rows::validate(c2) == CODE[a]);
        }
    }
    // "1 <= d <= 4096, k >= 1, m_eq >= 0, m_in >= 0, K = k + m_eq + m_in <= 16, n_qp >= 1": the limits on either side
    rows::Call c = good_call();
    c.d = 1, c.k = 1, c.m_eq = 0, c.m_in = 15, c.n_qp = 1;
    CHECK(rows::validate(c) == 0);
    c.m_in = 16;
    CHECK(rows::validate(c) == -8);
    c.d = 4096, c.k = 16, c.m_in = 0, c.n_qp = (int64_t)1 << 40;
    CHECK(rows::validate(c) == 0);
    c.k = 17;
    CHECK(rows::validate(c) == -5);
    c.k = 8, c.m_eq = 8;
    CHECK(rows::validate(c) == 0);
    c.m_eq = 2147483647;  // no overflow in the row count
    CHECK(rows::validate(c) == -8);
    c.m_eq = 0, c.d = 4097;
    CHECK(rows::validate(c) == -4);
    // "NULL where the count is 0"
    c = good_call();
    c.m_eq = 0, c.A_eq = c.b_eq = false;
    CHECK(rows::validate(c) == 0);
    c.m_in = 0, c.A_in = c.b_in = false;
    CHECK(rows::validate(c) == 0);  // no rows at all: mrbf_ds_direction's QP
    c.m_in = 1;
    CHECK(rows::validate(c) == -16);
    c.A_in = true;
    CHECK(rows::validate(c) == -17);
}

// "W = [G; A_eq; A_in], objective rows first"; equality rows are never dropped and block on either side
static void check_kinds() {
    for (int k = 1; k <= MAXK; ++k)
        for (int me = 0; k + me <= MAXK; ++me)
            for (int mi = 0; k + me + mi <= MAXK; ++mi) {
                ++g_cases;
                int n_obj = 0, n_eq = 0, n_in = 0, last = 0;
                for (int i = 0; i < k + me + mi; ++i) {
                    const int kind = kind_of(i, k, me);
                    CHECK(kind >= last);  // the kinds come in blocks, in this order
                    last = kind;
                    n_obj += kind == OBJECTIVE, n_eq += kind == EQUALITY, n_in += kind == INEQUALITY;
                    CHECK(droppable(kind) == (kind != EQUALITY) && two_sided(kind) == (kind == EQUALITY));
                }
                CHECK(n_obj == k && n_eq == me && n_in == mi);
            }
}

// "no smaller than what the normal-step LP leaves behind (1e-13 on its own row scale) and no larger than 1e-9"
static void check_constants() {
    CHECK(START_TOL >= 1e-13 && START_TOL <= 1e-9);
    CHECK(START_TOL > FEAS_TOL);  // a right-hand side the method itself accepts is always a start
    CHECK(iteration_cap(300, 16) == 8 * 316 + 16);
    CHECK(input_doubles(7, 2, 1, 3) == (size_t)(2 * 7 + 2 + 3 * 7 + 4 * 8));
    CHECK(input_doubles(5, 3, 0, 0) == (size_t)(3 * 5 + 3 + 3 * 5));  // mrbf_ds_direction's arena
    // the d-length state does not grow with the rows: one launch for the largest test shape
    CHECK(mrbf::dcall::chunk(37, ws_bytes(4096)) == 37);
}

// "offsets in bytes, each a multiple of 16"; the pieces do not overlap and the whole stays far below the 64 KiB a workgroup gets by default
static void check_carve() {
    CHECK(rows::NVEC >= 22 && rows::NIVEC == 5 && NISC >= 7 && NDSC >= 2);
    for (int K = 1; K <= MAXK; ++K) {
        const rows::Carve c = rows::carve(K);
        ++g_cases;
        const size_t off[] = {c.M, c.MU, c.L, c.A, c.vec, c.part, c.ipart, c.ivec, c.isc, c.dsc, c.total};
        const size_t kk = (size_t)K * K * 8;
        const size_t need[] = {kk, kk, kk, kk, (size_t)rows::NVEC * MAXK * 8, (size_t)THREADS * 8, (size_t)THREADS * 4,
                               (size_t)rows::NIVEC * MAXK * 4, (size_t)NISC * 4, (size_t)NDSC * 8};
        for (int i = 0; i < 10; ++i) {
            CHECK(off[i] % 16 == 0);
            CHECK(off[i] + need[i] <= off[i + 1]);
        }
        CHECK(c.M == 0 && c.total % 16 == 0 && c.total <= (size_t)16 * 1024);
        // row_pass forms M with one partial sum per entry and thread: K * K <= THREADS
        CHECK(K * K <= THREADS);
        std::vector<char> buf(c.total);
        for (int i = 0; i < 10; ++i) std::memset(buf.data() + off[i], i + 1, need[i]);
        for (int i = 0; i < 10; ++i) CHECK(buf[off[i]] == i + 1 && buf[off[i] + need[i] - 1] == i + 1);
    }
}

int main() {
    check_validate();
    check_kinds();
    check_constants();
    check_carve();
    std::printf("ds_rows_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("ds_rows_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
