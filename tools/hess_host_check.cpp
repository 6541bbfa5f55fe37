// Stand-alone host check of mrbf_eval_hessian's host logic (morbit.jl_amd/csrc/hess_host.hpp): the validation behind the call's return
// codes, the list of selected outputs, the shape of a launch, the split rule, the chunk rule and the layout of the work buffer.  Every
// case is judged by statements made directly from the header's text (include/mrbf.h "model Hessians" and the comments of
// hess_host.hpp), not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/hess_host_check.cpp -o /tmp/hess_host_check && /tmp/hess_host_check
// Enumerated: every defect of a call alone and in pairs (the order of the codes); row lists of 0 .. 4 entries over k in {1, 2, 3, 17};
// the split rule over m in {1 .. 70, 511, 512, 513, 4096}, n in {1 .. 70, 257, 300, 8192}, d in {1, 16, 64, 65, 128, 129, 300, 4096},
// r in {1, 2, 3, 4, 5, 17}; the chunk rule over m in 0 .. 40, point sizes 8 .. 4096 bytes and limits 1 .. 8192 bytes.
#include <cstdio>
#include <cstring>

#include "../morbit.jl_amd/csrc/hess_host.hpp"

using namespace mrbf::hess;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static const int32_t ROWS_OK[] = {2, 0, 2};

static Call good_call() {
    Call c;
    c.has_ctx = c.has_model = true;
    c.m = 5, c.k = 3;
    c.X = c.out = true;
    c.n_rows = 3, c.rows = ROWS_OK;
    return c;
}

// defects in the order the header lists the codes; the earlier one wins when two are present
enum Defect { NO_CTX, NO_MODEL, FOREIGN, NEG_M, NEG_ROWS, NULL_ROWS, ROW_HIGH, ROW_NEG, NO_X, NO_OUT, N_DEFECTS };
static const int CODE[N_DEFECTS] = {-1, -2, -4, -3, -5, -5, -6, -6, -4, -7};
static const int32_t ROWS_HIGH[] = {0, 3, 1}, ROWS_NEG[] = {1, -1, 0};

static void apply(Call &c, int defect) {
    switch (defect) {
        case NO_CTX: c.has_ctx = false; break;
        case NO_MODEL: c.has_model = false; break;
        case FOREIGN: c.foreign = true; break;
        case NEG_M: c.m = -1; break;
        case NEG_ROWS: c.n_rows = -1; break;
        case NULL_ROWS: c.rows = nullptr; break;  // n_rows = 3
        case ROW_HIGH: c.rows = ROWS_HIGH; break;  // 3 is outside [0, 3)
        case ROW_NEG: c.rows = ROWS_NEG; break;
        case NO_X: c.X = false; break;
        case NO_OUT: c.out = false; break;
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
            if ((a == NEG_ROWS || a == NULL_ROWS || a == ROW_HIGH || a == ROW_NEG) && (b == NEG_ROWS || b == NULL_ROWS || b == ROW_HIGH || b == ROW_NEG))
                continue;  // two defects of the same argument overwrite each other
            Call c2 = good_call();
            apply(c2, a), apply(c2, b);
            ++g_cases;
            CHECK(validate(c2) == CODE[a]);
        }
    }
    // "NULL with n_rows = 0 means all k outputs"; "m = 0 is treated as mrbf_eval treats it": legal with NULL X and NULL hess_out,
    // while a negative m and a bad row are still refused
    Call c = good_call();
    c.n_rows = 0, c.rows = nullptr;
    CHECK(validate(c) == 0);
    c.m = 0, c.X = false, c.out = false;
    CHECK(validate(c) == 0);
    c.n_rows = 3, c.rows = ROWS_HIGH;
    CHECK(validate(c) == -6);
    // rows 0 and k - 1 are inside
    const int32_t edge[] = {0, 2};
    c = good_call();
    c.n_rows = 2, c.rows = edge;
    CHECK(validate(c) == 0);
}

// "rows holds 0-based output indices.  Any order and repeats are allowed.  NULL with n_rows = 0 means all k outputs."
static void check_rows() {
    const int ks[] = {1, 2, 3, 17};
    for (int k : ks) {
        Call c = good_call();
        c.k = k, c.n_rows = 0, c.rows = nullptr;
        const std::vector<int32_t> all = row_list(c);
        ++g_cases;
        CHECK((int)all.size() == k);
        for (int l = 0; l < k; ++l) CHECK(all[(size_t)l] == l);
        for (int len = 1; len <= 4; ++len)
            for (int code = 0; code < 256; code += 3) {
                int32_t rows[4];
                for (int i = 0; i < len; ++i) rows[i] = (code >> (2 * i)) % k;
                c.n_rows = len, c.rows = rows;
                ++g_cases;
                CHECK(validate(c) == 0);
                const std::vector<int32_t> got = row_list(c);
                CHECK((int)got.size() == len && std::memcmp(got.data(), rows, sizeof(int32_t) * (size_t)len) == 0);
            }
    }
}

// "the split count is a function of (m, n, d, r) alone"; pieces are multiples of NC centres, cover the range, none is empty; a call
// with TARGET_WGS workgroups or more keeps the range in one piece; below, as many pieces as bring it there, at most ceil(n / NC) and
// at most MAX_SPLIT
static void check_split() {
    CHECK(SB == 64 && NC == 32 && MAX_RB == 4 && TARGET_WGS == 512 && MAX_SPLIT == 64);
    CHECK(rb(1) == 1 && rb(2) == 2 && rb(3) == 4 && rb(4) == 4 && rb(1024) == 4);
    CHECK(npass(1) == 1 && npass(2) == 1 && npass(3) == 1 && npass(4) == 1 && npass(5) == 2 && npass(17) == 5);
    CHECK(nblocks(1) == 1 && nblocks(64) == 1 && nblocks(65) == 2 && nblocks(300) == 5 && nblocks(4096) == 64);
    CHECK(npairs(64) == 1 && npairs(65) == 3 && npairs(140) == 6 && npairs(300) == 15 && npairs(4096) == 2080);
    std::vector<int64_t> ms, ns;
    for (int64_t v = 1; v <= 70; ++v) ms.push_back(v), ns.push_back(v);
    for (int64_t v : {511, 512, 513, 4096}) ms.push_back(v);
    for (int64_t v : {257, 300, 8192}) ns.push_back(v);
    const int ds[] = {1, 16, 64, 65, 128, 129, 300, 4096};
    const int rs[] = {1, 2, 3, 4, 5, 17};
    for (int64_t m : ms)
        for (int64_t n : ns)
            for (int d : ds)
                for (int r : rs) {
                    int64_t per = -1;
                    const int s = nsplit(m, n, d, r, &per);
                    ++g_cases;
                    CHECK(s == nsplit(m, n, d, r));  // a function of its arguments
                    CHECK(s >= 1 && per >= NC && per % NC == 0);
                    CHECK((int64_t)(s - 1) * per < n && (int64_t)s * per >= n);  // covers the range, the last piece not empty
                    const int64_t wgs = m * npairs(d) * npass(r);
                    if (wgs >= TARGET_WGS) CHECK(s == 1);
                    CHECK(s <= ceil_div(n, NC) && s <= MAX_SPLIT);
                    if (n <= NC) CHECK(s == 1);
                    if (s > 1) CHECK(wgs * (s - 1) < TARGET_WGS);   // one piece fewer would still be short of the target
                    CHECK(s == ceil_div(n, per));
                    CHECK(partial_doubles(m, d, r, s) == (s <= 1 ? 0 : (size_t)(m * npass(r) * npairs(d) * s) * (size_t)rb(r) * SB * SB));
                }
    // the shapes of the documentation
    CHECK(nsplit(1, 8192, 64, 2) == 64);    // m = 1 on C3's model: 64 pieces of 128 centres
    CHECK(nsplit(256, 8192, 64, 2) == 2);
    CHECK(nsplit(64, 257, 128, 2) == 3);
    CHECK(nsplit(16, 1024, 256, 2) == 4);
}

// "chunks of whole query points"; "one point larger than the limit is a chunk of its own"; "256 MiB by default"
static void check_chunks() {
    CHECK(STAGE_LIMIT_BYTES == (size_t)256 << 20);
    const size_t points[] = {8, 24, 800, 4096};
    for (int64_t m = 0; m <= 40; ++m)
        for (size_t pb : points)
            for (int64_t limit = 1; limit <= 8192; limit = limit * 2 + (limit % 3)) {
                const auto ch = chunks(m, pb, limit);
                ++g_cases;
                int64_t next = 0;
                for (size_t j = 0; j < ch.size(); ++j) {
                    CHECK(ch[j].first == next && ch[j].second >= 1);
                    CHECK((size_t)ch[j].second * pb <= (size_t)limit || ch[j].second == 1);
                    if (j + 1 < ch.size()) CHECK((size_t)(ch[j].second + 1) * pb > (size_t)limit);  // closed only where one more would not fit
                    next += ch[j].second;
                }
                CHECK(next == m);
                if (m == 0) CHECK(ch.empty());
            }
    // the default: C3's m = 256 (64 KiB per point) is one chunk; 300 x 300 x 2 blocks: 186 points per chunk
    CHECK(chunks(256, (size_t)2 * 64 * 64 * 8).size() == 1);
    CHECK(chunks(1000, (size_t)2 * 300 * 300 * 8).size() == 6 && chunks(1000, (size_t)2 * 300 * 300 * 8, 0)[0].second == 186);
    CHECK(chunks(3, (size_t)300 << 20).size() == 3);     // every point beyond the limit: one each
    CHECK(chunks(5, 0).size() == 1);
}

// "selected outputs (int32) | partial blocks"; "every piece a multiple of 16"
static void check_layout() {
    for (int64_t pts : {1, 2, 63})
        for (int d : {1, 64, 65, 300})
            for (int r : {1, 2, 3, 17})
                for (int s : {1, 2, 9}) {
                    const Layout L = layout(pts, d, r, s);
                    ++g_cases;
                    CHECK(L.rows == 0 && L.part % 16 == 0 && L.total % 16 == 0);
                    CHECK(L.part * sizeof(double) >= (size_t)r * sizeof(int32_t));       // the rows fit in front of the partial blocks
                    CHECK(L.total - L.part >= partial_doubles(pts, d, r, s));
                    if (s == 1) CHECK(L.total == L.part);
                }
}

int main() {
    check_validate();
    check_rows();
    check_split();
    check_chunks();
    check_layout();
    std::printf("hess_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("hess_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
