// Stand-alone host check of the resident site database's host logic (morbit.jl_amd/csrc/db_host.hpp): the capacity rule, the
// exclusion-mask builder, the validation of a batch's jobs and the layout of a batch's views, upload, read-back and scratch.  Every
// case is judged by statements made directly from the header's text (include/mrbf.h "resident site database" and the comments of
// db_host.hpp), not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/db_host_check.cpp -o /tmp/db_host_check && /tmp/db_host_check
// Enumerated: capacities 0 .. 300 against needs 0 .. 700; every exclude list of up to 4 entries from {-1, 0 .. 5, 6, 7} on databases of
// 0 .. 6 rows; batches of 1 .. 3 jobs with each defect in each position; layouts of 1 .. 4 starts with 0 .. 200 rows each (a stride
// through the combinations), d in {1, 3, 65, 128}.
#include <cstdio>
#include <cstring>
#include <set>

#include "../morbit.jl_amd/csrc/db_host.hpp"

using namespace mrbf::db;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

// "twice the capacity, at least what is needed, at least 64 rows"; unchanged while the rows fit
static void check_capacity() {
    for (int64_t cap = 0; cap <= 300; ++cap)
        for (int64_t need = 0; need <= 700; ++need) {
            const int64_t c = grow_capacity(cap, need);
            ++g_cases;
            CHECK(c >= need && c >= cap);
            if (need <= cap) CHECK(c == cap);
            else CHECK(c >= 2 * cap && c >= 64 && (c == 2 * cap || c == need || c == 64));
        }
    // m appends of one row: the rows copied by all reallocations stay below 2 m + 64
    int64_t cap = 0, copied = 0;
    for (int64_t n = 0; n < 100000; ++n) {
        const int64_t c = grow_capacity(cap, n + 1);
        if (c != cap) copied += n, cap = c;
    }
    CHECK(copied < 2 * 100000 + 64);
}

// "mask[i] = 1 iff i is in exclude, i in [0, n_sites); duplicates allowed, entries outside the range ignored"
static void check_mask() {
    const int64_t alphabet[] = {-1, 0, 1, 2, 3, 4, 5, 6, 7};
    const int A = 9;
    for (int64_t n = 0; n <= 6; ++n)
        for (int len = 0; len <= 4; ++len) {
            int total = 1;
            for (int i = 0; i < len; ++i) total *= A;
            for (int code = 0; code < total; ++code) {
                int64_t ex[4];
                for (int i = 0, c = code; i < len; ++i, c /= A) ex[i] = alphabet[c % A];
                std::vector<unsigned char> guard((size_t)n + 2, 0xAB);  // a byte before and behind the mask
                build_mask(n, len, ex, guard.data() + 1);
                ++g_cases;
                CHECK(guard[0] == 0xAB && guard[(size_t)n + 1] == 0xAB);
                for (int64_t i = 0; i < n; ++i) {
                    bool in = false;
                    for (int e = 0; e < len; ++e) in = in || ex[e] == i;
                    CHECK(guard[(size_t)i + 1] == (in ? 1 : 0));
                }
            }
        }
}

// the validation: "an invalid field of a job is an invalid jobs"; "a database may appear at most once per batch call"; an index out of
// range is the gather job's own rc (-3), not the call's
static void check_jobs() {
    const int d = 3;
    double lb[3] = {0, 0, 0}, ub[3] = {1, 1, 1}, x0[3] = {0, 0, 0}, row[3];
    int64_t ex[2] = {0, 9}, idx[3] = {2, 0, 2};
    int handles[3];
    for (int ns = 1; ns <= 3; ++ns) {
        // defect 0: none; 1: db NULL; 2: another context; 3: another d; 4: repeated db (ns > 1); box: 5 lb NULL, 6 x0 NULL, 7 negative
        // exclude count, 8 count without a list, 9 first_row NULL; gather: 5 negative n_idx, 6 indices NULL
        for (int defect_kind = 0; defect_kind <= 9; ++defect_kind)
            for (int at = 0; at < ns; ++at) {
                mrbf_db_box_job bj[3];
                mrbf_db_gather_job gj[3];
                DbInfo info[3];
                std::memset(bj, 0, sizeof(bj)), std::memset(gj, 0, sizeof(gj));
                for (int p = 0; p < ns; ++p) {
                    info[p] = DbInfo{&handles[p], d, 2, 5, true};
                    bj[p].lb = lb, bj[p].ub = ub, bj[p].x0 = x0, bj[p].n_exclude = 2, bj[p].exclude = ex, bj[p].first_row = row;
                    gj[p].n_idx = 3, gj[p].indices = idx;
                }
                bool box_bad = defect_kind != 0, gather_bad = defect_kind != 0 && defect_kind <= 6;
                switch (defect_kind) {
                    case 1: info[at].id = nullptr; break;
                    case 2: info[at].own = false; break;
                    case 3: info[at].d = d + 1; break;
                    case 4:
                        if (ns > 1) info[at].id = info[(at + 1) % ns].id;
                        else box_bad = gather_bad = false;
                        break;
                    case 5: bj[at].lb = nullptr, gj[at].n_idx = -1; break;
                    case 6: bj[at].x0 = nullptr, gj[at].indices = nullptr; break;
                    case 7: bj[at].n_exclude = -1; break;
                    case 8: bj[at].exclude = nullptr; break;
                    case 9: bj[at].first_row = nullptr; break;
                }
                const Defect B = check_box_jobs(ns, d, bj, info, 5), G = check_gather_jobs(ns, d, gj, info, 4);
                ++g_cases;
                CHECK(B.code == (box_bad ? -5 : 0));
                CHECK(G.code == (gather_bad ? -4 : 0));
                CHECK(B.msg.empty() == !box_bad && G.msg.empty() == !gather_bad);
            }
    }
    // an empty exclude list needs no pointer; no indices need none either
    {
        mrbf_db_box_job bj;
        mrbf_db_gather_job gj;
        std::memset(&bj, 0, sizeof(bj)), std::memset(&gj, 0, sizeof(gj));
        DbInfo info{&handles[0], d, 2, 0, true};
        bj.lb = lb, bj.ub = ub, bj.x0 = x0, bj.first_row = row;
        CHECK(check_box_jobs(1, d, &bj, &info, 5).code == 0);
        CHECK(check_gather_jobs(1, d, &gj, &info, 4).code == 0);
    }
    // the gather job's own rc: every list of up to 3 entries from {-1, 0, 1, 2, 3} on 0 .. 3 rows
    for (int64_t n = 0; n <= 3; ++n)
        for (int len = 0; len <= 3; ++len)
            for (int code = 0; code < 125; ++code) {
                int64_t l[3];
                bool bad = false;
                for (int i = 0, c = code; i < 3; ++i, c /= 5) l[i] = c % 5 - 1;
                for (int i = 0; i < len; ++i) bad = bad || l[i] < 0 || l[i] >= n;
                ++g_cases;
                CHECK(index_rc(n, len, l, GATHER_RC_INDEX) == (bad ? -3 : 0));
            }
}

// the layouts.  Box: every start's rows are its own (no two starts share a row of a per-row array or a workgroup), the views hold every
// row of every database twice (candidate sites, shifted rows) without overlap, upload, read-back and scratch are disjoint pieces of the
// work buffer in that order, and the head of the read-back (counts, picks, first rows) is a prefix of it.
static void check_layouts() {
    const int ds[] = {1, 3, 65, 128};
    const int64_t sizes[] = {0, 1, 63, 64, 65, 199, 200};
    const size_t desc = 120;
    for (int d : ds)
        for (int ns = 1; ns <= 4; ++ns) {
            int total = 1;
            for (int i = 0; i < ns; ++i) total *= 7;
            for (int code = 0; code < total; code += (ns == 4 ? 5 : 1)) {
                int64_t n[4];
                for (int i = 0, c = code; i < ns; ++i, c /= 7) n[i] = sizes[c % 7];
                const BoxLayout L = box_layout(ns, d, n, desc);
                ++g_cases;
                int64_t nblk_max = 0;
                for (int p = 0; p < ns; ++p) {
                    CHECK(L.roff[p] % ROWS == 0);
                    CHECK(L.roff[p + 1] - L.roff[p] >= n[p] && L.roff[p + 1] - L.roff[p] < n[p] + ROWS);
                    nblk_max = std::max(nblk_max, (n[p] + ROWS - 1) / ROWS);
                    // the views: n_p x d doubles each, inside the buffer, the next start's behind them, sites before shifted rows
                    CHECK(L.sites_view(p, d) + (size_t)n[p] * d <= (p + 1 < ns ? L.sites_view(p + 1, d) : L.shifted_view(0, d)));
                    CHECK(L.shifted_view(p, d) + (size_t)n[p] * d <= (p + 1 < ns ? L.shifted_view(p + 1, d) : L.view_doubles));
                }
                CHECK(L.rows == L.roff[ns] && L.nblk_max == nblk_max);
                const size_t R = (size_t)L.rows, NB = R / ROWS;
                // the pieces in order, each with room for what it holds
                const size_t at[] = {L.oDesc, L.oBounds, L.oMask, L.oHead, L.oFirst, L.oIdx, L.oNorm, L.oCnorm, L.oCount, L.oOffs, L.A.total};
                const size_t need[] = {ns * desc, (size_t)ns * 3 * d * 8, R, (size_t)ns * 16, (size_t)ns * d * 8, R * 8, R * 8, R * 8, NB * 4, NB * 4};
                CHECK(at[0] == 0);
                for (int i = 0; i < 10; ++i) CHECK(at[i] % 256 == 0 && at[i] + need[i] <= at[i + 1]);
                CHECK(L.A.upload_bytes() == L.oHead);
                CHECK(L.oHead + L.back_head_bytes == L.oIdx && L.oHead + L.A.back_bytes() == L.oNorm);
            }
        }
    // gather: a job that failed its own check (count -1) takes no room; the others' index lists follow each other, their views do not
    // overlap, every piece a multiple of 16 doubles
    for (int d : ds)
        for (int code = 0; code < 5 * 5 * 5; ++code) {
            const int64_t opts[] = {-1, 0, 1, 17, 300};
            int64_t m[3];
            const int k[3] = {1, 2, 5};
            for (int i = 0, c = code; i < 3; ++i, c /= 5) m[i] = opts[c % 5];
            const GatherLayout L = gather_layout(3, d, k, m, 56);
            ++g_cases;
            size_t end = 0;
            int64_t n_max = 0;
            for (int p = 0; p < 3; ++p) {
                const int64_t mm = std::max<int64_t>(m[p], 0);
                n_max = std::max(n_max, mm);
                CHECK(L.ioff[p + 1] - L.ioff[p] == mm);
                CHECK(L.soff[p] % 16 == 0 && L.voff[p] % 16 == 0);
                CHECK(L.soff[p] >= end && L.voff[p] >= L.soff[p] + (size_t)mm * d);
                end = L.voff[p] + (size_t)mm * k[p];
            }
            CHECK(L.view_doubles >= end && L.n_idx_max == n_max);
            CHECK(L.oIdx >= 3 * 56 && L.oIdx % 256 == 0 && L.A.upload_bytes() >= L.oIdx + (size_t)L.ioff[3] * 8);
        }
}

int main() {
    check_capacity();
    check_mask();
    check_jobs();
    check_layouts();
    if (g_failed) {
        std::printf("db_host_check: %d of %ld cases FAILED\n", g_failed, g_cases);
        return 1;
    }
    std::printf("db_host_check: ok (%ld cases)\n", g_cases);
    return 0;
}
