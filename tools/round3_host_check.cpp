// Stand-alone host check of the batched round 3's host logic (morbit.jl_amd/csrc/round3_host.hpp): a start's row counts, the validation
// of a batch's jobs, the reservation rule and the layout.  Every case is judged by statements made from the header's text
// (include/mrbf.h "Round 3 of the training-site selection"), not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/round3_host_check.cpp -o /tmp/round3_host_check && /tmp/round3_host_check
// Enumerated: n_missing, max_new in -1 .. 5, n_dirs 0 .. 4 (or the axes), the four (ensure_fully_linear, force_rebuild) settings and both
// modes for d in {1, 2, 3}; batches of 1 .. 3 jobs with each defect in each position; layouts of 1 .. 4 such starts on databases of
// 0 .. 70 rows with capacities 0, 4 and 64, d in {1, 2, 3, 65, 128}, host-side and device-side directions.
#include <cstdio>
#include <set>

#include "../morbit.jl_amd/csrc/round3_host.hpp"

using namespace mrbf::round3;
using mrbf::db::grow_capacity;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static double g_vec[4] = {0, 0, 0, 0};
static double g_dirs[128 * 8];
static int g_dbs[8];  // stand-ins for database handles

static mrbf_round3_job make_job(int n_missing, int max_new, int n_dirs, bool axes, int efl, int force, int mode) {
    mrbf_round3_job jb;
    std::memset(&jb, 0, sizeof(jb));
    jb.x = jb.lb = jb.ub = g_vec;
    jb.dirs = axes ? nullptr : g_dirs;
    jb.n_dirs = n_dirs, jb.n_missing = n_missing, jb.max_new = max_new;
    jb.ensure_fully_linear = efl, jb.force_rebuild = force, jb.mode = mode;
    return jb;
}

// "n_new = max(0, min(n_missing, max_new))"; the rebuild writes max(0, min(d, max_new)) rows and only a start with
// ensure_fully_linear && !force_rebuild can rebuild; "n_dirs < n_new (with dirs == NULL n_dirs is d) sets the job's own rc to -3";
// the improvement step uses direction 0 alone
static void check_counts() {
    for (int d = 1; d <= 3; ++d)
        for (int nm = -1; nm <= 5; ++nm)
            for (int mx = -1; mx <= 5; ++mx)
                for (int nd = 0; nd <= 5; ++nd)  // 5: the axes
                    for (int flags = 0; flags < 4; ++flags)
                        for (int mode = 0; mode < 2; ++mode) {
                            const bool axes = nd == 5;
                            const mrbf_round3_job jb = make_job(nm, mx, axes ? 0 : nd, axes, flags & 1, flags >> 1, mode);
                            const Counts c = counts_of(jb, d);
                            ++g_cases;
                            const int dirs = axes ? d : nd;
                            CHECK(c.n_dirs == dirs);
                            if (mode == MRBF_R3_IMPROVE) {
                                CHECK(c.rc == 0 && c.n1 == (dirs >= 1 ? 1 : 0) && c.n2 == 0 && !c.can_rebuild && c.rows() == c.n1);
                                continue;
                            }
                            const int n_new = std::max(0, std::min(nm, mx));
                            if (dirs < n_new) {
                                CHECK(c.rc == -3 && c.rows() == 0);
                                continue;
                            }
                            const bool can = (flags & 1) && !(flags >> 1);
                            CHECK(c.rc == 0 && c.n1 == n_new && c.can_rebuild == can);
                            CHECK(c.n2 == (can ? std::max(0, std::min(d, mx)) : 0));
                            CHECK(c.rows() == std::max(c.n1, c.n2) && c.n1 <= dirs && c.n2 <= d);
                        }
}

// "an invalid field, a database of another d or context or one named twice is an invalid `jobs` (-4)"
static void check_validation() {
    const int d = 3;
    for (int n = 1; n <= 3; ++n)
        for (int bad = -1; bad < n; ++bad)
            for (int defect = 0; defect < 9; ++defect) {
                if (bad < 0 && defect > 0) continue;
                std::vector<mrbf_round3_job> jobs;
                std::vector<DbInfo> info;
                for (int p = 0; p < n; ++p) {
                    jobs.push_back(make_job(2, 4, 3, false, 1, 0, MRBF_R3_UPDATE));
                    info.push_back(DbInfo{&g_dbs[p], d, 2, 10, true});
                }
                bool expect = bad >= 0;
                if (bad >= 0) {
                    mrbf_round3_job &jb = jobs[(size_t)bad];
                    DbInfo &di = info[(size_t)bad];
                    switch (defect) {
                        case 0: di.id = nullptr; break;
                        case 1: di.own = false; break;
                        case 2: di.d = d + 1; break;
                        case 3:
                            if (n < 2) expect = false;
                            else di.id = info[(size_t)((bad + 1) % n)].id;
                            break;
                        case 4: jb.x = nullptr; break;
                        case 5: jb.ub = nullptr; break;
                        case 6: jb.n_dirs = -1; break;
                        case 7: jb.mode = 2; break;
                        case 8: di.n = ((int64_t)1 << 31) - 64; break;  // two more rows would pass the row limit
                    }
                }
                const Defect df = check_jobs(n, d, jobs.data(), info.data(), 4);
                ++g_cases;
                CHECK((df.code == -4) == expect && (df.code == 0) == !expect);
                if (expect) CHECK(!df.msg.empty());
            }
    // a job whose own check fails (rc -3) is not a defect of the call
    mrbf_round3_job jb = make_job(3, 3, 2, false, 0, 0, MRBF_R3_UPDATE);
    DbInfo di{&g_dbs[0], d, 1, 0, true};
    CHECK(check_jobs(1, d, &jb, &di, 4).code == 0 && counts_of(jb, d).rc == -3);
}

struct Range {
    size_t lo, hi;
};
static bool disjoint(std::vector<Range> r) {
    std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i].lo < r[i - 1].hi) return false;
    return true;
}

// "room for the larger of the first attempt and the rebuild", "the kernels write only inside that reservation", by "the existing
// growth rule"; staging blocks, flag blocks and direction blocks of different starts do not overlap and lie inside their pieces; the
// pieces of the work buffer are in order, disjoint, 256-byte multiples; upload and read-back are each one contiguous range
static void check_layout() {
    const int ds[] = {1, 2, 3, 65, 128};
    const int64_t rows_of[] = {0, 1, 4, 63, 70}, caps_of[] = {0, 4, 64};
    const size_t desc_bytes = 104;
    long code = 0;
    for (int d : ds)
        for (int n = 1; n <= 4; ++n)
            for (int rep = 0; rep < 60; ++rep) {
                std::vector<mrbf_round3_job> jobs;
                std::vector<int64_t> rows, caps;
                std::vector<char> host;
                for (int p = 0; p < n; ++p, code += 7) {
                    const int nm = (int)(code % 7) - 1, mx = (int)(code / 7 % 7) - 1, nd = (int)(code / 49 % 6), flags = (int)(code / 3 % 4);
                    const int mode = code % 11 == 0 ? MRBF_R3_IMPROVE : MRBF_R3_UPDATE;
                    jobs.push_back(make_job(std::min(nm, d), mx, nd == 5 ? 0 : std::min(nd, d), nd == 5, flags & 1, flags >> 1, mode));
                    rows.push_back(rows_of[code % 5]);
                    caps.push_back(std::max(caps_of[code / 5 % 3], rows.back()));
                    host.push_back(code % 2 == 0);
                }
                const Layout L = layout(n, d, jobs.data(), rows.data(), caps.data(), reinterpret_cast<const bool *>(host.data()), desc_bytes);
                ++g_cases;
                std::vector<Range> stage, flags, dirs;
                int max1 = 0, max2 = 0;
                for (size_t p = 0; p < (size_t)n; ++p) {
                    const Counts c = counts_of(jobs[p], d);
                    CHECK(L.cnt[p].rc == c.rc && L.cnt[p].n1 == c.n1 && L.cnt[p].n2 == c.n2);
                    // the reservation: exactly the rows either attempt can write, and the growth rule's capacity holds them
                    CHECK(L.reserve[p] == rows[p] + std::max(c.rc ? 0 : c.n1, c.rc ? 0 : c.n2));
                    CHECK(L.capacity[p] == grow_capacity(caps[p], L.reserve[p]) && L.capacity[p] >= L.reserve[p]);
                    // every row offset a kernel forms (attempt rows i < n1, rebuild rows i < n2) lies inside the reservation
                    for (int i = 0; i < c.rows(); ++i) CHECK(rows[p] + i < L.reserve[p]);
                    CHECK(L.roff[p + 1] - L.roff[p] == c.rows());
                    stage.push_back({(size_t)L.roff[p] * d, (size_t)L.roff[p + 1] * d});
                    flags.push_back({(size_t)L.roff[p], (size_t)L.roff[p + 1]});
                    const bool up = c.rc == 0 && jobs[p].dirs && host[p];
                    CHECK(L.doff[p + 1] - L.doff[p] >= (up ? (int64_t)c.n1 * d : 0) && L.doff[p] % 2 == 0);
                    if (!up) CHECK(L.doff[p + 1] == L.doff[p]);
                    dirs.push_back({(size_t)L.doff[p], (size_t)L.doff[p + 1]});
                    // the uploaded columns are the ones the first attempt reads: the first n1, or with `reversed` the last n1
                    CHECK(L.first_col(p, 0) == 0 && L.first_col(p, 1) == c.n_dirs - c.n1 && L.first_col(p, 1) >= 0);
                    if (c.rc == 0) max1 = std::max(max1, c.n1), max2 = std::max(max2, c.n2);
                }
                CHECK(L.rows_max1 == max1 && L.rows_max2 == max2);
                CHECK(disjoint(stage) && disjoint(flags) && disjoint(dirs));
                const size_t R = (size_t)L.roff[(size_t)n];
                CHECK(L.oDesc == 0 && L.oXlu >= (size_t)n * desc_bytes && L.oDirs >= L.oXlu + (size_t)n * 3 * d * 8);
                CHECK(L.A.upload_bytes() >= L.oDirs + (size_t)L.doff[(size_t)n] * 8 && L.oOut == L.A.upload_bytes());
                CHECK(L.oStage >= L.oOut + (size_t)n * 16 && L.oFail >= L.oStage + R * d * 8 && L.A.back_bytes() == L.oFail - L.oOut);
                CHECK(L.A.total >= L.oFail + R * 4);
                for (size_t o : {L.oDesc, L.oXlu, L.oDirs, L.A.upload_bytes(), L.oOut, L.oStage, L.oFail, L.A.total}) CHECK(o % 256 == 0);
            }
}

int main() {
    check_counts();
    check_validation();
    check_layout();
    std::printf("round3_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("round3_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
