// Stand-alone host check of mrbf_eval_hessian_batch's host logic (morbit.jl_amd/csrc/hess_batch_host.hpp): the validation behind the
// call's return codes and every job's own status, the grouping key, the descriptors and first-block tables of the launches, the
// lookup a workgroup makes, the chunk rule and the layout of a chunk's arena.  Every case is judged by statements made directly from
// the header's text (include/mrbf.h "many-start model Hessians" and the comments of hess_batch_host.hpp), not by a second copy of
// the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/hess_batch_host_check.cpp -o /tmp/hbc && /tmp/hbc
// Enumerated: every defect of a job alone, in pairs within a job and across two jobs, with and without a foreign model; batches drawn
// from a pool of shapes (d = 1 .. 300, n = 1 .. 8192, m = 0 .. 4096, r = 1 .. 5, three kernel variants, host and device buffers, and
// jobs of up to 4e7 points that the 2^30 cut divides, one of them into two launches) in every order of a fixed walk; limits from 1 byte to 2 GiB.
#include <cstdio>
#include <cstring>
#include <set>

#include "../morbit.jl_amd/csrc/hess_batch_host.hpp"

using namespace mrbf::hessbatch;
namespace hs = mrbf::hess;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static const int32_t ROWS_OK[] = {2, 0, 2}, ROWS_HIGH[] = {0, 3, 1}, ROWS_NEG[] = {1, -1, 0};
static const size_t DD = 19;  // doubles of a descriptor, as the library's is

static Job good_job() {
    Job J;
    J.has_model = true;
    J.m = 5, J.n = 40, J.d = 7, J.k = 3;
    J.X = J.out = true;
    J.n_rows = 3, J.rows = ROWS_OK;
    return J;
}

// defects in the order of the single call's codes; the earlier one wins when a job has two
enum Defect { NO_MODEL, NEG_M, NEG_ROWS, NULL_ROWS, ROW_HIGH, ROW_NEG, NO_X, NO_OUT, N_DEFECTS };
static const int CODE[N_DEFECTS] = {-2, -3, -5, -5, -6, -6, -4, -7};

static void apply(Job &J, int defect) {
    switch (defect) {
        case NO_MODEL: J.has_model = false; break;
        case NEG_M: J.m = -1; break;
        case NEG_ROWS: J.n_rows = -1; break;
        case NULL_ROWS: J.rows = nullptr; break;
        case ROW_HIGH: J.rows = ROWS_HIGH; break;
        case ROW_NEG: J.rows = ROWS_NEG; break;
        case NO_X: J.X = false; break;
        case NO_OUT: J.out = false; break;
    }
}

static void check_validate() {
    int64_t which = 7;
    CHECK(validate(nullptr, 3, nullptr, &which) == -3 && which == -1);  // `jobs` NULL
    for (int a = -1; a < N_DEFECTS; ++a)
        for (int b = -1; b < N_DEFECTS; ++b)
            for (int foreign = 0; foreign < 4; ++foreign) {
                // job 0: defect a (and b in the same job when two = 0); job 2: defect b when two = 1; job 1 always valid
                for (int two = 0; two < 2; ++two) {
                    const bool a_rows = a == NULL_ROWS || a == ROW_HIGH || a == ROW_NEG, b_rows = b == NULL_ROWS || b == ROW_HIGH || b == ROW_NEG;
                    if (!two && a_rows && b_rows && a != b) continue;  // one job has one row list
                    Job jobs[3] = {good_job(), good_job(), good_job()};
                    if (a >= 0) apply(jobs[0], a);
                    if (b >= 0) apply(jobs[two ? 2 : 0], b);
                    jobs[0].foreign = foreign & 1, jobs[1].foreign = (foreign & 2) != 0;
                    int32_t st[3] = {9, 9, 9};
                    which = 9;
                    const int rc = validate(jobs, 3, st, &which);
                    ++g_cases;
                    int want0, want2;
                    if (two) {
                        want0 = a >= 0 ? CODE[a] : 0, want2 = b >= 0 ? CODE[b] : 0;
                    } else {
                        // two defects of one job: the earlier code wins (m < 0 in front of the NULL X / NULL hess_out that count with m > 0)
                        const int first = a >= 0 && b >= 0 ? (a < b ? a : b) : (a >= 0 ? a : b);
                        want0 = first >= 0 ? CODE[first] : 0, want2 = 0;
                    }
                    const bool invalid = want0 != 0 || want2 != 0;
                    if (invalid) {
                        CHECK(rc == -3);  // -3 goes in front of -4
                        CHECK(st[0] == want0 && st[1] == 0 && st[2] == want2);  // every job's own status, a foreign model not among them
                        CHECK(which == (want0 != 0 ? 0 : 2));
                    } else if (foreign) {
                        CHECK(rc == -4 && which == ((foreign & 1) ? 0 : 1));
                    } else {
                        CHECK(rc == 0 && st[0] == 0 && st[1] == 0 && st[2] == 0);
                    }
                }
            }
    // an m = 0 job needs neither X nor hess_out and is not active
    Job J = good_job();
    J.m = 0, J.X = J.out = false;
    CHECK(job_status(J) == 0 && !active(J) && need_doubles(J, DD) == 0);
    J.m = 1;
    CHECK(job_status(J) == -4);
    J.X = true;
    CHECK(job_status(J) == -7);
    // NULL rows with n_rows = 0 selects all k outputs
    J = good_job();
    J.n_rows = 0, J.rows = nullptr;
    CHECK(job_status(J) == 0 && outputs(J) == 3);
}

// ---- a pool of shapes
static Job shape(int64_t m, int64_t n, int d, int k, int r, int variant, bool xdev, bool odev) {
    Job J;
    J.has_model = true;
    J.m = m, J.n = n, J.d = d, J.k = k, J.variant = variant;
    J.X = J.out = true, J.X_dev = xdev, J.out_dev = odev;
    J.n_rows = r == k ? 0 : r, J.rows = r == k ? nullptr : ROWS_OK;  // (the tables read the count alone)
    return J;
}

static std::vector<Job> pool() {
    std::vector<Job> P;
    const int ds[] = {1, 16, 64, 65, 129, 300};
    const int64_t ns[] = {1, 33, 257, 8192};
    const int64_t ms[] = {0, 1, 3, 64, 4096};
    int t = 0;
    for (int d : ds)
        for (int64_t n : ns)
            for (int64_t m : ms) {
                const int r = 1 + t % 5;
                P.push_back(shape(m, n, d, 5, r, t % 3, (t & 1) != 0, (t & 2) != 0));
                ++t;
            }
    // jobs the 2^30 cut divides (device buffers: nobody holds that many Hessians on the host); the first has more than 2^30 blocks
    P.push_back(shape(40000000, 100, 300, 5, 5, 1, true, true));
    P.push_back(shape(((int64_t)1 << 26) + 5, 64, 1, 1, 1, 0, true, true));
    P.push_back(shape(((int64_t)1 << 25) + 1, 64, 65, 2, 2, 2, true, true));
    return P;
}

// the tables of one chunk, judged by the header's sentences
static void check_tables(const std::vector<Job> &jobs, int64_t first, int64_t count) {
    for (int reduce = 0; reduce < 2; ++reduce) {
        const Table T = table(jobs.data(), first, count, reduce != 0);
        ++g_cases;
        // every block of every active job (of every split job, for the combining kernel) exactly once and in order
        std::vector<int64_t> next_point((size_t)count, 0);
        std::vector<bool> seen((size_t)count, false);
        size_t covered = 0;
        std::set<int> keys_closed;
        for (size_t li = 0; li < T.launches.size(); ++li) {
            const Launch &L = T.launches[li];
            CHECK(L.first == covered && L.count >= 1);
            CHECK(L.grid >= 1 && L.grid <= MAX_GRID);  // no grid above 2^30
            CHECK(T.first_block[L.table] == 0 && T.first_block[L.table + L.count] == (uint32_t)L.grid);
            if (li > 0 && T.launches[li - 1].key != L.key) keys_closed.insert(T.launches[li - 1].key);
            CHECK(!keys_closed.count(L.key));  // a key's launches are adjacent
            // ... and a key is cut into two launches only where the next descriptor would not fit
            if (li > 0 && T.launches[li - 1].key == L.key) CHECK(T.launches[li - 1].grid + T.items[L.first].blocks > MAX_GRID);
            int64_t at = 0;
            for (size_t t = L.first; t < L.first + L.count; ++t) {
                const Item &it = T.items[t];
                const Job &J = jobs[(size_t)it.job];
                CHECK(it.job >= first && it.job < first + count && active(J));
                CHECK(it.key == (reduce ? reduce_key(J) : main_key(J)) && it.key == L.key);
                if (reduce) CHECK(split(J) > 1);
                CHECK(it.cnt >= 1 && it.p0 == next_point[(size_t)(it.job - first)]);  // a job's points in order, none twice
                next_point[(size_t)(it.job - first)] = it.p0 + it.cnt;
                seen[(size_t)(it.job - first)] = true;
                const int r = outputs(J);
                const int64_t per_point = reduce ? (int64_t)hs::npass(r) * hs::npairs(J.d) * hs::rb(r) * 16
                                                 : (int64_t)hs::npass(r) * hs::npairs(J.d) * hs::nsplit(J.m, J.n, J.d, r);
                CHECK(it.blocks == it.cnt * per_point && it.blocks >= 1 && it.blocks <= MAX_GRID);
                if (split(J) > 1) CHECK(it.p0 == 0 && it.cnt == J.m);  // a split job is never cut: its partial blocks have one owner
                CHECK(T.first_block[L.table + (t - L.first)] == (uint32_t)at);
                // the lookup: first, last and boundary blocks
                uint32_t local = 77;
                const uint32_t *tb = &T.first_block[L.table];
                const int nd = (int)L.count, me = (int)(t - L.first);
                CHECK(lookup(tb, nd, (uint32_t)at, &local) == me && local == 0);
                CHECK(lookup(tb, nd, (uint32_t)(at + it.blocks - 1), &local) == me && local == (uint32_t)(it.blocks - 1));
                if (it.blocks > 2) CHECK(lookup(tb, nd, (uint32_t)(at + it.blocks / 2), &local) == me && local == (uint32_t)(it.blocks / 2));
                if (me > 0) CHECK(lookup(tb, nd, (uint32_t)(at - 1), &local) == me - 1);
                if (me + 1 < nd) CHECK(lookup(tb, nd, (uint32_t)(at + it.blocks), &local) == me + 1 && local == 0);
                at += it.blocks;
                // jobs of a key keep the batch's order
                if (t > L.first && T.items[t - 1].job != it.job) CHECK(T.items[t - 1].job < it.job);
            }
            CHECK(at == L.grid);
            covered += L.count;
        }
        CHECK(covered == T.items.size());
        size_t entries = 0;
        for (const Launch &L : T.launches) entries += L.count + 1;
        CHECK(entries == T.first_block.size());
        for (int64_t i = 0; i < count; ++i) {
            const Job &J = jobs[(size_t)(first + i)];
            const bool due = active(J) && (!reduce || split(J) > 1);
            CHECK(seen[(size_t)i] == due);
            if (due) CHECK(next_point[(size_t)i] == J.m);
        }
    }
}

static void check_layout(const std::vector<Job> &jobs, int64_t first, int64_t count, size_t need_sum) {
    const Table mt = table(jobs.data(), first, count, false), rt = table(jobs.data(), first, count, true);
    const Layout L = layout(jobs.data(), first, count, mt, rt, DD);
    ++g_cases;
    // pieces in the order of the header, disjoint, aligned, within total
    struct Piece {
        size_t at, cnt;
    };
    std::vector<Piece> pieces;
    pieces.push_back({L.main_desc, mt.items.size() * DD});
    pieces.push_back({L.red_desc, rt.items.size() * DD});
    pieces.push_back({L.main_table, (mt.first_block.size() + 1) / 2});
    pieces.push_back({L.red_table, (rt.first_block.size() + 1) / 2});
    CHECK(L.at.size() == (size_t)count);
    for (int64_t i = 0; i < count; ++i) {
        const Job &J = jobs[(size_t)(first + i)];
        CHECK((L.at[(size_t)i].rows != NONE) == active(J));
        if (active(J)) pieces.push_back({L.at[(size_t)i].rows, ((size_t)outputs(J) + 1) / 2});
    }
    for (int64_t i = 0; i < count; ++i) {
        const Job &J = jobs[(size_t)(first + i)];
        CHECK((L.at[(size_t)i].X != NONE) == (active(J) && !J.X_dev));
        if (L.at[(size_t)i].X != NONE) pieces.push_back({L.at[(size_t)i].X, (size_t)J.m * J.d});
    }
    const size_t n_up = pieces.size();
    for (int64_t i = 0; i < count; ++i) {
        const Job &J = jobs[(size_t)(first + i)];
        CHECK((L.at[(size_t)i].part != NONE) == (active(J) && split(J) > 1));
        if (L.at[(size_t)i].part != NONE)
            pieces.push_back({L.at[(size_t)i].part, (size_t)J.m * hs::npass(outputs(J)) * hs::npairs(J.d) * split(J) * hs::rb(outputs(J)) * 64 * 64});
    }
    const size_t n_part = pieces.size();
    for (int64_t i = 0; i < count; ++i) {
        const Job &J = jobs[(size_t)(first + i)];
        CHECK((L.at[(size_t)i].out != NONE) == (active(J) && !J.out_dev));
        if (L.at[(size_t)i].out != NONE) pieces.push_back({L.at[(size_t)i].out, (size_t)J.m * outputs(J) * J.d * J.d});
    }
    size_t end = 0;
    for (size_t p = 0; p < pieces.size(); ++p) {
        CHECK(pieces[p].at % 16 == 0);
        CHECK(pieces[p].at >= end);  // disjoint and in order
        end = pieces[p].at + pieces[p].cnt;
        if (p + 1 == n_up) CHECK(end <= L.up_cnt);
        if (p == n_up) CHECK(pieces[p].at >= L.up_cnt);
        if (p == n_part) CHECK(pieces[p].at >= L.out0);
    }
    CHECK(end <= L.total && L.total % 16 == 0 && L.up_cnt % 16 == 0 && L.out0 % 16 == 0);
    CHECK(L.out0 + L.out_cnt == L.total && L.up_cnt <= L.out0);
    CHECK(L.total <= need_sum);  // what the chunk rule counted covers what the layout takes
}

static void check_batches() {
    const std::vector<Job> P = pool();
    const size_t limits[] = {1, 4096, (size_t)1 << 20, (size_t)24 << 20, (size_t)2 << 30};
    // a fixed walk through the pool: batches of 1 .. 9 jobs at strides that mix every shape with every other
    for (size_t stride = 1; stride <= 11; stride += 2)
        for (size_t len = 1; len <= 9; ++len)
            for (size_t start = 0; start < P.size(); start += 5) {
                std::vector<Job> jobs;
                for (size_t i = 0; i < len; ++i) jobs.push_back(P[(start + i * stride) % P.size()]);
                std::vector<size_t> need;
                for (const Job &J : jobs) need.push_back(need_doubles(J, DD));
                check_tables(jobs, 0, (int64_t)jobs.size());
                for (size_t limit : limits) {
                    const std::vector<Chunk> C = chunks(need, limit);
                    ++g_cases;
                    int64_t next = 0;
                    for (size_t c = 0; c < C.size(); ++c) {
                        CHECK(C[c].first == next && C[c].count >= 1);  // the jobs in order, none twice
                        next += C[c].count;
                        size_t sum = 0;
                        for (int64_t i = C[c].first; i < C[c].first + C[c].count; ++i) sum += need[(size_t)i];
                        // within the limit, except single-job chunks, which run the single call's chain
                        CHECK(C[c].single == (sum * sizeof(double) > limit / sizeof(double) * sizeof(double) && C[c].count == 1));
                        if (sum > limit / sizeof(double)) CHECK(C[c].count == 1 && C[c].single);
                        // closed only in front of the job that would carry it beyond the limit
                        if (c + 1 < C.size()) CHECK(sum + need[(size_t)(C[c].first + C[c].count)] > limit / sizeof(double));
                        if (!C[c].single) {
                            check_tables(jobs, C[c].first, C[c].count);
                            check_layout(jobs, C[c].first, C[c].count, sum);
                        }
                    }
                    CHECK(next == (int64_t)jobs.size());
                }
            }
    // keys: n, d, k and the kernel's parameters split no group; the variant and the pass width do
    Job a = shape(1, 65, 65, 2, 2, 1, false, false), b = shape(1, 257, 300, 7, 2, 1, true, false);
    CHECK(main_key(a) == main_key(b) && reduce_key(a) == reduce_key(b));
    b.variant = 2;
    CHECK(main_key(a) != main_key(b) && reduce_key(a) == reduce_key(b));
    Job c = shape(1, 65, 65, 3, 3, 1, false, false), e = shape(1, 65, 65, 5, 5, 1, false, false);
    CHECK(main_key(c) == main_key(e) && main_key(c) != main_key(a) && reduce_key(c) != reduce_key(a));
    // the many-start case: one radial function, one r, any mix of n: one main launch and one combining launch
    std::vector<Job> starts;
    const int64_t nn[] = {65, 66, 97, 129, 257};
    for (int64_t n : nn) starts.push_back(shape(1, n, 65, 2, 2, 1, false, false));
    CHECK(table(starts.data(), 0, 5, false).launches.size() == 1 && table(starts.data(), 0, 5, true).launches.size() == 1);
    // several launches of one key: 72 descriptors, 1.2e9 blocks
    std::vector<Job> big(1, shape(40000000, 100, 300, 5, 5, 1, true, true));
    const Table T = table(big.data(), 0, 1, false);
    CHECK(T.launches.size() > 1 && T.items.size() == desc_count(big[0]));
}

int main() {
    check_validate();
    check_batches();
    if (g_failed) {
        std::printf("hess_batch_host_check: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("hess_batch_host_check: ok (%ld cases)\n", g_cases);
    return 0;
}
