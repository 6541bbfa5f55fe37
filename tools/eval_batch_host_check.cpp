// Stand-alone host check of mrbf_eval_batch's host logic (morbit.jl_amd/csrc/eval_batch_host.hpp): the validation behind the call's
// return codes, which jobs do any work, the rule that cuts a batch into chunks of consecutive jobs, and the layout of a chunk's arena.
// Every case is judged by statements made directly from the header's text (include/mrbf.h "many-start evaluation" and the comments of
// eval_batch_host.hpp), not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/eval_batch_host_check.cpp -o /tmp/eval_batch_host_check && /tmp/eval_batch_host_check
// Enumerated: batches of 1 .. 3 jobs with each defect in each position; every chunk rule input of up to 6 jobs with sizes from
// {0, 1, 5, 16, 17, 40} (in doubles) against limits of 0 .. 48 doubles; layouts of 1 .. 3 jobs over every mix of host / device / absent
// buffers, m in {0, 1, 7, 64}, (d, k) in {(1, 1), (3, 2), (65, 17)}, first job at 0 or 1 of the batch.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../morbit.jl_amd/csrc/eval_batch_host.hpp"

using namespace mrbf::evalbatch;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                                     \
    } while (0)

static Job good_job(int64_t m) {
    Job J;
    J.has_model = true, J.m = m, J.d = 3, J.k = 2;
    J.X = m > 0, J.vals = true;
    return J;
}

// "-3 for an invalid job: NULL model, m < 0, or NULL X with m > 0"; "-4 for a model of another context"; m == 0 with NULL X is legal,
// and so is a job with both outputs NULL; -3 is reported in front of -4 whatever the positions
static void check_validate() {
    for (int n = 1; n <= 3; ++n)
        for (int pos = 0; pos < n; ++pos)
            for (int defect = 0; defect <= 6; ++defect) {
                std::vector<Job> jobs;
                for (int i = 0; i < n; ++i) jobs.push_back(good_job(1 + i));
                Job &J = jobs[(size_t)pos];
                int want = 0;
                switch (defect) {
                    case 0: break;
                    case 1: J.has_model = false, want = -3; break;
                    case 2: J.m = -1, want = -3; break;
                    case 3: J.X = false, want = -3; break;           // m > 0
                    case 4: J.m = 0, J.X = false; break;             // legal
                    case 5: J.vals = false, J.jac = false; break;    // legal: does nothing
                    case 6: J.foreign = true, want = -4; break;
                }
                int64_t which = -1;
                const int rc = validate(jobs.data(), n, &which);
                ++g_cases;
                CHECK(rc == want);
                if (want != 0) CHECK(which == pos);
                CHECK(validate(jobs.data(), n, nullptr) == want);
                if (defect == 6 && n >= 2) {  // an invalid job anywhere wins over a foreign model
                    jobs[(size_t)((pos + 1) % n)].m = -5;
                    CHECK(validate(jobs.data(), n, &which) == -3 && which == (pos + 1) % n);
                }
                if (defect == 4 || defect == 5) CHECK(!active(J));
                if (defect == 0) CHECK(active(J));
            }
}

// "chunks of consecutive jobs that cover 0 .. n_jobs - 1 in order"; "a chunk is closed in front of the job that would carry its arena
// beyond the limit"; "a single job beyond the limit is a chunk of its own"
static void check_chunks() {
    const size_t sizes[] = {0, 1, 5, 16, 17, 40};
    const int A = 6;
    for (int n = 0; n <= 6; ++n) {
        long combos = 1;
        for (int i = 0; i < n; ++i) combos *= A;
        for (long c = 0; c < combos; c += (n >= 5 ? 7 : 1)) {
            std::vector<size_t> need((size_t)n);
            long r = c;
            for (int i = 0; i < n; ++i) need[(size_t)i] = sizes[r % A], r /= A;
            for (size_t limit = 0; limit <= 48; ++limit) {
                const auto ch = chunks(need, limit * sizeof(double));
                ++g_cases;
                int64_t next = 0;
                for (size_t j = 0; j < ch.size(); ++j) {
                    CHECK(ch[j].first == next && ch[j].second >= 1);
                    size_t sum = 0;
                    for (int64_t i = ch[j].first; i < ch[j].first + ch[j].second; ++i) sum += need[(size_t)i];
                    CHECK(sum <= limit || ch[j].second == 1);                      // within the limit, or a single job
                    next = ch[j].first + ch[j].second;
                    if (j + 1 < ch.size()) CHECK(sum + need[(size_t)next] > limit);  // closed only where the next job would not fit
                }
                CHECK(next == n);
                if (n == 0) CHECK(ch.empty());
            }
        }
    }
    // the call's own limit: 2 GiB
    CHECK(ARENA_LIMIT_BYTES == (size_t)2 << 30);
    CHECK(chunks({1, 1, 1}).size() == 1);
    const size_t half = ARENA_LIMIT_BYTES / sizeof(double) / 2;
    CHECK(chunks({half, half, 16}).size() == 2);   // C4's host-side Jacobians, 64 x 6450: more than one chunk
    CHECK(chunks(std::vector<size_t>(64, (size_t)6450 * 2 * 128)).size() == 1);
    CHECK(chunks(std::vector<size_t>(64, (size_t)6450 * 2 * 128 * 4)).size() > 1);
}

// "descriptors | host-side query rows: one upload; evaluation scratch; host-side values | host-side Jacobians: one read-back";
// "every piece a multiple of 16"; "buffers the caller keeps on the device have no place in the arena"; an inactive job has no place
static void check_layout() {
    const int64_t ms[] = {0, 1, 7, 64};
    const int dk[][2] = {{1, 1}, {3, 2}, {65, 17}};
    // a buffer is 0 absent, 1 host, 2 device; X absent only with m == 0
    for (int n = 1; n <= 3; ++n) {
        long combos = 1;
        for (int i = 0; i < n; ++i) combos *= 2 * 3 * 3 * 4 * 3;
        const long stride = n == 3 ? 101 : (n == 2 ? 3 : 1);
        for (long c = 0; c < combos; c += stride)
            for (int64_t first = 0; first <= 1; ++first) {
                std::vector<Job> jobs((size_t)(first + n));
                jobs[0] = good_job(5);  // (the job in front of the chunk when first == 1: must not show in the layout)
                long r = c;
                for (int i = 0; i < n; ++i) {
                    Job &J = jobs[(size_t)(first + i)];
                    const int xs = 1 + r % 2; r /= 2;
                    const int vs = r % 3; r /= 3;
                    const int js = r % 3; r /= 3;
                    J.m = ms[r % 4]; r /= 4;
                    J.d = dk[r % 3][0], J.k = dk[r % 3][1]; r /= 3;
                    J.has_model = true;
                    J.X = true, J.X_dev = xs == 2;
                    J.vals = vs != 0, J.vals_dev = vs == 2;
                    J.jac = js != 0, J.jac_dev = js == 2;
                }
                const size_t desc = 21 * (size_t)n, scratch = 33 * (size_t)n;
                const Layout L = layout(jobs.data(), first, n, desc, scratch);
                ++g_cases;
                CHECK(L.at.size() == (size_t)n);
                // the pieces, in order, disjoint, each a multiple of 16 long and inside [0, total)
                struct Piece {
                    size_t at, cnt;
                    int region;  // 0 upload, 1 scratch, 2 read-back
                };
                std::vector<Piece> pieces;
                pieces.push_back({L.desc, desc, 0});
                pieces.push_back({L.scratch, scratch, 1});
                for (int i = 0; i < n; ++i) {
                    const Job &J = jobs[(size_t)(first + i)];
                    const Place &P = L.at[(size_t)i];
                    const bool act = J.m > 0 && (J.vals || J.jac);
                    CHECK((P.X != NONE) == (act && !J.X_dev));
                    CHECK((P.vals != NONE) == (act && J.vals && !J.vals_dev));
                    CHECK((P.jac != NONE) == (act && J.jac && !J.jac_dev));
                    if (P.X != NONE) pieces.push_back({P.X, (size_t)J.m * J.d, 0});
                    if (P.vals != NONE) pieces.push_back({P.vals, (size_t)J.m * J.k, 2});
                    if (P.jac != NONE) pieces.push_back({P.jac, (size_t)J.m * J.k * J.d, 2});
                }
                std::sort(pieces.begin(), pieces.end(), [](const Piece &a, const Piece &b) { return a.at < b.at; });
                size_t end = 0;
                int region = 0;
                for (const Piece &p : pieces) {
                    CHECK(p.at % 16 == 0 && p.at >= end && p.region >= region);
                    end = p.at + p.cnt, region = p.region;
                    if (p.region == 0) CHECK(p.at + p.cnt <= L.up_cnt);
                    if (p.region == 1) CHECK(p.at >= L.up_cnt && p.at + p.cnt <= L.out0);
                    if (p.region == 2) CHECK(p.at >= L.out0 && p.at + p.cnt <= L.out0 + L.out_cnt);
                }
                CHECK(L.desc == 0 && L.up_cnt % 16 == 0 && L.out0 % 16 == 0 && L.total % 16 == 0);
                CHECK(L.out0 + L.out_cnt == L.total && end <= L.total);
                // a chunk of device-resident buffers alone: descriptors and scratch, nothing else
                bool any_host = false;
                for (int i = 0; i < n; ++i) any_host = any_host || L.at[(size_t)i].X != NONE || L.at[(size_t)i].vals != NONE || L.at[(size_t)i].jac != NONE;
                if (!any_host) CHECK(L.up_cnt == pad16(desc) && L.out_cnt == 0 && L.total == pad16(desc) + pad16(scratch));
            }
    }
}

int main() {
    check_validate();
    check_chunks();
    check_layout();
    std::printf("eval_batch_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("eval_batch_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
