// Host logic of mrbf_eval_hessian_batch (hess.hip), free of HIP so that tools/hess_batch_host_check.cpp drives it on the CPU under the
// sanitizers: what the call is told of a job, the validation behind its return codes and every job's own status, which jobs do any
// work, the key that decides which jobs share a launch, the descriptors and first-block tables of the launches (with the cut that keeps
// every grid at or below 2^30 blocks), the lookup a workgroup makes in such a table, the rule that cuts a batch into chunks of
// consecutive jobs, and the layout of a chunk's arena
//     descriptors | block tables | row lists (int32) | host-side query rows        one upload
//     partial blocks of the split jobs
//     host-side results                                                           one read-back
// counted in doubles, every piece a multiple of 16.  Buffers the caller keeps on the device have no place in the arena: the
// descriptors carry their addresses.  Every job has the shape of the single call it stands for (hess_host.hpp: nsplit, npass, npairs).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "hess_host.hpp"

#ifndef MRBF_HD
#define MRBF_HD  // hess.hip: __host__ __device__, so that the kernels make the lookup the check enumerates
#endif

namespace mrbf {
namespace hessbatch {

constexpr size_t ARENA_LIMIT_BYTES = (size_t)2 << 30;  // a call whose arena would exceed this is processed in chunks of jobs
constexpr int64_t MAX_GRID = (int64_t)1 << 30;         // most blocks of one launch
constexpr size_t NONE = ~(size_t)0;

// what the call knows of a job before anything is launched
struct Job {
    bool has_model = false;  // jobs[i].model != NULL
    bool foreign = false;    // the model was created through another context
    int64_t m = 0;
    int64_t n = 0;           // the model's centres, dimension, outputs
    int d = 0, k = 0;
    int variant = 0;         // the instantiation of the main kernel the model's radial function takes, without the pass width
    bool X = false, out = false;          // pointer given
    bool X_dev = false, out_dev = false;  // ... and device memory
    int32_t n_rows = 0;
    const int32_t *rows = nullptr;
};

using hess::pad16;

// a job's own status: what mrbf_eval_hessian would have returned for it on its own context (-2, -3, -5, -6, -4, -7 in the single
// call's precedence; 0 for a valid job)
inline int job_status(const Job &J) {
    hess::Call c;
    c.has_ctx = true, c.has_model = J.has_model, c.foreign = false;
    c.m = J.m, c.k = J.k, c.X = J.X, c.out = J.out, c.n_rows = J.n_rows, c.rows = J.rows;
    return hess::validate(c);
}

// 0, or the call's return code with the first offending job in *which: -3 (`jobs` NULL, or a job with a status of its own), then -4 (a
// model of another context).  status (may be NULL; n_jobs entries) receives every job's own status whenever the answer is 0 or -3 with
// jobs given.  All jobs are looked at before anything is launched or written.
inline int validate(const Job *jobs, int64_t n_jobs, int32_t *status, int64_t *which) {
    if (!jobs) {
        if (which) *which = -1;
        return -3;
    }
    int rc = 0;
    for (int64_t i = n_jobs - 1; i >= 0; --i) {
        const int s = job_status(jobs[i]);
        if (status) status[i] = s;
        if (s) {
            rc = -3;
            if (which) *which = i;
        }
    }
    if (rc) return rc;
    for (int64_t i = 0; i < n_jobs; ++i)
        if (jobs[i].foreign) {
            if (which) *which = i;
            return -4;
        }
    return 0;
}

// a job that launches something
inline bool active(const Job &J) { return J.m > 0; }

// the shape of a validated job: selected outputs, pieces of the centre range and their length -- the single call's
inline int outputs(const Job &J) { return J.n_rows > 0 ? J.n_rows : J.k; }
inline int split(const Job &J, int64_t *per = nullptr) { return hess::nsplit(J.m, J.n, J.d, outputs(J), per); }

// Jobs share a launch where they share the kernel's template instantiation: (variant, pass width) for the main kernel, the pass width
// alone for the combining kernel.  n, d, k and the radial function's parameters travel in the descriptor and split no group.
inline int main_key(const Job &J) { return J.variant * 8 + hess::rb(outputs(J)); }
inline int reduce_key(const Job &J) { return hess::rb(outputs(J)); }

// ---- descriptors and first-block tables
// A descriptor stands for points p0 .. p0 + cnt - 1 of a job.  A job is cut where the single call cuts it: at most
// max(1, 2^30 / (64 blocks_per_point)) points per descriptor, which keeps both the main kernel's and the combining kernel's blocks of
// a descriptor at or below 2^30.  A split job (fewer than hess::TARGET_WGS workgroups per piece, at most 64 pieces) is never cut, so the
// partial blocks of a job belong to one descriptor.
struct Item {
    int64_t job = 0, p0 = 0, cnt = 0;
    int64_t blocks = 0;  // of the kernel the table is for
    int key = 0;
};
struct Launch {
    int key = 0;
    size_t first = 0, count = 0;  // items [first, first + count)
    size_t table = 0;             // its count + 1 first-block entries start here: 0, ..., grid
    int64_t grid = 0;
};
struct Table {
    std::vector<Item> items;  // in launch order
    std::vector<Launch> launches;
    std::vector<uint32_t> first_block;
};

inline int64_t points_per_desc(const Job &J) {
    const int r = outputs(J);
    const int64_t per_point = (int64_t)hess::npass(r) * hess::npairs(J.d) * split(J);
    return std::max<int64_t>(1, MAX_GRID / (per_point * 64));
}
inline int64_t main_blocks(const Job &J, int64_t cnt) { return cnt * hess::npass(outputs(J)) * hess::npairs(J.d) * split(J); }
inline int64_t reduce_blocks(const Job &J, int64_t cnt) {
    return cnt * hess::npass(outputs(J)) * hess::npairs(J.d) * hess::rb(outputs(J)) * 16;
}

// the launches of jobs first .. first + count - 1: items in job order within a key, keys ascending; a launch is closed where the key
// changes and in front of the item that would carry its grid beyond MAX_GRID.  reduce: the combining kernel's table (split jobs only).
inline Table table(const Job *jobs, int64_t first, int64_t count, bool reduce) {
    Table T;
    for (int64_t i = first; i < first + count; ++i) {
        const Job &J = jobs[i];
        if (!active(J) || (reduce && split(J) <= 1)) continue;
        const int64_t most = points_per_desc(J);
        for (int64_t p0 = 0; p0 < J.m; p0 += most) {
            Item it;
            it.job = i, it.p0 = p0, it.cnt = std::min(most, J.m - p0);
            it.blocks = reduce ? reduce_blocks(J, it.cnt) : main_blocks(J, it.cnt);
            it.key = reduce ? reduce_key(J) : main_key(J);
            T.items.push_back(it);
        }
    }
    std::stable_sort(T.items.begin(), T.items.end(), [](const Item &a, const Item &b) { return a.key < b.key; });
    for (size_t i = 0; i < T.items.size(); ++i) {
        const Item &it = T.items[i];
        if (T.launches.empty() || T.launches.back().key != it.key || T.launches.back().grid + it.blocks > MAX_GRID) {
            if (!T.launches.empty()) T.first_block.push_back((uint32_t)T.launches.back().grid);
            Launch L;
            L.key = it.key, L.first = i, L.table = T.first_block.size();
            T.launches.push_back(L);
        }
        Launch &L = T.launches.back();
        T.first_block.push_back((uint32_t)L.grid);
        L.grid += it.blocks, ++L.count;
    }
    if (!T.launches.empty()) T.first_block.push_back((uint32_t)T.launches.back().grid);
    return T;
}

// The lookup of a workgroup: the descriptor i of a launch with first-block entries tb[0] = 0 <= tb[1] <= ... <= tb[nd] = grid for which
// tb[i] <= block < tb[i + 1] (every descriptor has at least one block, so i is unique); *local: the block's index within it.
MRBF_HD inline int lookup(const uint32_t *tb, int nd, uint32_t block, uint32_t *local) {
    int lo = 0, hi = nd;  // tb[lo] <= block < tb[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb[mid] <= block) lo = mid;
        else hi = mid;
    }
    *local = block - tb[lo];
    return lo;
}

// ---- what a job adds to an arena, piece by piece (doubles)
inline size_t rows_doubles(const Job &J) { return active(J) ? pad16(((size_t)outputs(J) + 1) / 2) : 0; }
inline size_t upload_doubles(const Job &J) { return active(J) && !J.X_dev ? pad16((size_t)J.m * J.d) : 0; }
inline size_t part_doubles(const Job &J) { return active(J) ? pad16(hess::partial_doubles(J.m, J.d, outputs(J), split(J))) : 0; }
inline size_t out_doubles(const Job &J) { return active(J) && !J.out_dev ? pad16((size_t)J.m * outputs(J) * J.d * J.d) : 0; }
// ... its descriptors in both tables (desc_doubles: doubles of one descriptor) and its first-block entries, each table's closing entry
// counted with every descriptor
inline size_t desc_count(const Job &J) { return active(J) ? (size_t)hess::ceil_div(J.m, points_per_desc(J)) : 0; }
inline size_t need_doubles(const Job &J, size_t desc_doubles) {
    if (!active(J)) return 0;
    const size_t nd = desc_count(J), nr = split(J) > 1 ? nd : 0;
    return pad16(nd * desc_doubles) + pad16(nr * desc_doubles) + pad16(nd) + pad16(nr) + rows_doubles(J) + upload_doubles(J) +
           part_doubles(J) + out_doubles(J);
}

// Chunks of consecutive jobs that cover 0 .. n_jobs - 1 in order: a chunk is closed in front of the job that would carry its arena
// beyond limit_bytes.  need[i]: need_doubles of job i.  A single job beyond the limit is a chunk of its own and runs the single call's
// chain, with its own staging rule, inside the call (`single`).  limit_bytes is an argument so that a test can cut a small batch.
struct Chunk {
    int64_t first = 0, count = 0;
    bool single = false;
};
inline std::vector<Chunk> chunks(const std::vector<size_t> &need, size_t limit_bytes = ARENA_LIMIT_BYTES) {
    std::vector<Chunk> out;
    const size_t limit = limit_bytes / sizeof(double);
    int64_t first = 0;
    size_t sum = 0;
    auto close = [&](int64_t end) {
        Chunk c;
        c.first = first, c.count = end - first, c.single = c.count == 1 && sum > limit;
        out.push_back(c);
    };
    for (int64_t i = 0; i < (int64_t)need.size(); ++i) {
        if (i > first && sum + need[(size_t)i] > limit) {
            close(i);
            first = i, sum = 0;
        }
        sum += need[(size_t)i];
    }
    if ((int64_t)need.size() > first) close((int64_t)need.size());
    return out;
}

// where a job's pieces live in the chunk's arena (offsets in doubles; NONE: in place on the device, or nothing to keep)
struct Place {
    size_t rows = NONE, X = NONE, part = NONE, out = NONE;
};
struct Layout {
    size_t main_desc = 0, red_desc = 0;    // the two descriptor arrays
    size_t main_table = 0, red_table = 0;  // the two first-block tables (uint32)
    size_t up_cnt = 0;                     // the upload: [0, up_cnt)
    size_t out0 = 0, out_cnt = 0;          // the read-back block: [out0, out0 + out_cnt)
    size_t total = 0;
    std::vector<Place> at;  // per job of the chunk
};

inline Layout layout(const Job *jobs, int64_t first, int64_t count, const Table &main, const Table &red, size_t desc_doubles) {
    Layout L;
    L.at.resize((size_t)count);
    size_t o = 0;
    auto take = [&](size_t cnt) {
        const size_t at = o;
        o += pad16(cnt);
        return at;
    };
    L.main_desc = take(main.items.size() * desc_doubles);
    L.red_desc = take(red.items.size() * desc_doubles);
    L.main_table = take((main.first_block.size() + 1) / 2);
    L.red_table = take((red.first_block.size() + 1) / 2);
    for (int64_t i = 0; i < count; ++i)
        if (const size_t c = rows_doubles(jobs[first + i])) L.at[(size_t)i].rows = take(c);
    for (int64_t i = 0; i < count; ++i)
        if (const size_t c = upload_doubles(jobs[first + i])) L.at[(size_t)i].X = take(c);
    L.up_cnt = o;
    for (int64_t i = 0; i < count; ++i)
        if (const size_t c = part_doubles(jobs[first + i])) L.at[(size_t)i].part = take(c);
    L.out0 = o;
    for (int64_t i = 0; i < count; ++i)
        if (const size_t c = out_doubles(jobs[first + i])) L.at[(size_t)i].out = take(c);
    L.out_cnt = o - L.out0;
    L.total = o;
    return L;
}

}  // namespace hessbatch
}  // namespace mrbf
