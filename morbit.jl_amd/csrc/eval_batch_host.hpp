// Host logic of mrbf_eval_batch (eval_batch.hip), free of HIP so that tools/eval_batch_host_check.cpp drives it on the CPU under the
// sanitizers: what the call is told of a job, the validation behind its return codes, which jobs do any work, the rule that cuts a
// batch into chunks of consecutive jobs, and the layout of a chunk's arena
//     descriptors | host-side query rows        one upload
//     evaluation scratch                        (batch_chain.hpp: Plan::carve)
//     host-side values | host-side Jacobians    one read-back
// counted in doubles, every piece a multiple of 16.  Buffers the caller keeps on the device have no place in the arena: the
// descriptors carry their addresses.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mrbf {
namespace evalbatch {

constexpr size_t ARENA_LIMIT_BYTES = (size_t)2 << 30;  // a call whose arena would exceed this is processed in chunks of jobs
constexpr size_t NONE = ~(size_t)0;

// what the call knows of a job before anything is launched
struct Job {
    bool has_model = false;  // jobs[i].model != NULL
    bool foreign = false;    // the model was created through another context (and so, possibly, on another device)
    int64_t m = 0;
    int d = 0, k = 0;        // the model's
    bool X = false, vals = false, jac = false;              // pointer given
    bool X_dev = false, vals_dev = false, jac_dev = false;  // ... and device memory
};

inline size_t pad16(size_t cnt) { return (cnt + 15) & ~(size_t)15; }

// 0, or the call's return code with the first offending job in *which: -3 (NULL model, m < 0, NULL X with m > 0), -4 (a model of
// another context).  All jobs are looked at before anything is launched or written.
inline int validate(const Job *jobs, int64_t n_jobs, int64_t *which) {
    for (int64_t i = 0; i < n_jobs; ++i) {
        const Job &J = jobs[i];
        if (!J.has_model || J.m < 0 || (J.m > 0 && !J.X)) {
            if (which) *which = i;
            return -3;
        }
    }
    for (int64_t i = 0; i < n_jobs; ++i)
        if (jobs[i].foreign) {
            if (which) *which = i;
            return -4;
        }
    return 0;
}

// a job that launches something: query rows and at least one output
inline bool active(const Job &J) { return J.m > 0 && (J.vals || J.jac); }

// the doubles of the arena a job's host-side buffers take: its query rows in the upload, its outputs in the read-back block
inline size_t upload_doubles(const Job &J) { return active(J) && !J.X_dev ? pad16((size_t)J.m * J.d) : 0; }
inline size_t vals_doubles(const Job &J) { return active(J) && J.vals && !J.vals_dev ? pad16((size_t)J.m * J.k) : 0; }
inline size_t jac_doubles(const Job &J) { return active(J) && J.jac && !J.jac_dev ? pad16((size_t)J.m * J.k * J.d) : 0; }

// Chunks of consecutive jobs (first, count) that cover 0 .. n_jobs - 1 in order: a chunk is closed in front of the job that would carry
// its arena beyond limit_bytes.  doubles[i]: everything job i adds to an arena (descriptor, host-side buffers, scratch).  A single
// job beyond the limit is a chunk of its own -- the single call would need as much.  limit_bytes is an argument so that a test can
// cut a small batch; the call passes ARENA_LIMIT_BYTES.
inline std::vector<std::pair<int64_t, int64_t>> chunks(const std::vector<size_t> &doubles, size_t limit_bytes = ARENA_LIMIT_BYTES) {
    std::vector<std::pair<int64_t, int64_t>> out;
    const size_t limit = limit_bytes / sizeof(double);
    int64_t first = 0;
    size_t sum = 0;
    for (int64_t i = 0; i < (int64_t)doubles.size(); ++i) {
        if (i > first && sum + doubles[(size_t)i] > limit) {
            out.push_back({first, i - first});
            first = i, sum = 0;
        }
        sum += doubles[(size_t)i];
    }
    if ((int64_t)doubles.size() > first) out.push_back({first, (int64_t)doubles.size() - first});
    return out;
}

// where a job's host-side buffers live in the chunk's arena (offsets in doubles; NONE: in place on the device, or not asked for)
struct Place {
    size_t X = NONE, vals = NONE, jac = NONE;
};
struct Layout {
    size_t desc = 0;     // the descriptor array
    size_t up_cnt = 0;   // the upload: [0, up_cnt)
    size_t scratch = 0;  // the evaluation scratch: [scratch, out0)
    size_t out0 = 0, out_cnt = 0;  // the read-back block: [out0, out0 + out_cnt)
    size_t total = 0;
    std::vector<Place> at;  // per job of the chunk
};

inline Layout layout(const Job *jobs, int64_t first, int64_t count, size_t desc_doubles, size_t scratch_doubles) {
    Layout L;
    L.at.resize((size_t)count);
    size_t o = 0;
    auto take = [&](size_t cnt) {
        const size_t at = o;
        o += pad16(cnt);
        return at;
    };
    L.desc = take(desc_doubles);
    for (int64_t i = 0; i < count; ++i)
        if (const size_t c = upload_doubles(jobs[first + i])) L.at[(size_t)i].X = take(c);
    L.up_cnt = o;
    L.scratch = take(scratch_doubles);
    L.out0 = o;
    for (int64_t i = 0; i < count; ++i) {
        if (const size_t c = vals_doubles(jobs[first + i])) L.at[(size_t)i].vals = take(c);
        if (const size_t c = jac_doubles(jobs[first + i])) L.at[(size_t)i].jac = take(c);
    }
    L.out_cnt = o - L.out0;
    L.total = o;
    return L;
}

}  // namespace evalbatch
}  // namespace mrbf
