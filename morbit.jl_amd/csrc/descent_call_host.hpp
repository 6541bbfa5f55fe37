// Host arithmetic that the direction calls share (sd_lp.hip, normal_lp.hip, ds_qp.hip, sd_step.hip), free of HIP so that
// tools/descent_call_host_check.cpp drives it on the CPU under the sanitizers: the rule that cuts a batch into launches, the staging
// layout of a *_direction entry's outputs, and the offsets of a single-start call's packed input block.  DESIGN.md section 8a.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mrbf {
namespace dcall {

constexpr size_t WS_LIMIT_BYTES = (size_t)256 << 20;
// problems per launch: all of them, unless their workspaces would pass `limit` bytes; at least one
inline int64_t chunk(int64_t n_problems, size_t bytes_per_problem, size_t limit = WS_LIMIT_BYTES) {
    const int64_t fit = (int64_t)(limit / (bytes_per_problem ? bytes_per_problem : 1));
    return fit < 1 || n_problems < 1 ? 1 : (n_problems < fit ? n_problems : fit);
}

// ---- outputs: one that the caller keeps in device memory is written in place, every other into one staging buffer and copied back
// before the call's one synchronisation.  The buffer holds the doubles of every output of the call in list order, then the int words
// likewise: a piece has its place whatever the output's residency, and whether or not an optional output was given.
constexpr size_t NONE = ~(size_t)0;
struct Out {
    void *user;  // the caller's buffer; NULL: an optional output that was not given
    size_t count;
    bool is_int, device = false;  // int32 words, else doubles; `user` is device memory
    size_t at = NONE;             // out_layout: byte offset of the staged piece; NONE: in place, or not given
};
// fills in Out::at; returns the doubles of the staging buffer
inline size_t out_layout(Out *o, size_t n) {
    size_t n_dbl = 0, n_int = 0;
    for (size_t i = 0; i < n; ++i) (o[i].is_int ? n_int : n_dbl) += o[i].count;
    size_t at_dbl = 0, at_int = n_dbl * sizeof(double);
    for (size_t i = 0; i < n; ++i) {
        size_t &at = o[i].is_int ? at_int : at_dbl;
        o[i].at = o[i].user && !o[i].device ? at : NONE;
        at += o[i].count * (o[i].is_int ? sizeof(int32_t) : sizeof(double));
    }
    return n_dbl + (n_int + 1) / 2 + 1;
}

// ---- the packed input block of a single-start call: add(count) gives a piece's offset in doubles, in the host vector and the device arena alike
struct Pack {
    size_t total = 0;
    size_t add(size_t count) { return (total += count) - count; }
};

}  // namespace dcall
}  // namespace mrbf
