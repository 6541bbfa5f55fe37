// Host logic of mrbf_eval_hessian (hess.hip, api.hip), free of HIP so that tools/hess_host_check.cpp drives it on the CPU under the
// sanitizers: the validation behind the call's return codes, the list of selected outputs, the shape of a launch (coordinate blocks,
// block pairs, output passes), the rule that splits the centre range over workgroups, the rule that cuts a host-side result into
// chunks of whole query points, and the layout of the call's work buffer
//     selected outputs (int32) | partial blocks of the split centre range
// counted in doubles, every piece a multiple of 16.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mrbf {
namespace hess {

constexpr int SB = 64;            // coordinates of a block: 4 MFMA tiles of 16; a workgroup owns one pair of blocks (bi <= bj)
constexpr int NC = 32;            // centres a workgroup takes per round; a split's centre range is a multiple of it
constexpr int MAX_RB = 4;         // outputs that share one pass over the centres (accumulators of one wave: 4 tiles x 4 outputs)
constexpr int64_t TARGET_WGS = 512;  // workgroups a call should have before the centre range stays in one piece: 2 per compute unit
constexpr int MAX_SPLIT = 64;     // most pieces: beyond, a piece's few rounds no longer pay for its partial blocks and their sum
constexpr size_t STAGE_LIMIT_BYTES = (size_t)256 << 20;  // a host-side result beyond this is staged in chunks of whole query points

// what the call knows before anything is launched
struct Call {
    bool has_ctx = false, has_model = false;
    bool foreign = false;  // the model was created through another context
    int64_t m = 0;
    int k = 0;             // the model's outputs
    bool X = false, out = false;  // pointer given
    int32_t n_rows = 0;
    const int32_t *rows = nullptr;
};

// 0, or the call's return code (include/mrbf.h): -1 no context; -2 NULL model; -4 a model of another context (mrbf_eval_batch's code);
// -3 m < 0; -5 n_rows < 0, or n_rows > 0 with NULL rows; -6 a row outside [0, k); then, with m > 0 only, -4 NULL X and -7 NULL hess_out.
// NULL rows with n_rows = 0 selects all k outputs.
inline int validate(const Call &c) {
    if (!c.has_ctx) return -1;
    if (!c.has_model) return -2;
    if (c.foreign) return -4;
    if (c.m < 0) return -3;
    if (c.n_rows < 0 || (c.n_rows > 0 && !c.rows)) return -5;
    for (int32_t i = 0; i < c.n_rows; ++i)
        if (c.rows[i] < 0 || c.rows[i] >= c.k) return -6;
    if (c.m > 0 && !c.X) return -4;
    if (c.m > 0 && !c.out) return -7;
    return 0;
}

// the selected outputs of a validated call, in the caller's order, repeats kept
inline std::vector<int32_t> row_list(const Call &c) {
    std::vector<int32_t> r;
    if (c.n_rows == 0)
        for (int32_t l = 0; l < c.k; ++l) r.push_back(l);
    else
        r.assign(c.rows, c.rows + c.n_rows);
    return r;
}

inline size_t pad16(size_t cnt) { return (cnt + 15) & ~(size_t)15; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the shape of a launch: r outputs go in passes of rb(r); d coordinates in nblocks(d) blocks, the upper triangle in npairs(d)
inline int rb(int r) { return r >= 3 ? MAX_RB : r; }
inline int npass(int r) { return (int)ceil_div(r, rb(r)); }
inline int nblocks(int d) { return (int)ceil_div(d, SB); }
inline int64_t npairs(int d) { return (int64_t)nblocks(d) * (nblocks(d) + 1) / 2; }

// The split rule: a function of (m, n, d, r) alone.  A call of m queries has m * npairs(d) * npass(r) workgroups per piece of the
// centre range; below TARGET_WGS the range is cut into as many pieces as bring the call there -- at most MAX_SPLIT --, each a multiple
// of NC centres and none empty.  *per: the centres of a piece.
inline int nsplit(int64_t m, int64_t n, int d, int r, int64_t *per = nullptr) {
    const int64_t wgs = m * npairs(d) * npass(r);
    int64_t want = (wgs <= 0 || wgs >= TARGET_WGS) ? 1 : ceil_div(TARGET_WGS, wgs);
    const int64_t most = ceil_div(n, NC);
    if (want > most) want = most;
    if (want > MAX_SPLIT) want = MAX_SPLIT;
    if (want < 1) want = 1;
    const int64_t len = ceil_div(ceil_div(n, want), NC) * NC;
    if (per) *per = len;
    return (int)ceil_div(n, len);
}

// Chunks of whole query points (first, count) that cover 0 .. m - 1 in order, each within limit_bytes of the staged result; one point
// beyond the limit is a chunk of its own.  limit_bytes is an argument so that a test can cut a small call; <= 0 is STAGE_LIMIT_BYTES.
inline std::vector<std::pair<int64_t, int64_t>> chunks(int64_t m, size_t point_bytes, int64_t limit_bytes = 0) {
    std::vector<std::pair<int64_t, int64_t>> out;
    const size_t limit = limit_bytes > 0 ? (size_t)limit_bytes : STAGE_LIMIT_BYTES;
    int64_t per = point_bytes == 0 ? m : (int64_t)(limit / point_bytes);
    if (per < 1) per = 1;
    for (int64_t first = 0; first < m; first += per) out.push_back({first, first + per <= m ? per : m - first});
    return out;
}

// the doubles of partial blocks a launch of `points` queries writes (0: the centre range is in one piece)
inline size_t partial_doubles(int64_t points, int d, int r, int ns) {
    return ns <= 1 ? 0 : (size_t)points * (size_t)npass(r) * (size_t)npairs(d) * (size_t)ns * (size_t)rb(r) * SB * SB;
}

// the call's work buffer (offsets in doubles)
struct Layout {
    size_t rows = 0;  // r int32
    size_t part = 0;  // partial blocks
    size_t total = 0;
};
inline Layout layout(int64_t points, int d, int r, int ns) {
    Layout L;
    L.rows = 0;
    L.part = pad16(((size_t)r + 1) / 2);
    L.total = L.part + pad16(partial_doubles(points, d, r, ns));
    return L;
}

}  // namespace hess
}  // namespace mrbf
