// Host logic of the resident site database (db.hip; include/mrbf.h "resident site database"): the capacity rule, the exclusion-mask
// builder, the validation of a batch's jobs with the ABI's return codes and the layout of a batch's views, upload, read-back and
// scratch.  Host code without a HIP include and without a context, so that tools/db_host_check.cpp can drive it as a plain C++
// program (the pattern of descent_problem.hpp): the caller describes the databases (d, k, rows), a defect comes back by value.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mrbf.h"
#include "select_host.hpp"

namespace mrbf {
namespace db {

constexpr int ROWS = 64;  // B: database rows per workgroup of the flag and compaction kernels (four waves, sixteen rows each)
constexpr int64_t MIN_CAPACITY = 64;

// ---- the capacity rule: rows allocated once `needed` rows must fit into an allocation of `cap` rows.  Unchanged while they fit;
// else twice the capacity, at least what is needed, at least MIN_CAPACITY: m appends of one row copy O(m) rows in all
inline int64_t grow_capacity(int64_t cap, int64_t needed) {
    if (needed <= cap) return cap;
    return std::max(std::max(2 * cap, needed), MIN_CAPACITY);
}

// ---- the exclusion mask of one start: mask[i] = 1 iff i is in `exclude`, i in [0, n_sites); duplicates allowed, entries outside the
// range ignored.  Built on the host and uploaded with the descriptors (one byte per row: no memset, no scatter launch)
inline void build_mask(int64_t n_sites, int64_t n_exclude, const int64_t *exclude, unsigned char *mask) {
    std::memset(mask, 0, (size_t)n_sites);
    for (int64_t e = 0; e < n_exclude; ++e)
        if (exclude[e] >= 0 && exclude[e] < n_sites) mask[exclude[e]] = 1;
}

// ---- what the validation is told of a job's database
struct DbInfo {
    const void *id;  // the handle (NULL: the job has none)
    int d, k;
    int64_t n;       // rows
    bool own;        // created through the context of the call
};
DbInfo info_of(const mrbf_ctx *ctx, const mrbf_db *db);  // (db.hip) of a handle, NULL included
using mrbf::Defect;
inline Defect defect(int code, const char *what, int64_t p) {
    char buf[160];
    std::snprintf(buf, sizeof(buf), "jobs[%lld]: %s", (long long)p, what);
    Defect D;
    D.code = code, D.msg = buf;
    return D;
}
// a database may appear at most once per batch call
inline int64_t first_repeated(int64_t n_starts, const DbInfo *info) {
    std::vector<std::pair<const void *, int64_t>> ids((size_t)n_starts);
    for (int64_t p = 0; p < n_starts; ++p) ids[(size_t)p] = {info[p].id, p};
    std::sort(ids.begin(), ids.end());
    int64_t hit = -1;
    for (size_t i = 1; i < ids.size(); ++i)
        if (ids[i].first == ids[i - 1].first && (hit < 0 || ids[i].second < hit)) hit = ids[i].second;
    return hit;
}
inline Defect check_dbs(int64_t n_starts, int d, const DbInfo *info, int arg) {
    for (int64_t p = 0; p < n_starts; ++p) {
        if (!info[p].id) return defect(-arg, "db is NULL", p);
        if (!info[p].own) return defect(-arg, "db belongs to another context", p);
        if (d >= 0 && info[p].d != d) return defect(-arg, "db has another d than the call", p);  // (d < 0: the call has no d)
    }
    const int64_t rep = first_repeated(n_starts, info);
    if (rep >= 0) return defect(-arg, "db appears twice in the batch", rep);
    return Defect();
}
// mrbf_db_box_batch: `jobs` is argument `arg` (5)
inline Defect check_box_jobs(int64_t n_starts, int d, const mrbf_db_box_job *jobs, const DbInfo *info, int arg) {
    if (Defect D = check_dbs(n_starts, d, info, arg)) return D;
    for (int64_t p = 0; p < n_starts; ++p) {
        const mrbf_db_box_job &jb = jobs[p];
        if (!jb.lb || !jb.ub || !jb.x0) return defect(-arg, "lb, ub or x0 is NULL", p);
        if (jb.n_exclude < 0 || (jb.n_exclude > 0 && !jb.exclude)) return defect(-arg, "exclude list is NULL or its count negative", p);
        if (!jb.first_row) return defect(-arg, "first_row is NULL", p);
    }
    return Defect();
}
// mrbf_db_gather_batch: `jobs` is argument `arg` (4).  An index out of range is the job's own failure (index_rc), not the call's
inline Defect check_gather_jobs(int64_t n_starts, int d, const mrbf_db_gather_job *jobs, const DbInfo *info, int arg) {
    if (Defect D = check_dbs(n_starts, d, info, arg)) return D;
    for (int64_t p = 0; p < n_starts; ++p) {
        if (jobs[p].n_idx < 0) return defect(-arg, "n_idx is negative", p);
        if (jobs[p].n_idx > 0 && !jobs[p].indices) return defect(-arg, "indices is NULL", p);
    }
    return Defect();
}
constexpr int GATHER_RC_INDEX = -3;  // `indices` is the third field of mrbf_db_gather_job
constexpr int SET_VALUES_RC_INDEX = -4;  // what mrbf_db_set_values returns for an index that is not a row
// a job's own rc: `rc` when one of its m indices is not a row of the database
inline int index_rc(int64_t n_sites, int64_t m, const int64_t *indices, int rc) {
    for (int64_t i = 0; i < m; ++i)
        if (indices[i] < 0 || indices[i] >= n_sites) return rc;
    return 0;
}

// mrbf_db_append_batch / mrbf_db_set_values_batch: `jobs` is argument `arg` (3); the databases of a call may differ in d and k
inline Defect check_append_jobs(int64_t n_starts, const mrbf_db_append_job *jobs, const DbInfo *info, int arg) {
    if (Defect D = check_dbs(n_starts, -1, info, arg)) return D;
    for (int64_t p = 0; p < n_starts; ++p) {
        if (jobs[p].m < 0 || info[p].n + jobs[p].m > ((int64_t)1 << 31) - ROWS) return defect(-arg, "m is negative or beyond the row limit", p);
        if (jobs[p].m > 0 && !jobs[p].sites) return defect(-arg, "sites is NULL", p);
    }
    return Defect();
}
inline Defect check_set_values_jobs(int64_t n_starts, const mrbf_db_set_values_job *jobs, const DbInfo *info, int arg) {
    if (Defect D = check_dbs(n_starts, -1, info, arg)) return D;
    for (int64_t p = 0; p < n_starts; ++p) {
        if (jobs[p].m < 0) return defect(-arg, "m is negative", p);
        if (jobs[p].m > 0 && (!jobs[p].indices || !jobs[p].values)) return defect(-arg, "indices or values is NULL", p);
    }
    return Defect();
}
// (the packed upload of either call is a ByteArena: the descriptors, then the host-side pieces of start after start)

// ---- the layout of a box batch.  Start p owns the rows roff[p] .. roff[p] + n_p - 1 of every per-row array (roff: prefix sums of n_p
// rounded up to ROWS, so a workgroup's rows belong to one start) and the workgroups roff[p] / ROWS ...
//   views (doubles, a buffer of their own): candidate sites of start p at roff[p] * d, shifted rows at (rows + roff[p]) * d --
//     room for every row of the database, as the count is known only after the scan;
//   work buffer (bytes): upload = descriptors | lb, ub, x0 (3 d doubles per start) | masks (a byte per row; the flag kernel turns
//     them into the candidate flags in place); read-back = mc and first pick (2 x int64 per start) | first rows (d doubles per
//     start) | candidate indices (an int64 per row); scratch = row norms | candidate norms (a double per row each) | counts |
//     offsets (an int per workgroup each).  The marks of `A` bound the upload and the whole read-back; its head (without the
//     candidate indices) is back_head_bytes.
struct BoxLayout {
    std::vector<int64_t> roff;  // n_starts + 1
    int64_t rows = 0, nblk_max = 0;
    size_t view_doubles = 0;
    ByteArena A;
    size_t oDesc = 0, oBounds = 0, oMask = 0;
    size_t oHead = 0, oFirst = 0, oIdx = 0, back_head_bytes = 0;
    size_t oNorm = 0, oCnorm = 0, oCount = 0, oOffs = 0;
    size_t sites_view(int64_t p, int d) const { return (size_t)roff[(size_t)p] * (size_t)d; }
    size_t shifted_view(int64_t p, int d) const { return (size_t)(rows + roff[(size_t)p]) * (size_t)d; }
};
inline BoxLayout box_layout(int64_t n_starts, int d, const int64_t *n_sites, size_t desc_bytes) {
    BoxLayout L;
    const size_t N = (size_t)n_starts, D = (size_t)d;
    L.roff.assign(N + 1, 0);
    for (size_t p = 0; p < N; ++p) {
        const int64_t padded = (n_sites[p] + ROWS - 1) / ROWS * ROWS;
        L.roff[p + 1] = L.roff[p] + padded;
        L.nblk_max = std::max(L.nblk_max, padded / ROWS);
    }
    L.rows = L.roff[N];
    const size_t R = (size_t)L.rows, NB = R / ROWS;
    L.view_doubles = 2 * R * D;
    L.oDesc = L.A.take(N * desc_bytes), L.oBounds = L.A.take(N * 3 * D * sizeof(double)), L.oMask = L.A.take(R);
    L.oHead = L.A.take(N * 2 * sizeof(int64_t)), L.oFirst = L.A.take(N * D * sizeof(double));
    L.oIdx = L.A.take(R * sizeof(int64_t));
    L.oNorm = L.A.take(R * sizeof(double)), L.oCnorm = L.A.take(R * sizeof(double));
    L.oCount = L.A.take(NB * sizeof(int)), L.oOffs = L.A.take(NB * sizeof(int));
    L.A.up_end = L.A.back_at = L.oHead, L.A.back_end = L.oNorm, L.back_head_bytes = L.oIdx - L.oHead;
    return L;
}

// ---- the layout of a gather batch: start p's index list at ioff[p] of the uploaded list (prefix sums of the counts of the jobs that
// take part: n_idx[p] < 0 marks a job that failed its own check), its site rows at soff[p] and its value rows at voff[p] of the
// views (doubles, every piece a multiple of 16); the upload (bytes, `A`) = descriptors | index lists
struct GatherLayout {
    std::vector<int64_t> ioff;        // n_starts + 1
    std::vector<size_t> soff, voff;   // n_starts
    int64_t n_idx_max = 0;
    size_t view_doubles = 0;
    ByteArena A;
    size_t oDesc = 0, oIdx = 0;
};
inline GatherLayout gather_layout(int64_t n_starts, int d, const int *k, const int64_t *n_idx, size_t desc_bytes) {
    GatherLayout L;
    const size_t N = (size_t)n_starts;
    L.ioff.assign(N + 1, 0), L.soff.assign(N, 0), L.voff.assign(N, 0);
    auto up16 = [](size_t c) { return (c + 15) & ~(size_t)15; };
    size_t at = 0;
    for (size_t p = 0; p < N; ++p) {
        const int64_t m = std::max<int64_t>(n_idx[p], 0);
        L.ioff[p + 1] = L.ioff[p] + m;
        L.n_idx_max = std::max(L.n_idx_max, m);
        L.soff[p] = at, at += up16((size_t)m * (size_t)d);
        L.voff[p] = at, at += up16((size_t)m * (size_t)k[p]);
    }
    L.view_doubles = at;
    L.oDesc = L.A.take(N * desc_bytes), L.oIdx = L.A.take((size_t)L.ioff[N] * sizeof(int64_t));
    L.A.up_end = L.A.total;
    return L;
}

}  // namespace db
}  // namespace mrbf
