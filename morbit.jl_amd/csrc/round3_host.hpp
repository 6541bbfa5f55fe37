// Host logic of round 3 for a batch of starts (round3.hip; include/mrbf.h "Round 3 of the training-site selection"): how many rows
// a start's first attempt and its rebuild write, the validation of a batch's jobs with the ABI's return codes, and the one function
// that decides the reservation of every database and where every row, flag and descriptor of the batch lives.  Host code without a HIP
// include and without a context, so that tools/round3_host_check.cpp can drive it as a plain C++ program (the pattern of db_host.hpp).
#pragma once
#include "db_host.hpp"

namespace mrbf {
namespace round3 {

using namespace db;  // DbInfo, Defect, defect, check_dbs, grow_capacity

// ---- one start's row counts (RbfModel.jl:274, :634-637, :699-732)
struct Counts {
    int rc = 0;        // 0, or JOB_RC_DIRS: the job takes no part
    int n_dirs = 0;    // of the list the first attempt reads (d for the axes)
    int n1 = 0;        // rows of the first attempt
    int n2 = 0;        // rows of the rebuild along the axes (0 when the start cannot rebuild)
    bool can_rebuild = false;
    int rows() const { return rc != 0 ? 0 : std::max(n1, n2); }  // rows the kernels may write behind the database's last row
};
constexpr int JOB_RC_DIRS = -3;  // n_dirs < n_new: the reference's @assert (RbfModel.jl:278)
inline Counts counts_of(const mrbf_round3_job &jb, int d) {
    Counts c;
    c.n_dirs = jb.dirs ? jb.n_dirs : d;
    if (jb.mode == MRBF_R3_IMPROVE) {
        c.n1 = c.n_dirs >= 1 ? 1 : 0;  // popfirst! of an empty list: the reference warns and does nothing
        return c;
    }
    c.n1 = std::max(0, std::min(jb.n_missing, jb.max_new));
    if (c.n_dirs < c.n1) {
        c.rc = JOB_RC_DIRS, c.n1 = 0;
        return c;
    }
    c.can_rebuild = jb.ensure_fully_linear != 0 && jb.force_rebuild == 0;
    c.n2 = c.can_rebuild ? std::max(0, std::min(d, jb.max_new)) : 0;
    return c;
}

// mrbf_db_round3_batch: `jobs` is argument `arg` (4)
inline Defect check_jobs(int64_t n_starts, int d, const mrbf_round3_job *jobs, const DbInfo *info, int arg) {
    if (Defect D = db::check_dbs(n_starts, d, info, arg)) return D;
    for (int64_t p = 0; p < n_starts; ++p) {
        const mrbf_round3_job &jb = jobs[p];
        if (!jb.x || !jb.lb || !jb.ub) return defect(-arg, "x, lb or ub is NULL", p);
        if (jb.n_dirs < 0) return defect(-arg, "n_dirs is negative", p);
        if (jb.mode != MRBF_R3_UPDATE && jb.mode != MRBF_R3_IMPROVE) return defect(-arg, "mode is neither MRBF_R3_UPDATE nor MRBF_R3_IMPROVE", p);
        if (info[p].n + counts_of(jb, d).rows() > ((int64_t)1 << 31) - db::ROWS) return defect(-arg, "the database would outgrow its row limit", p);
    }
    return Defect();
}

// ---- reservation and layout.  Start p may write the rows n_p .. n_p + rows_p - 1 of its database (reserve[p] = n_p + rows_p rows must
// fit; capacity[p] is what the growth rule makes of the present capacity) and owns the rows roff[p] .. roff[p] + rows_p - 1 of the
// staging block and of the fail flags; the columns of a host-side `dirs` that its first attempt reads (n1 of them: the first, or with
// `reversed` the last) are uploaded at doff[p] doubles of the direction block.  Work buffer (bytes, every piece a multiple of 256):
//   upload = descriptors | x, lb, ub (3 d doubles per start) | direction block;
//   read-back = status, n_new, fully_linear, 0 (4 ints per start) | staging rows (d doubles per row);
//   scratch = fail flags (an int per row).
struct Layout {
    std::vector<Counts> cnt;              // n_starts
    std::vector<int64_t> reserve, capacity;  // n_starts
    std::vector<int64_t> roff, doff;      // n_starts + 1
    int rows_max1 = 0, rows_max2 = 0;     // grid of the first attempt / of the rebuild
    ByteArena A;                          // its marks bound the upload and the read-back
    size_t oDesc = 0, oXlu = 0, oDirs = 0, oOut = 0, oStage = 0, oFail = 0;
    // first uploaded column of start p's `dirs` (the kernels index the uploaded block from 0)
    int first_col(size_t p, int reversed) const { return reversed ? cnt[p].n_dirs - cnt[p].n1 : 0; }
};
inline Layout layout(int64_t n_starts, int d, const mrbf_round3_job *jobs, const int64_t *n_sites, const int64_t *cap, const bool *dirs_on_host,
                     size_t desc_bytes) {
    Layout L;
    const size_t N = (size_t)n_starts, D = (size_t)d;
    L.cnt.resize(N), L.reserve.resize(N), L.capacity.resize(N);
    L.roff.assign(N + 1, 0), L.doff.assign(N + 1, 0);
    for (size_t p = 0; p < N; ++p) {
        const Counts c = counts_of(jobs[p], d);
        L.cnt[p] = c;
        L.reserve[p] = n_sites[p] + c.rows();
        L.capacity[p] = db::grow_capacity(cap[p], L.reserve[p]);
        L.roff[p + 1] = L.roff[p] + c.rows();
        const int64_t up = (c.rc == 0 && jobs[p].dirs && dirs_on_host[p]) ? (int64_t)c.n1 * d : 0;
        L.doff[p + 1] = L.doff[p] + (up + 1) / 2 * 2;  // (16-byte pieces)
        if (c.rc == 0) L.rows_max1 = std::max(L.rows_max1, c.n1), L.rows_max2 = std::max(L.rows_max2, c.n2);
    }
    L.oDesc = L.A.take(N * desc_bytes), L.oXlu = L.A.take(N * 3 * D * sizeof(double)), L.oDirs = L.A.take((size_t)L.doff[N] * sizeof(double));
    L.oOut = L.A.take(N * 4 * sizeof(int)), L.oStage = L.A.take((size_t)L.roff[N] * D * sizeof(double));
    L.oFail = L.A.take((size_t)L.roff[N] * sizeof(int));
    L.A.up_end = L.A.back_at = L.oOut, L.A.back_end = L.oFail;
    return L;
}

}  // namespace round3
}  // namespace mrbf
