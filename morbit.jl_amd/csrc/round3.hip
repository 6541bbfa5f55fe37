// Round 3 of the training-site selection for a batch of starts (include/mrbf.h "Round 3 of the training-site selection"): _rbf_round3
// (src/models/RbfModel.jl:269-307), the rebuild along the coordinate axes it falls back to (:286-289 -> :633-637) and the improvement
// step (:699-732), written straight into the resident databases of db.hip.  The host mirror (morbit.jl_amd/sampling.py: _rbf_round3 on
// descent.intersect_box) is the specification; everything that must round like it runs without FMA contraction.
//
// The chain, at most four launches:
//   r3_dir_kernel     a wave per (direction, start), lanes striding over the coordinates (two per lane and load where d is even).
//                     Pass 1 reduces sigma+ (minimum of the candidates >= 0) and sigma- (maximum of the others, NaN included) of
//                     intersect_box over the wave; pass 2 forms offset = len * dir, its inf-norm and the point x + offset, and writes the
//                     row at position n_sites + i of the database and of the staging block, its fail flag and the NaN values row
//   r3_decide_kernel  a workgroup per start: any fail -> status, n_new, fully_linear
//   the same two again along the axes, launched only when some job may rebuild: every workgroup reads its start's status and returns
//   at once unless it asks for the rebuild; they overwrite the same rows.
// Min and max are order-free, so no result depends on the shape of a reduction; no atomics.
#include "round3_host.hpp"
#include "select_call.hpp"  // chain::SelectCall: the host scaffold of a batched call

namespace mrbf {
namespace round3 {

static_assert(sizeof(mrbf_round3_job) == 112, "the job struct of include/mrbf.h");
constexpr int NT = 256;  // four waves: four directions of one start

struct Desc {
    double *S, *V;       // the database's rows behind its last one: sites (d) and values (k)
    const double *xlu;   // x | lb | ub
    const double *dirs;  // d x ncols column-major; NULL: the coordinate axes
    double *stage;       // the start's rows of the staging block
    int *fail;           // per row
    int *out;            // status, n_new, fully_linear, 0
    double pivot;
    int k, n1, n2, ncols, n_dirs, reversed, n_missing, improve, can_rebuild, vec;
};

// the maximum as Julia's and NumPy's: a NaN wins
__device__ __forceinline__ double nan_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

struct Sigma {
    double pos = INFINITY, neg = -INFINITY;  // identities: entries are filed by sign, the flags tell an empty set
    int anyp = 0, anyn = 0, nz = 0;
};
// the entries of _intersect_bound_vec (utilities.jl:126-152) one coordinate contributes: the steps to lb and to ub along dv
__device__ __forceinline__ void take(Sigma &s, double xv, double dv, double l, double u) {
#pragma clang fp contract(off)
    if (dv == 0.0) return;  // (a NaN component is not zero: its entries are NaN and land in sigma-)
    s.nz = 1;
    const double tl = l - xv, tu = u - xv;
    const double cl = tl == 0.0 ? (dv > 0.0 ? INFINITY : 0.0) : tl / dv;
    const double cu = tu == 0.0 ? (dv < 0.0 ? INFINITY : 0.0) : tu / dv;
    if (cl >= 0.0) s.pos = cl < s.pos ? cl : s.pos, s.anyp = 1;
    else s.neg = nan_max(s.neg, cl), s.anyn = 1;
    if (cu >= 0.0) s.pos = cu < s.pos ? cu : s.pos, s.anyp = 1;
    else s.neg = nan_max(s.neg, cu), s.anyn = 1;
}

__global__ __launch_bounds__(NT) void r3_dir_kernel(const Desc *desc, int d, int rebuild) {
#pragma clang fp contract(off)
    const Desc J = desc[blockIdx.y];
    if (rebuild && J.out[0] != MRBF_R3_REBUILT) return;
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);  // the same in every lane of the wave
    if (i >= (rebuild ? J.n2 : J.n1)) return;
    const bool axes = rebuild || J.dirs == nullptr;
    const double *x = J.xlu, *lb = x + d, *ub = lb + d;
    const double *col = axes ? nullptr : J.dirs + (size_t)(J.reversed ? J.ncols - 1 - i : i) * d;
    const bool vec = J.vec != 0 && (d & 1) == 0;
    auto dir_at = [&](int j) { return axes ? (j == i ? 1.0 : 0.0) : col[j]; };
    // ---- pass 1: len = intersect_box(x, dir, lb, ub; :absmax)
    Sigma s;
    if (vec) {
        const double2 *x2 = reinterpret_cast<const double2 *>(x), *l2 = reinterpret_cast<const double2 *>(lb),
                      *u2 = reinterpret_cast<const double2 *>(ub), *c2 = reinterpret_cast<const double2 *>(col);
        for (int j = lane; j < d / 2; j += 64) {
            const double2 xv = x2[j], l = l2[j], u = u2[j];
            const double2 dv = axes ? make_double2(dir_at(2 * j), dir_at(2 * j + 1)) : c2[j];
            take(s, xv.x, dv.x, l.x, u.x);
            take(s, xv.y, dv.y, l.y, u.y);
        }
    } else {
        for (int j = lane; j < d; j += 64) take(s, x[j], dir_at(j), lb[j], ub[j]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double p2 = __shfl_xor(s.pos, o, 64), n2 = __shfl_xor(s.neg, o, 64);
        s.pos = p2 < s.pos ? p2 : s.pos;
        s.neg = nan_max(s.neg, n2);
        s.anyp |= __shfl_xor(s.anyp, o, 64), s.anyn |= __shfl_xor(s.anyn, o, 64), s.nz |= __shfl_xor(s.nz, o, 64);
    }
    const double sp = s.anyp ? s.pos : 0.0, sn = s.anyn ? s.neg : 0.0;
    const double len = !s.nz ? INFINITY : (fabs(sp) >= fabs(sn) ? sp : sn);
    // ---- pass 2: offset = len .* dir, norm(offset, Inf), x .+ offset
    double *row = J.S + (size_t)i * d, *st = J.stage + (size_t)i * d;
    double nrm = 0.0;
    if (vec) {
        const double2 *x2 = reinterpret_cast<const double2 *>(x), *c2 = reinterpret_cast<const double2 *>(col);
        double2 *row2 = reinterpret_cast<double2 *>(row), *st2 = reinterpret_cast<double2 *>(st);
        for (int j = lane; j < d / 2; j += 64) {
            const double2 xv = x2[j];
            const double2 dv = axes ? make_double2(dir_at(2 * j), dir_at(2 * j + 1)) : c2[j];
            const double ox = len * dv.x, oy = len * dv.y;
            nrm = nan_max(nan_max(nrm, fabs(ox)), fabs(oy));
            const double2 pt = make_double2(xv.x + ox, xv.y + oy);
            row2[j] = pt, st2[j] = pt;
        }
    } else {
        for (int j = lane; j < d; j += 64) {
            const double o = len * dir_at(j);
            nrm = nan_max(nrm, fabs(o));
            const double pt = x[j] + o;
            row[j] = pt, st[j] = pt;
        }
    }
    for (int o = 32; o > 0; o >>= 1) nrm = nan_max(nrm, __shfl_xor(nrm, o, 64));
    // (RbfModel.jl:284: fails iff norm <= pivot; :718: the improvement step keeps the point iff norm > pivot)
    if (lane == 0) J.fail[i] = J.improve ? !(nrm > J.pivot) : (nrm <= J.pivot);
    double *vrow = J.V + (size_t)i * J.k;
    for (int j = lane; j < J.k; j += 64) vrow[j] = __longlong_as_double(0x7ff8000000000000ll);  // new_result!(db, p, F[])
}

__global__ __launch_bounds__(NT) void r3_decide_kernel(const Desc *desc, int d, int rebuild) {
    const Desc J = desc[blockIdx.x];
    if (rebuild && J.out[0] != MRBF_R3_REBUILT) return;  // (uniform over the workgroup)
    const int cnt = rebuild ? J.n2 : J.n1;
    int mine = 0;
    for (int i = threadIdx.x; i < cnt; i += NT) mine |= J.fail[i];
    const int any = __syncthreads_or(mine);
    if (threadIdx.x != 0) return;
    int status = MRBF_R3_DONE, n_new = cnt, fl;
    if (rebuild) {
        status = MRBF_R3_REBUILT;
        fl = cnt >= d && !any;
    } else if (J.improve) {
        n_new = (cnt == 1 && !any) ? 1 : 0;
        fl = n_new == 1 && J.n_dirs == 1;
    } else if (any && J.can_rebuild) {
        status = MRBF_R3_REBUILT, n_new = J.n2, fl = 0;  // decided by the second pair of launches
    } else {
        fl = cnt >= J.n_missing && !any;
    }
    J.out[0] = status, J.out[1] = n_new, J.out[2] = fl, J.out[3] = 0;
}

}  // namespace round3
}  // namespace mrbf

using namespace mrbf;

extern "C" int32_t mrbf_db_round3_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, mrbf_round3_job *jobs, float *ms_total) {
    using namespace round3;
    std::vector<DbInfo> info;
    MRBF_TRY(db::open_batch(ctx, "mrbf_db_round3_batch", n_starts, d, jobs, 4, info, [&] { return check_jobs(n_starts, d, jobs, info.data(), 4); }));
    const size_t N = (size_t)n_starts, D = (size_t)d;
    std::vector<int64_t> rows(N), caps(N);
    for (size_t p = 0; p < N; ++p) rows[p] = info[p].n, caps[p] = jobs[p].db->cap;
    chain::SelectCall call(ctx, ms_total);
    std::vector<char> host_flag(N);
    bool *on_host = reinterpret_cast<bool *>(host_flag.data());
    for (size_t p = 0; p < N; ++p) on_host[p] = jobs[p].dirs != nullptr && !is_device_ptr(jobs[p].dirs);
    const Layout L = layout(n_starts, d, jobs, rows.data(), caps.data(), on_host, sizeof(Desc));
    // ---- the reservation: room for the larger of the first attempt and the rebuild; the kernels write only inside it
    for (size_t p = 0; p < N; ++p)
        if (L.cnt[p].rows() > 0) MRBF_TRY(db_reserve(ctx, jobs[p].db, L.reserve[p]));
    // ---- one upload: descriptors, x | lb | ub, the host-side direction blocks
    MRBF_TRY(call.open(S_DB_WS, L.A, L.oDirs));
    Desc *hdesc = call.host<Desc>(L.oDesc);
    bool any_rebuild = false;
    for (size_t p = 0; p < N; ++p) {
        const mrbf_round3_job &jb = jobs[p];
        const Counts &c = L.cnt[p];
        Desc &h = hdesc[p];
        h.S = jb.db->sites + (size_t)rows[p] * D, h.V = jb.db->values + (size_t)rows[p] * (size_t)info[p].k;
        h.xlu = call.dev<const double>(L.oXlu) + p * 3 * D, h.stage = call.dev<double>(L.oStage) + (size_t)L.roff[p] * D;
        h.fail = call.dev<int>(L.oFail) + L.roff[p], h.out = call.dev<int>(L.oOut) + 4 * p;
        h.pivot = jb.pivot_val;
        h.k = info[p].k, h.n1 = c.n1, h.n2 = c.n2, h.n_dirs = c.n_dirs, h.reversed = jb.reversed != 0, h.n_missing = jb.n_missing;
        h.improve = jb.mode == MRBF_R3_IMPROVE, h.can_rebuild = c.can_rebuild;
        double *b = call.host<double>(L.oXlu) + p * 3 * D;
        std::memcpy(b, jb.x, D * sizeof(double)), std::memcpy(b + D, jb.lb, D * sizeof(double)), std::memcpy(b + 2 * D, jb.ub, D * sizeof(double));
        if (c.rc == 0 && jb.dirs && c.n1 > 0) {
            if (on_host[p]) {  // the n1 columns the first attempt reads
                std::memcpy(call.host<double>(L.oDirs) + L.doff[p], jb.dirs + (size_t)L.first_col(p, h.reversed) * D, (size_t)c.n1 * D * sizeof(double));
                h.dirs = call.dev<const double>(L.oDirs) + L.doff[p], h.ncols = c.n1;
            } else {
                h.dirs = jb.dirs, h.ncols = c.n_dirs;
            }
        }
        h.vec = (d & 1) == 0 && (reinterpret_cast<uintptr_t>(h.dirs) & 15) == 0;
        any_rebuild = any_rebuild || (c.rc == 0 && c.can_rebuild);
    }
    MRBF_TRY(call.begin());
    MRBF_TRY(call.upload());
    const Desc *ddesc = call.dev<const Desc>(L.oDesc);
    for (int pass = 0; pass < (any_rebuild ? 2 : 1); ++pass) {
        const int rmax = pass ? L.rows_max2 : L.rows_max1;
        if (rmax > 0) hipLaunchKernelGGL(r3_dir_kernel, dim3((unsigned)((rmax + 3) / 4), (unsigned)N), dim3(NT), 0, call.s, ddesc, d, pass);
        hipLaunchKernelGGL(r3_decide_kernel, dim3((unsigned)N), dim3(NT), 0, call.s, ddesc, d, pass);
    }
    // ---- one read-back: status, n_new, fully_linear per start, and the staging rows
    MRBF_TRY(call.finish(L.A.back_bytes()));
    const int *out = reinterpret_cast<const int *>(call.back.p);
    const double *stage = reinterpret_cast<const double *>(call.back.p + (L.oStage - L.oOut));
    for (size_t p = 0; p < N; ++p) {
        mrbf_round3_job &jb = jobs[p];
        const Counts &c = L.cnt[p];
        if (c.rc != 0) {
            jb.rc = c.rc;
            continue;
        }
        const int status = out[4 * p], n_new = out[4 * p + 1];
        if ((status != MRBF_R3_DONE && status != MRBF_R3_REBUILT) || n_new < 0 || n_new > c.rows()) {  // (cannot happen: the kernels' own counts)
            jb.rc = MRBF_EHIP;
            continue;
        }
        if (jb.new_sites_out && n_new > 0) std::memcpy(jb.new_sites_out, stage + (size_t)L.roff[p] * D, (size_t)n_new * D * sizeof(double));
        jb.first_index = jb.db->n;
        jb.db->n += n_new;  // rows of a discarded attempt lie beyond the count
        jb.n_new = n_new, jb.fully_linear = out[4 * p + 2], jb.status = status;
        jb.n_dirs_used = jb.mode == MRBF_R3_IMPROVE ? std::min(c.n_dirs, 1) : (status == MRBF_R3_REBUILT ? c.n2 : c.n1);
        jb.rc = 0;
    }
    return MRBF_OK;
}
