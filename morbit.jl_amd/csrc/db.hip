// The resident site database (include/mrbf.h "resident site database"): a start's sites and values stay on the device and are appended
// to as the run goes; the box scan of results_in_box_indices (src/Databases.jl:324-327) with the filter's shifted rows and first pick
// (AffinelyIndependentPoints.jl:25, :53), and the row gathers of round 4 and the fit (RbfModel.jl:372, :747-757), run for a whole
// batch of starts with the start on a grid dimension, one packed upload and one read-back per call.  Their outputs are device views
// the batched calls (mrbf_affine_select_batch, mrbf_round4_batch, mrbf_fit_batch) take as they take any device pointer.
//
// The box chain, four launches:
//   db_flag_kernel     a workgroup per ROWS database rows, a wave per row at a time, consecutive lanes on consecutive coordinates: the
//                      row is read once, the box test and the p-norm of site - x0 are reduced over it in the same pass; the row's
//                      exclusion byte (built on the host, uploaded with the descriptors) becomes its candidate flag; per-workgroup counts
//   db_scan_kernel     per start: exclusive scan of the workgroup counts, the candidate count to the read-back block
//   db_compact_kernel  index, site row, shifted row and norm of every candidate to its position: ascending database order by the scan
//   db_pick_kernel     per start: first maximiser of the candidates' norms (lowest position wins ties), its shifted row to the read-back
//                      block, then zeroed in the view when asked
// mrbf_db_append_batch and mrbf_db_set_values_batch are mrbf_db_append and mrbf_db_set_values for every start of a batch: the host-side
// rows and index lists of all starts travel in one packed upload behind the descriptors, one launch copies or scatters them.
#include "select_call.hpp"  // chain::SelectCall, the host scaffold of a batched call; db_host.hpp

namespace mrbf {
namespace db {

static_assert(sizeof(mrbf_db_box_job) == 120 && sizeof(mrbf_db_gather_job) == 64, "the job structs of include/mrbf.h");
static_assert(sizeof(mrbf_db_append_job) == 48 && sizeof(mrbf_db_set_values_job) == 40, "the job structs of include/mrbf.h");
constexpr int NT = 256;            // four waves
constexpr int WROWS = ROWS / 4;    // rows of a wave

struct BoxDesc {
    const double *S;       // the database's sites, n x d
    const double *bounds;  // lb | ub | x0
    unsigned char *flag;   // per row: in = excluded, out = candidate
    double *norm, *cnorm;  // per row / per candidate
    int *count, *offs;     // per workgroup
    long long *head;       // mc, first pick
    double *first;         // d: the first pick's shifted row
    long long *idx;        // the candidates' database indices
    double *vs, *vh;       // the views: candidate sites, shifted rows
    long long n;
    int nblk, zero;
};
struct GatherDesc {
    const double *S, *V;
    const long long *idx;
    double *so, *vo;
    long long m;
    int k, pad;
};

// `b` takes the place of `a` as the maximum: strictly greater, or the first NaN (findmax and np.argmax both return the first NaN)
__device__ __forceinline__ bool better(double b, double a) { return b > a || (b != b && a == a); }
__device__ __forceinline__ double norm_max(double a, double b) { return better(b, a) ? b : a; }

__global__ __launch_bounds__(NT) void db_flag_kernel(const BoxDesc *desc, int d, int p_is_inf) {
    const BoxDesc J = desc[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __shared__ int cnt[4];
    const double *lb = J.bounds, *ub = lb + d, *x0 = ub + d;
    int mine = 0;
    for (int r = 0; r < WROWS; ++r) {
        const long long i = (long long)blockIdx.x * ROWS + w * WROWS + r;  // the same in every lane of the wave
        if (i >= J.n) break;
        const double *row = J.S + i * d;
        bool in = true;
        double acc = 0.0;
        auto take = [&](double v, double l, double u, double c) {
            in = in && (l <= v) && (v <= u);  // a NaN coordinate fails both
            const double s = v - c;
            if (p_is_inf) acc = norm_max(acc, fabs(s));
            else acc += s * s;
        };
        if ((d & 1) == 0) {  // rows and bounds are 16-byte aligned: two coordinates per lane and load
            const double2 *row2 = reinterpret_cast<const double2 *>(row), *lb2 = reinterpret_cast<const double2 *>(lb),
                          *ub2 = reinterpret_cast<const double2 *>(ub), *x2 = reinterpret_cast<const double2 *>(x0);
            for (int j = lane; j < d / 2; j += 64) {
                const double2 v = row2[j], l = lb2[j], u = ub2[j], c = x2[j];
                take(v.x, l.x, u.x, c.x);
                take(v.y, l.y, u.y, c.y);
            }
        } else {
            for (int j = lane; j < d; j += 64) take(row[j], lb[j], ub[j], x0[j]);
        }
        for (int s = 32; s > 0; s >>= 1) {
            const double o = __shfl_xor(acc, s, 64);
            acc = p_is_inf ? norm_max(acc, o) : acc + o;
        }
        const bool all_in = __all(in ? 1 : 0) != 0;
        const int excluded = __shfl(lane == 0 ? (int)J.flag[i] : 0, 0, 64);  // read and rewritten by the same lane
        const int cand = (all_in && excluded == 0) ? 1 : 0;
        if (lane == 0) {
            J.flag[i] = (unsigned char)cand;
            J.norm[i] = p_is_inf ? acc : sqrt(acc);
        }
        mine += cand;
    }
    if (lane == 0) cnt[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) J.count[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

__global__ __launch_bounds__(NT) void db_scan_kernel(const BoxDesc *desc) {
    const BoxDesc J = desc[blockIdx.x];
    __shared__ int sh[NT];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < J.nblk; b0 += NT) {
        const int b = b0 + t;
        const int c = b < J.nblk ? J.count[b] : 0;
        sh[t] = c;
        __syncthreads();
        for (int s = 1; s < NT; s <<= 1) {
            const int v = t >= s ? sh[t - s] : 0;
            __syncthreads();
            sh[t] += v;
            __syncthreads();
        }
        const int base = carry, incl = sh[t];
        if (b < J.nblk) J.offs[b] = base + incl - c;
        __syncthreads();
        if (t == NT - 1) carry = base + incl;
        __syncthreads();
    }
    if (t == 0) J.head[0] = carry;
}

__global__ __launch_bounds__(NT) void db_compact_kernel(const BoxDesc *desc, int d) {
    const BoxDesc J = desc[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __shared__ int pos[ROWS];
    if (w == 0) {  // ROWS == 64: one wave places the workgroup's candidates behind the workgroups before it
        const long long i = (long long)blockIdx.x * ROWS + lane;
        const int f = i < J.n ? J.flag[i] : 0;
        const unsigned long long m = __ballot(f);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        pos[lane] = f ? J.offs[blockIdx.x] + before : -1;
    }
    __syncthreads();
    const double *x0 = J.bounds + 2 * (size_t)d;
    for (int r = 0; r < WROWS; ++r) {
        const int rl = w * WROWS + r;
        const int dst = pos[rl];  // the same in every lane of the wave
        if (dst < 0) continue;
        const long long i = (long long)blockIdx.x * ROWS + rl;
        const double *row = J.S + i * d;
        double *os = J.vs + (size_t)dst * d, *oh = J.vh + (size_t)dst * d;
        if (lane == 0) {
            J.idx[dst] = i;
            J.cnorm[dst] = J.norm[i];
        }
        for (int j = lane; j < d; j += 64) {
            const double v = row[j];
            os[j] = v;
            oh[j] = v - x0[j];
        }
    }
}

__global__ __launch_bounds__(NT) void db_pick_kernel(const BoxDesc *desc, int d) {
    const BoxDesc J = desc[blockIdx.x];
    const long long mc = J.head[0];
    __shared__ double sv[NT];
    __shared__ long long si[NT];
    const int t = threadIdx.x;
    double bv = 0.0;
    long long bi = -1;
    for (long long c = t; c < mc; c += NT) {  // ascending: a thread keeps the first of its maximisers
        const double v = J.cnorm[c];
        if (bi < 0 || better(v, bv)) bv = v, bi = c;
    }
    sv[t] = bv, si[t] = bi;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double v2 = sv[t + s];
            const long long i2 = si[t + s];
            const double v1 = sv[t];
            const long long i1 = si[t];
            const bool take2 = i2 >= 0 && (i1 < 0 || better(v2, v1) || (!better(v1, v2) && i2 < i1));
            if (take2) sv[t] = v2, si[t] = i2;
        }
        __syncthreads();
    }
    const long long pick = si[0];
    if (t == 0) J.head[1] = pick;
    if (pick < 0) return;
    double *rowp = J.vh + (size_t)pick * d;
    for (int j = t; j < d; j += NT) {
        J.first[j] = rowp[j];
        if (J.zero) rowp[j] = 0.0;
    }
}

__global__ __launch_bounds__(NT) void db_gather_kernel(const GatherDesc *desc, int d) {
    const GatherDesc J = desc[blockIdx.y];
    const int lane = threadIdx.x & 63;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < J.m; r += (long long)gridDim.x * 4) {
        const long long i = J.idx[r];  // checked against the database's rows on the host
        const double *srow = J.S + i * d, *vrow = J.V + i * J.k;
        double *so = J.so + r * d, *vo = J.vo + r * J.k;
        for (int j = lane; j < d; j += 64) so[j] = srow[j];
        for (int j = lane; j < J.k; j += 64) vo[j] = vrow[j];
    }
}

__global__ void db_fill_nan_kernel(double *p, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = __longlong_as_double(0x7ff8000000000000ll);
}
__global__ void db_set_values_kernel(double *V, const long long *idx, const double *vals, long long m, int k) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m * k) V[idx[t / k] * k + t % k] = vals[t];
}

static int reserve(mrbf_ctx *ctx, mrbf_db *db, int64_t needed) {
    const int64_t cap = grow_capacity(db->cap, needed);
    if (cap == db->cap) return 0;
    double *ns = nullptr, *nv = nullptr;
    MRBF_HIP(ctx, hipMalloc(&ns, (size_t)cap * db->d * sizeof(double)));
    hipError_t e = hipMalloc(&nv, (size_t)cap * db->k * sizeof(double));
    if (e != hipSuccess) {
        (void)hipFree(ns);
        MRBF_HIP(ctx, e);
    }
    hipError_t e1 = hipSuccess, e2 = hipSuccess;
    if (db->n > 0) {  // earlier rows keep their bits
        e1 = hipMemcpyAsync(ns, db->sites, (size_t)db->n * db->d * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        e2 = hipMemcpyAsync(nv, db->values, (size_t)db->n * db->k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
    }
    const hipError_t e3 = hipStreamSynchronize(ctx->stream);  // (also: no launch still reads the old allocation)
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        (void)hipFree(ns);
        (void)hipFree(nv);
        MRBF_HIP(ctx, e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3));
    }
    if (db->sites) (void)hipFree(db->sites);
    if (db->values) (void)hipFree(db->values);
    db->sites = ns, db->values = nv, db->cap = cap;
    return 0;
}

DbInfo info_of(const mrbf_ctx *ctx, const mrbf_db *db) {
    return db ? DbInfo{db, db->d, db->k, db->n, db->ctx == ctx} : DbInfo{nullptr, 0, 0, 0, false};
}

// ---- the batched siblings of mrbf_db_append and mrbf_db_set_values: one workgroup column per start, rows strided over blockIdx.x
struct AppendDesc {
    double *S, *V;            // the database's first new row
    const double *ss, *sv;    // the new rows (device view of the caller's, or the uploaded copy); sv == NULL: NaN
    long long m;
    int d, k;
};
struct SetDesc {
    double *V;
    const long long *idx;
    const double *vals;
    long long m;
    int k, pad;
};
__global__ __launch_bounds__(NT) void db_append_batch_kernel(const AppendDesc *desc) {
    const AppendDesc J = desc[blockIdx.y];
    const long long cs = J.m * J.d, cv = J.m * J.k, step = (long long)gridDim.x * NT;
    for (long long t = (long long)blockIdx.x * NT + threadIdx.x; t < cs; t += step) J.S[t] = J.ss[t];
    for (long long t = (long long)blockIdx.x * NT + threadIdx.x; t < cv; t += step)
        J.V[t] = J.sv ? J.sv[t] : __longlong_as_double(0x7ff8000000000000ll);
}
__global__ __launch_bounds__(NT) void db_set_values_batch_kernel(const SetDesc *desc) {
    const SetDesc J = desc[blockIdx.y];
    const long long cv = J.m * J.k, step = (long long)gridDim.x * NT;
    for (long long t = (long long)blockIdx.x * NT + threadIdx.x; t < cv; t += step) J.V[J.idx[t / J.k] * J.k + t % J.k] = J.vals[t];
}

// a view's `count` doubles to the caller's buffer (host or device), where it gave one
static bool view_out(double *dst, const double *src, size_t count) {
    if (!dst || count == 0 || hipMemcpy(dst, src, count * sizeof(double), hipMemcpyDefault) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
// ---- the one launch of mrbf_db_append_batch / mrbf_db_set_values_batch: at most 1024 workgroups of NT threads per start over cnt_max elements
template <class Desc>
static int launch_update(chain::SelectCall &call, void (*kernel)(const Desc *), size_t N, int64_t cnt_max) {
    MRBF_TRY(call.begin());
    MRBF_TRY(call.upload());
    if (cnt_max > 0) {
        const dim3 grid((unsigned)std::min<int64_t>((cnt_max + NT - 1) / NT, 1024), (unsigned)N);
        hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, call.s, call.dev<const Desc>(0));
    }
    return call.finish(0);
}

}  // namespace db

int db_reserve(mrbf_ctx *ctx, mrbf_db *h, int64_t needed) { return db::reserve(ctx, h, needed); }

}  // namespace mrbf

using namespace mrbf;

extern "C" {

int32_t mrbf_db_create(mrbf_ctx *ctx, int32_t d, int32_t k, int64_t capacity_hint, mrbf_db **out) {
    if (!ctx) return -1;
    if (d < 1 || d > 4096) return fail(ctx, -2, "mrbf_db_create: d = %d", d);
    if (k < 1) return fail(ctx, -3, "mrbf_db_create: k = %d", k);
    if (!out) return fail(ctx, -5, "mrbf_db_create: db is NULL");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    mrbf_db *h = new mrbf_db();
    h->ctx = ctx, h->d = d, h->k = k;
    if (capacity_hint > 0) {
        // (the hint is taken as it is: the growth rule applies from the first row that does not fit)
        hipError_t e = hipMalloc(&h->sites, (size_t)capacity_hint * d * sizeof(double));
        if (e == hipSuccess) e = hipMalloc(&h->values, (size_t)capacity_hint * k * sizeof(double));
        if (e != hipSuccess) {
            if (h->sites) (void)hipFree(h->sites);
            delete h;
            MRBF_HIP(ctx, e);
        }
        h->cap = capacity_hint;
    }
    ++ctx->live_dbs;
    *out = h;
    return MRBF_OK;
}

int32_t mrbf_db_append(mrbf_ctx *ctx, mrbf_db *h, int64_t m, const double *sites, const double *values, int64_t *first_index) {
    if (!ctx) return -1;
    if (!h || h->ctx != ctx) return fail(ctx, -2, "mrbf_db_append: db is NULL or belongs to another context");
    if (m < 0 || h->n + m > ((int64_t)1 << 31) - db::ROWS) return fail(ctx, -3, "mrbf_db_append: m = %lld", (long long)m);
    if (m > 0 && !sites) return fail(ctx, -4, "mrbf_db_append: sites is NULL");
    (void)hipSetDevice(ctx->device);
    if (first_index) *first_index = h->n;
    if (m == 0) return MRBF_OK;
    MRBF_TRY(db::reserve(ctx, h, h->n + m));
    hipStream_t s = ctx->stream;
    const size_t D = (size_t)h->d, K = (size_t)h->k, n = (size_t)h->n, M = (size_t)m;
    MRBF_HIP(ctx, hipMemcpyAsync(h->sites + n * D, sites, M * D * sizeof(double), hipMemcpyDefault, s));
    if (values) {
        MRBF_HIP(ctx, hipMemcpyAsync(h->values + n * K, values, M * K * sizeof(double), hipMemcpyDefault, s));
    } else {  // unevaluated rows
        const long long cnt = (long long)(M * K);
        hipLaunchKernelGGL(db::db_fill_nan_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, h->values + n * K, cnt);
        MRBF_HIP(ctx, hipGetLastError());
    }
    MRBF_HIP(ctx, hipStreamSynchronize(s));  // the caller's buffers are its own again
    h->n += m;
    return MRBF_OK;
}

int32_t mrbf_db_set_values(mrbf_ctx *ctx, mrbf_db *h, int64_t m, const int64_t *indices, const double *values) {
    if (!ctx) return -1;
    if (!h || h->ctx != ctx) return fail(ctx, -2, "mrbf_db_set_values: db is NULL or belongs to another context");
    if (m < 0) return fail(ctx, -3, "mrbf_db_set_values: m = %lld", (long long)m);
    if (m == 0) return MRBF_OK;
    if (!indices) return fail(ctx, -4, "mrbf_db_set_values: indices is NULL");
    if (!values) return fail(ctx, -5, "mrbf_db_set_values: values is NULL");
    for (int64_t i = 0; i < m; ++i)
        if (indices[i] < 0 || indices[i] >= h->n) return fail(ctx, -4, "mrbf_db_set_values: indices[%lld] = %lld is not a row", (long long)i, (long long)indices[i]);
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    const size_t M = (size_t)m, K = (size_t)h->k, bIdx = up256(M * sizeof(int64_t));
    char *base;
    MRBF_TRY(get_buf(ctx, S_DB_WS, bIdx + M * K * sizeof(double), &base));
    MRBF_HIP(ctx, hipMemcpyAsync(base, indices, M * sizeof(int64_t), hipMemcpyHostToDevice, s));
    MRBF_HIP(ctx, hipMemcpyAsync(base + bIdx, values, M * K * sizeof(double), hipMemcpyDefault, s));
    const long long cnt = (long long)(M * K);
    hipLaunchKernelGGL(db::db_set_values_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, h->values,
                       reinterpret_cast<const long long *>(base), reinterpret_cast<const double *>(base + bIdx), (long long)m, h->k);
    MRBF_HIP(ctx, hipGetLastError());
    MRBF_HIP(ctx, hipStreamSynchronize(s));
    return MRBF_OK;
}

int32_t mrbf_db_read(mrbf_ctx *ctx, const mrbf_db *h, int64_t first, int64_t m, double *sites_out, double *values_out) {
    if (!ctx) return -1;
    if (!h || h->ctx != ctx) return fail(ctx, -2, "mrbf_db_read: db is NULL or belongs to another context");
    if (first < 0 || first > h->n) return fail(ctx, -3, "mrbf_db_read: first = %lld of %lld rows", (long long)first, (long long)h->n);
    if (m < 0 || first + m > h->n) return fail(ctx, -4, "mrbf_db_read: m = %lld from row %lld of %lld", (long long)m, (long long)first, (long long)h->n);
    if (m == 0) return MRBF_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    const size_t D = (size_t)h->d, K = (size_t)h->k, F = (size_t)first, M = (size_t)m;
    if (sites_out) MRBF_HIP(ctx, hipMemcpyAsync(sites_out, h->sites + F * D, M * D * sizeof(double), hipMemcpyDefault, s));
    if (values_out) MRBF_HIP(ctx, hipMemcpyAsync(values_out, h->values + F * K, M * K * sizeof(double), hipMemcpyDefault, s));
    MRBF_HIP(ctx, hipStreamSynchronize(s));
    return MRBF_OK;
}

int32_t mrbf_db_dims(const mrbf_db *h, int64_t *n_sites, int32_t *d, int32_t *k) {
    if (!h) return -1;
    if (n_sites) *n_sites = h->n;
    if (d) *d = h->d;
    if (k) *k = h->k;
    return MRBF_OK;
}

int32_t mrbf_db_free(mrbf_ctx *ctx, mrbf_db *h) {
    if (!ctx) return -1;
    if (!h) return MRBF_OK;
    if (h->ctx != ctx) return fail(ctx, -2, "mrbf_db_free: db belongs to another context");
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (h->sites) (void)hipFree(h->sites);
    if (h->values) (void)hipFree(h->values);
    --ctx->live_dbs;
    delete h;
    return MRBF_OK;
}

int32_t mrbf_db_box_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, int32_t p_is_inf, mrbf_db_box_job *jobs, float *ms_total) {
    using namespace db;
    std::vector<DbInfo> info;
    MRBF_TRY(open_batch(ctx, "mrbf_db_box_batch", n_starts, d, jobs, 5, info, [&] { return check_box_jobs(n_starts, d, jobs, info.data(), 5); }));
    const size_t N = (size_t)n_starts, D = (size_t)d;
    std::vector<int64_t> rows(N);
    for (size_t p = 0; p < N; ++p) rows[p] = info[p].n;
    const BoxLayout L = box_layout(n_starts, d, rows.data(), sizeof(BoxDesc));
    chain::SelectCall call(ctx, ms_total);
    hipStream_t s = call.s;
    double *views;
    MRBF_TRY(get_buf(ctx, S_DB_BOX, L.view_doubles, &views));
    // ---- one upload: descriptors, bounds and centres, exclusion masks
    MRBF_TRY(call.open(S_DB_WS, L.A, L.A.upload_bytes()));
    BoxDesc *hdesc = call.host<BoxDesc>(L.oDesc);
    bool want_idx = false;
    for (size_t p = 0; p < N; ++p) {
        const mrbf_db_box_job &jb = jobs[p];
        const size_t r0 = (size_t)L.roff[p];
        BoxDesc &h = hdesc[p];
        h.S = jb.db->sites;
        h.bounds = call.dev<const double>(L.oBounds) + p * 3 * D, h.flag = call.dev<unsigned char>(L.oMask) + r0;
        h.norm = call.dev<double>(L.oNorm) + r0, h.cnorm = call.dev<double>(L.oCnorm) + r0;
        h.count = call.dev<int>(L.oCount) + r0 / ROWS, h.offs = call.dev<int>(L.oOffs) + r0 / ROWS;
        h.head = call.dev<long long>(L.oHead) + 2 * p, h.first = call.dev<double>(L.oFirst) + p * D, h.idx = call.dev<long long>(L.oIdx) + r0;
        h.vs = views + L.sites_view((int64_t)p, d), h.vh = views + L.shifted_view((int64_t)p, d);
        h.n = rows[p], h.nblk = (int)((rows[p] + ROWS - 1) / ROWS), h.zero = jb.zero_first_pick != 0;
        double *b = call.host<double>(L.oBounds) + p * 3 * D;
        std::memcpy(b, jb.lb, D * sizeof(double)), std::memcpy(b + D, jb.ub, D * sizeof(double)), std::memcpy(b + 2 * D, jb.x0, D * sizeof(double));
        build_mask(rows[p], jb.n_exclude, jb.exclude, call.host<unsigned char>(L.oMask) + r0);
        want_idx = want_idx || jb.indices_out != nullptr;
    }
    MRBF_TRY(call.begin());
    MRBF_TRY(call.upload());
    const BoxDesc *ddesc = call.dev<const BoxDesc>(L.oDesc);
    const dim3 grows((unsigned)std::max<int64_t>(L.nblk_max, 1), (unsigned)N);
    if (L.nblk_max > 0) hipLaunchKernelGGL(db_flag_kernel, grows, dim3(NT), 0, s, ddesc, d, p_is_inf ? 1 : 0);
    hipLaunchKernelGGL(db_scan_kernel, dim3((unsigned)N), dim3(NT), 0, s, ddesc);
    if (L.nblk_max > 0) hipLaunchKernelGGL(db_compact_kernel, grows, dim3(NT), 0, s, ddesc, d);
    hipLaunchKernelGGL(db_pick_kernel, dim3((unsigned)N), dim3(NT), 0, s, ddesc, d);
    // ---- one read-back: counts, first picks and their rows [, the candidates' indices]
    MRBF_TRY(call.finish(want_idx ? L.A.back_bytes() : L.back_head_bytes));
    const long long *head = reinterpret_cast<const long long *>(call.back.p);
    const double *first = reinterpret_cast<const double *>(call.back.p + (L.oFirst - L.oHead));
    const long long *idx = reinterpret_cast<const long long *>(call.back.p + (L.oIdx - L.oHead));
    for (size_t p = 0; p < N; ++p) {
        mrbf_db_box_job &jb = jobs[p];
        const int64_t mc = head[2 * p], pick = head[2 * p + 1];
        if (mc < 0 || mc > rows[p] || pick >= mc) {  // (cannot happen: a count the kernels produced)
            jb.rc = MRBF_EHIP;
            continue;
        }
        if (!view_out(jb.sites_out, hdesc[p].vs, (size_t)mc * D) || !view_out(jb.shifted_out, hdesc[p].vh, (size_t)mc * D)) {
            jb.rc = MRBF_EHIP;
            continue;
        }
        if (jb.indices_out)
            for (int64_t i = 0; i < mc; ++i) jb.indices_out[i] = (int64_t)idx[(size_t)L.roff[p] + (size_t)i];
        if (mc > 0) std::memcpy(jb.first_row, first + p * D, D * sizeof(double));
        jb.mc = mc, jb.first_pick = pick;
        jb.cand_sites_dev = hdesc[p].vs, jb.shifted_dev = hdesc[p].vh;
        jb.rc = 0;
    }
    return MRBF_OK;
}

int32_t mrbf_db_gather_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, mrbf_db_gather_job *jobs, float *ms_total) {
    using namespace db;
    std::vector<DbInfo> info;
    MRBF_TRY(open_batch(ctx, "mrbf_db_gather_batch", n_starts, d, jobs, 4, info, [&] { return check_gather_jobs(n_starts, d, jobs, info.data(), 4); }));
    const size_t N = (size_t)n_starts, D = (size_t)d;
    std::vector<int64_t> cnt(N);
    std::vector<int> ks(N), rcs(N);
    for (size_t p = 0; p < N; ++p) {
        rcs[p] = index_rc(info[p].n, jobs[p].n_idx, jobs[p].indices, GATHER_RC_INDEX);
        cnt[p] = rcs[p] == 0 ? jobs[p].n_idx : -1;  // a job that failed its own check takes no part
        ks[p] = info[p].k;
    }
    const GatherLayout L = gather_layout(n_starts, d, ks.data(), cnt.data(), sizeof(GatherDesc));
    chain::SelectCall call(ctx, ms_total);
    double *views;
    MRBF_TRY(get_buf(ctx, S_DB_GATHER, L.view_doubles, &views));
    MRBF_TRY(call.open(S_DB_WS, L.A, L.A.total));
    GatherDesc *hdesc = call.host<GatherDesc>(L.oDesc);
    for (size_t p = 0; p < N; ++p) {
        GatherDesc &h = hdesc[p];
        h.S = jobs[p].db->sites, h.V = jobs[p].db->values;
        h.idx = call.dev<const long long>(L.oIdx) + L.ioff[p];
        h.so = views + L.soff[p], h.vo = views + L.voff[p];
        h.m = std::max<int64_t>(cnt[p], 0), h.k = ks[p];
        if (h.m > 0) std::memcpy(call.host<int64_t>(L.oIdx) + L.ioff[p], jobs[p].indices, (size_t)h.m * sizeof(int64_t));
    }
    MRBF_TRY(call.begin());
    MRBF_TRY(call.upload());
    if (L.n_idx_max > 0) {
        const dim3 grid((unsigned)std::min<int64_t>((L.n_idx_max + 3) / 4, 1024), (unsigned)N);
        hipLaunchKernelGGL(db_gather_kernel, grid, dim3(NT), 0, call.s, call.dev<const GatherDesc>(L.oDesc), d);
    }
    MRBF_TRY(call.finish(0));
    for (size_t p = 0; p < N; ++p) {
        mrbf_db_gather_job &jb = jobs[p];
        if (rcs[p] != 0) {
            jb.rc = rcs[p];
            continue;
        }
        const size_t m = (size_t)jb.n_idx;
        if (!view_out(jb.sites_out, hdesc[p].so, m * D) || !view_out(jb.values_out, hdesc[p].vo, m * (size_t)ks[p])) {
            jb.rc = MRBF_EHIP;
            continue;
        }
        jb.sites_dev = hdesc[p].so, jb.values_dev = hdesc[p].vo;
        jb.rc = 0;
    }
    return MRBF_OK;
}

int32_t mrbf_db_append_batch(mrbf_ctx *ctx, int64_t n_starts, mrbf_db_append_job *jobs, float *ms_total) {
    using namespace db;
    std::vector<DbInfo> info;
    MRBF_TRY(open_batch(ctx, "mrbf_db_append_batch", n_starts, 1, jobs, 3, info, [&] { return check_append_jobs(n_starts, jobs, info.data(), 3); }));
    const size_t N = (size_t)n_starts;
    chain::SelectCall call(ctx, ms_total);
    // ---- the upload: the descriptors, then the host-side rows of every start (device-side rows are read in place)
    ByteArena A;
    A.take(N * sizeof(AppendDesc));
    std::vector<size_t> os(N, 0), ov(N, 0);  // (0: read in place, or none)
    int64_t cnt_max = 0;
    for (size_t p = 0; p < N; ++p) {
        const mrbf_db_append_job &jb = jobs[p];
        const size_t M = (size_t)jb.m, D = (size_t)info[p].d, K = (size_t)info[p].k;
        cnt_max = std::max<int64_t>(cnt_max, (int64_t)(M * std::max(D, K)));
        if (M == 0) continue;
        if (!is_device_ptr(jb.sites)) os[p] = A.take(M * D * sizeof(double));
        if (jb.values && !is_device_ptr(jb.values)) ov[p] = A.take(M * K * sizeof(double));
    }
    A.up_end = A.total;
    for (size_t p = 0; p < N; ++p) MRBF_TRY(reserve(ctx, jobs[p].db, info[p].n + jobs[p].m));
    MRBF_TRY(call.open(S_DB_WS, A, N * sizeof(AppendDesc)));
    for (size_t p = 0; p < N; ++p) {
        const mrbf_db_append_job &jb = jobs[p];
        const mrbf_db *h = jb.db;
        const size_t M = (size_t)jb.m, D = (size_t)h->d, K = (size_t)h->k, n = (size_t)h->n;
        AppendDesc &a = call.host<AppendDesc>(0)[p];
        a.S = h->sites + n * D, a.V = h->values + n * K, a.m = jb.m, a.d = h->d, a.k = h->k;
        if (M == 0) continue;
        a.ss = os[p] ? call.dev<const double>(os[p]) : jb.sites;
        a.sv = ov[p] ? call.dev<const double>(ov[p]) : jb.values;
        if (os[p]) std::memcpy(call.host<char>(os[p]), jb.sites, M * D * sizeof(double));
        if (ov[p]) std::memcpy(call.host<char>(ov[p]), jb.values, M * K * sizeof(double));
    }
    MRBF_TRY(launch_update(call, db_append_batch_kernel, N, cnt_max));  // (synchronised: the callers' buffers are their own again)
    for (size_t p = 0; p < N; ++p) {
        jobs[p].first_index = jobs[p].db->n;
        jobs[p].db->n += jobs[p].m;
        jobs[p].rc = 0;
    }
    return MRBF_OK;
}

int32_t mrbf_db_set_values_batch(mrbf_ctx *ctx, int64_t n_starts, mrbf_db_set_values_job *jobs, float *ms_total) {
    using namespace db;
    std::vector<DbInfo> info;
    MRBF_TRY(open_batch(ctx, "mrbf_db_set_values_batch", n_starts, 1, jobs, 3, info, [&] { return check_set_values_jobs(n_starts, jobs, info.data(), 3); }));
    const size_t N = (size_t)n_starts;
    chain::SelectCall call(ctx, ms_total);
    ByteArena A;
    A.take(N * sizeof(SetDesc));
    std::vector<size_t> oi(N, 0), ov(N, 0);  // (ov 0: read in place)
    std::vector<int> rcs(N, 0);
    int64_t cnt_max = 0;
    for (size_t p = 0; p < N; ++p) {
        const mrbf_db_set_values_job &jb = jobs[p];
        rcs[p] = index_rc(info[p].n, jb.m, jb.indices, SET_VALUES_RC_INDEX);
        if (rcs[p] != 0 || jb.m == 0) continue;  // a job that failed its own check takes no part
        const size_t M = (size_t)jb.m, K = (size_t)info[p].k;
        cnt_max = std::max<int64_t>(cnt_max, (int64_t)(M * K));
        oi[p] = A.take(M * sizeof(int64_t));
        if (!is_device_ptr(jb.values)) ov[p] = A.take(M * K * sizeof(double));
    }
    A.up_end = A.total;
    MRBF_TRY(call.open(S_DB_WS, A, N * sizeof(SetDesc)));
    for (size_t p = 0; p < N; ++p) {
        const mrbf_db_set_values_job &jb = jobs[p];
        SetDesc &a = call.host<SetDesc>(0)[p];
        a.V = jb.db->values, a.k = jb.db->k;
        if (rcs[p] != 0 || jb.m == 0) continue;
        const size_t M = (size_t)jb.m, K = (size_t)a.k;
        a.m = jb.m;
        a.idx = call.dev<const long long>(oi[p]);
        a.vals = ov[p] ? call.dev<const double>(ov[p]) : jb.values;
        std::memcpy(call.host<char>(oi[p]), jb.indices, M * sizeof(int64_t));
        if (ov[p]) std::memcpy(call.host<char>(ov[p]), jb.values, M * K * sizeof(double));
    }
    MRBF_TRY(launch_update(call, db_set_values_batch_kernel, N, cnt_max));
    for (size_t p = 0; p < N; ++p) jobs[p].rc = rcs[p];
    return MRBF_OK;
}

}  // extern "C"
