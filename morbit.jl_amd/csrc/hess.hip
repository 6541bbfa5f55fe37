// Model Hessians: the second derivative of model(x, l) with respect to the scaled site, for m queries and r selected outputs,
//     H_l(x) = sum_c w_cl [ psi(s_c) I + chi(s_c) (x - c)(x - c)' ],   s_c = |x - c|^2,  psi = phi'/rho,  chi = 2 dpsi/ds
// (radial.hpp: rbf_psi_chi; the polynomial tail has degree <= 1 and no second derivative).  For one query and output the rank-one
// sum is a d x n by n x d product, done on the fp64 matrix cores (v_mfma_f64_16x16x4_f64) with the differences x - c as both factors:
// the difference form of DESIGN.md section 4b for every radial function, on the coordinates as given (mrbf_model::C, the caller's X).
//
// hess_kernel: one workgroup = (query, output pass, pair of 64-coordinate blocks bi <= bj, piece of the centre range).  Per round of
// NC = 32 centres
//   phase A   8 threads per centre walk the d coordinates once: x - c, the sum of squares behind s (a fixed order: every thread its
//             stride-8 coordinates in turn, then a three-level exchange), the columns of the two blocks kept in LDS; psi and chi of s,
//             g_cl = w_cl chi for the pass's outputs (0 at s = 0 and for padding centres: selected, not multiplied)
//   phase B   the upper-triangle 16 x 16 tiles of the block pair dealt round-robin to the four waves (at most four each), per tile and
//             output one MFMA per four centres with A = g (x - c)_i, B = (x - c)_j read from the same LDS columns
// and the diagonal term sum_c w_cl psi_c is summed in centre order by one thread per output of the diagonal pairs and added once, at
// the store.  The centre range in one piece: the tiles go to hess_out, the mirrored entry written from the same register.  Split
// (hess_host.hpp: nsplit): every piece writes its tiles to a partial block, hess_reduce_kernel adds the pieces in order 0, 1, ...
// and stores both triangles.  No atomics: a query's blocks depend on its coordinates, the model and the split count alone.
//
// Many starts (mrbf_eval_hessian_batch): the two bodies are device functions; hess_batch_kernel and
// hess_reduce_batch_kernel run them for an array of HessArgs -- one per job, or per range of a job's points -- with the block index
// local to the descriptor a workgroup finds in a table of first blocks (hess_batch_host.hpp).  Every job keeps the split of the single
// call it stands for, so its bits are that call's.
#include <algorithm>

#define MRBF_HD __host__ __device__
#include "radial.hpp"
#include "hess_batch_host.hpp"

using namespace mrbf;

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int SB = hess::SB, NC = hess::NC;
constexpr int LDD = SB + 8;  // row stride of the difference columns in LDS (doubles)

struct HessArgs {
    const double *X;      // the launch's queries, points x d
    const double *C;      // n x d centres as given
    const double *W;      // n x k weights
    const int32_t *rows;  // r selected outputs
    double *out;          // points x r x d x d
    double *part;         // partial blocks (nsplit > 1)
    int64_t n, per;       // centres; centres of a piece
    int d, k, r, npass, nsplit, nb;
    int64_t npairs;
    KP kp;
};

// upper-triangle tiles of a diagonal block pair in the order they are dealt: (ti, tj) of entry t in nibble t
constexpr unsigned long long UT_I = 0x3221110000ULL, UT_J = 0x3323213210ULL;

// the work of one workgroup of the main kernel: block `blk` of the launch (or of the descriptor) that A describes
template <int KID, bool FAST, int RB>
__device__ __forceinline__ void hess_body(const HessArgs &A, const uint32_t blk) {
    __shared__ double Di[NC][LDD], Dj[NC][LDD];
    __shared__ double G[NC][RB], WP[NC][RB];
    __shared__ double dsum_s[RB];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blk = ((p * npass + pass) * npairs + pair) * nsplit + sp
    int64_t idx = blk;
    const int sp = (int)(idx % A.nsplit);
    idx /= A.nsplit;
    int pair = (int)(idx % A.npairs);
    idx /= A.npairs;
    const int pass = (int)(idx % A.npass);
    const int64_t p = idx / A.npass;
    int bi = 0;
    while (pair >= A.nb - bi) pair -= A.nb - bi, ++bi;
    const int bj = bi + pair;
    const bool diag = bi == bj;
    const int d = A.d;
    const int64_t c0 = (int64_t)sp * A.per, c1 = c0 + A.per < A.n ? c0 + A.per : A.n;
    const double *x = A.X + p * d;
    double(*Dcol)[LDD] = diag ? Di : Dj;

    // this wave's tiles
    const int ntl = diag ? 10 : 16;
    int ti[4], tj[4];
    bool on[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = wave + 4 * q;
        ti[q] = diag ? (int)((UT_I >> (4 * t)) & 15) : t >> 2;
        tj[q] = diag ? (int)((UT_J >> (4 * t)) & 15) : t & 3;
        on[q] = t < ntl && bi * SB + ti[q] * 16 < d && bj * SB + tj[q] * 16 < d;
    }
    v4d acc[4][RB];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int l = 0; l < RB; ++l) acc[q][l] = v4d{0.0, 0.0, 0.0, 0.0};
    double dsum = 0.0;

    const int cl = tid >> 3, u = tid & 7;
    const int tmax = (bj + 1) * SB > d ? (bj + 1) * SB : d;
    for (int64_t cb = c0; cb < c1; cb += NC) {
        // ---- phase A
        const int64_t cg = cb + cl;
        const bool valid = cg < c1;
        const double *crow = A.C + (valid ? cg : c0) * d;
        double s = 0.0;
        for (int t = u; t < tmax; t += 8) {
            const double dl = (valid && t < d) ? x[t] - crow[t] : 0.0;
            s = fma(dl, dl, s);
            const int a = t - bi * SB, b = t - bj * SB;
            if (a >= 0 && a < SB) Di[cl][a] = dl;
            if (!diag && b >= 0 && b < SB) Dj[cl][b] = dl;
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        double psi, chi;
        rbf_psi_chi<KID, FAST>(s, A.kp, psi, chi);
        if (u < RB) {
            const int lg = pass * RB + u;
            const double w = (valid && lg < A.r) ? A.W[cg * A.k + A.rows[lg]] : 0.0;
            G[cl][u] = (valid && s > 0.0) ? w * chi : 0.0;
            WP[cl][u] = valid ? w * psi : 0.0;
        }
        __syncthreads();
        if (diag && tid < RB)
            for (int c = 0; c < NC; ++c) dsum += WP[c][tid];
        // ---- phase B
#pragma unroll 2
        for (int kk = 0; kk < NC / 4; ++kk) {
            const int c = kk * 4 + l4;
            double g[RB];
#pragma unroll
            for (int l = 0; l < RB; ++l) g[l] = G[c][l];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (on[q]) {
                    const double a = Di[c][ti[q] * 16 + l15], b = Dcol[c][tj[q] * 16 + l15];
#pragma unroll
                    for (int l = 0; l < RB; ++l) acc[q][l] = __builtin_amdgcn_mfma_f64_16x16x4f64(a * g[l], b, acc[q][l], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    if (diag && tid < RB) dsum_s[tid] = dsum;
    __syncthreads();

    // ---- store (f64 MFMA C/D layout: col = lane & 15 -> j, row = (lane >> 4) + 4 reg -> i)
    const bool split = A.nsplit > 1;
    double *pblk = split ? A.part + (int64_t)blk * RB * SB * SB : nullptr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!on[q]) continue;
#pragma unroll
        for (int l = 0; l < RB; ++l) {
            const int lg = pass * RB + l;
            if (lg >= A.r) continue;
            double *H = A.out + (p * A.r + lg) * (int64_t)d * d;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int il = ti[q] * 16 + l4 + 4 * reg, jl = tj[q] * 16 + l15;
                const int i = bi * SB + il, j = bj * SB + jl;
                if (i >= d || j >= d || i > j) continue;
                double v = acc[q][l][reg];
                if (i == j) v += dsum_s[l];
                if (split) {
                    pblk[((int64_t)l * SB + il) * SB + jl] = v;
                } else {
                    H[(int64_t)i * d + j] = v;
                    if (i != j) H[(int64_t)j * d + i] = v;
                }
            }
        }
    }
}

template <int KID, bool FAST, int RB>
__global__ __launch_bounds__(256) void hess_kernel(const HessArgs A) {
    hess_body<KID, FAST, RB>(A, blockIdx.x);
}

// The batched form: nd descriptors and their first blocks tb[0] = 0, ..., tb[nd] = gridDim.x (hess_batch_host.hpp).  The lookup reads
// blockIdx.x and kernel arguments alone, so the descriptor's index is uniform over the workgroup and its fields come by scalar loads;
// every workgroup of the grid belongs to a descriptor and has work.
template <int KID, bool FAST, int RB>
__global__ __launch_bounds__(256) void hess_batch_kernel(const HessArgs *__restrict__ descs, const uint32_t *__restrict__ tb, const int nd) {
    uint32_t local;
    const int i = hessbatch::lookup(tb, nd, blockIdx.x, &local);
    const HessArgs A = descs[i];
    hess_body<KID, FAST, RB>(A, local);
}

// block (((p * npass + pass) * npairs + pair) * RB + l) * 16 + g: output l of the pass, rows 4 g .. 4 g + 3 of the 64 x 64 block, one
// entry per thread.  The pieces of the centre range are added in order 0, 1, ..., both triangles stored.
template <int RB>
__device__ __forceinline__ void hess_reduce_body(const HessArgs &A, const uint32_t rblk) {
    int64_t idx = rblk;
    const int g = (int)(idx % 16);
    idx /= 16;
    const int l = (int)(idx % RB);
    idx /= RB;
    const int64_t blk = idx;  // (p * npass + pass) * npairs + pair: the main launch's block index without the piece
    int pair = (int)(idx % A.npairs);
    idx /= A.npairs;
    const int pass = (int)(idx % A.npass);
    const int64_t p = idx / A.npass;
    int bi = 0;
    while (pair >= A.nb - bi) pair -= A.nb - bi, ++bi;
    const int bj = bi + pair;
    const int d = A.d;
    const int lg = pass * RB + l;
    if (lg >= A.r) return;
    const int e = g * 256 + threadIdx.x;
    const int i = bi * SB + e / SB, j = bj * SB + e % SB;
    if (i >= d || j >= d || i > j) return;
    const double *src = A.part + (blk * A.nsplit * RB + l) * (int64_t)(SB * SB) + e;
    const int64_t stride = (int64_t)RB * SB * SB;
    double v = src[0];
#pragma unroll 8
    for (int s = 1; s < A.nsplit; ++s) v += src[s * stride];
    double *H = A.out + (p * A.r + lg) * (int64_t)d * d;
    H[(int64_t)i * d + j] = v;
    if (i != j) H[(int64_t)j * d + i] = v;
}

template <int RB>
__global__ __launch_bounds__(256) void hess_reduce_kernel(const HessArgs A) {
    hess_reduce_body<RB>(A, blockIdx.x);
}

template <int RB>
__global__ __launch_bounds__(256) void hess_reduce_batch_kernel(const HessArgs *__restrict__ descs, const uint32_t *__restrict__ tb, const int nd) {
    uint32_t local;
    const int i = hessbatch::lookup(tb, nd, blockIdx.x, &local);
    const HessArgs A = descs[i];
    hess_reduce_body<RB>(A, local);
}

// one launch of the main kernel: the single call's (one HessArgs by value) or the batched form's (descriptors and first blocks)
struct MainLaunch {
    const HessArgs *single = nullptr;
    const HessArgs *descs = nullptr;
    const uint32_t *tb = nullptr;
    int nd = 0;
};

template <int KID, bool FAST, int RB>
void launch_one(const MainLaunch &L, int64_t grid, hipStream_t st) {
    if (L.single) hipLaunchKernelGGL((hess_kernel<KID, FAST, RB>), dim3((unsigned)grid), dim3(256), 0, st, *L.single);
    else hipLaunchKernelGGL((hess_batch_kernel<KID, FAST, RB>), dim3((unsigned)grid), dim3(256), 0, st, L.descs, L.tb, L.nd);
}

template <int KID, bool FAST>
void launch_rb(const MainLaunch &L, int rb, int64_t grid, hipStream_t st) {
    if (rb == 1) launch_one<KID, FAST, 1>(L, grid, st);
    else if (rb == 2) launch_one<KID, FAST, 2>(L, grid, st);
    else launch_one<KID, FAST, 4>(L, grid, st);
}

// the instantiation a radial function takes: the fast form where it has one and the parameters ask for it
void launch_main(const KP &kp, const MainLaunch &L, int rb, int64_t grid, hipStream_t st) {
    const bool fast = kp.fast != 0;
    MRBF_DISPATCH_KID(kp.kid, {
        constexpr bool HAS_FAST = KID == MRBF_CUBIC || KID == MRBF_MULTIQUADRIC || KID == MRBF_INV_MULTIQUADRIC;
        if constexpr (HAS_FAST) {
            if (fast) launch_rb<KID, true>(L, rb, grid, st);
            else launch_rb<KID, false>(L, rb, grid, st);
        } else {
            launch_rb<KID, false>(L, rb, grid, st);
        }
    });
}

// ... and its number, without the pass width: what decides, with it, which jobs of a batch share a launch
int variant_of(const KP &kp) {
    int v = 0;
    MRBF_DISPATCH_KID(kp.kid, {
        constexpr bool HAS_FAST = KID == MRBF_CUBIC || KID == MRBF_MULTIQUADRIC || KID == MRBF_INV_MULTIQUADRIC;
        v = 2 * KID + (HAS_FAST && kp.fast != 0 ? 1 : 0);
    });
    return v;
}

void launch_reduce(const MainLaunch &L, int rb, int64_t grid, hipStream_t st) {
    if (L.single) {
        if (rb == 1) hipLaunchKernelGGL((hess_reduce_kernel<1>), dim3((unsigned)grid), dim3(256), 0, st, *L.single);
        else if (rb == 2) hipLaunchKernelGGL((hess_reduce_kernel<2>), dim3((unsigned)grid), dim3(256), 0, st, *L.single);
        else hipLaunchKernelGGL((hess_reduce_kernel<4>), dim3((unsigned)grid), dim3(256), 0, st, *L.single);
    } else {
        if (rb == 1) hipLaunchKernelGGL((hess_reduce_batch_kernel<1>), dim3((unsigned)grid), dim3(256), 0, st, L.descs, L.tb, L.nd);
        else if (rb == 2) hipLaunchKernelGGL((hess_reduce_batch_kernel<2>), dim3((unsigned)grid), dim3(256), 0, st, L.descs, L.tb, L.nd);
        else hipLaunchKernelGGL((hess_reduce_batch_kernel<4>), dim3((unsigned)grid), dim3(256), 0, st, L.descs, L.tb, L.nd);
    }
}

// `points` queries at Xd into out (device, points x r x d x d)
int launch_points(mrbf_ctx *ctx, const mrbf_model *M, int64_t points, const double *Xd, const int32_t *rows, int r, int ns, int64_t per,
                  double *part, double *out) {
    HessArgs A;
    A.C = M->C, A.W = M->W, A.rows = rows, A.part = part;
    A.n = M->n, A.per = per, A.d = M->d, A.k = M->k, A.r = r;
    A.npass = hess::npass(r), A.nsplit = ns, A.nb = hess::nblocks(M->d), A.npairs = hess::npairs(M->d);
    A.kp = M->kp;
    const int rb = hess::rb(r);
    const int64_t per_point = (int64_t)A.npass * A.npairs * ns;
    const int64_t most = std::max<int64_t>(1, ((int64_t)1 << 30) / (per_point * 64));  // grid.x of both launches stays below 2^31
    for (int64_t p0 = 0; p0 < points; p0 += most) {
        const int64_t cnt = std::min(most, points - p0);
        A.X = Xd + p0 * M->d;
        A.out = out + p0 * r * (int64_t)M->d * M->d;
        MainLaunch L;
        L.single = &A;
        launch_main(A.kp, L, rb, cnt * per_point, ctx->stream);
        MRBF_HIP(ctx, hipGetLastError());
        if (ns > 1) {
            launch_reduce(L, rb, cnt * A.npass * A.npairs * rb * 16, ctx->stream);
            MRBF_HIP(ctx, hipGetLastError());
        }
    }
    return 0;
}

static_assert(sizeof(mrbf_hess_job) == 56, "mrbf_hess_job is 56 bytes");
static_assert(sizeof(mrbf_hess_batch_info) == 16, "mrbf_hess_batch_info is 16 bytes");
static_assert(sizeof(HessArgs) % sizeof(double) == 0, "descriptors are counted in doubles");
constexpr size_t DESC_DOUBLES = sizeof(HessArgs) / sizeof(double);

// jobs first .. first + count - 1 (validated, at least one active): tables, arena, upload, launches, read-back, synchronisation
int run_batch_chunk(mrbf_ctx *ctx, mrbf_hess_job *jobs, const hessbatch::Job *shape, int64_t first, int64_t count, float *ms, int *groups) {
    const hessbatch::Table mt = hessbatch::table(shape, first, count, false), rt = hessbatch::table(shape, first, count, true);
    const hessbatch::Layout L = hessbatch::layout(shape, first, count, mt, rt, DESC_DOUBLES);
    PinGuard pin(ctx);
    double *base;
    MRBF_TRY(get_buf(ctx, S_HESS_BATCH, L.total, &base));
    const size_t staged_most = (size_t)4 << 20;
    std::vector<double> own_up, own_down;
    double *hup = L.up_cnt * sizeof(double) <= staged_most ? reinterpret_cast<double *>(pin_take(ctx, L.up_cnt * sizeof(double))) : nullptr;
    if (!hup) {
        own_up.resize(L.up_cnt);
        hup = own_up.data();
    }
    // ---- the upload: row lists, host-side query rows, descriptors, first blocks
    for (int64_t i = 0; i < count; ++i) {
        const hessbatch::Job &S = shape[first + i];
        if (!hessbatch::active(S)) continue;
        const hessbatch::Place &at = L.at[(size_t)i];
        hess::Call c;
        c.k = S.k, c.n_rows = S.n_rows, c.rows = S.rows;
        const std::vector<int32_t> rows = hess::row_list(c);
        std::memcpy(hup + at.rows, rows.data(), rows.size() * sizeof(int32_t));
        if (at.X != hessbatch::NONE) std::memcpy(hup + at.X, jobs[first + i].X, (size_t)S.m * S.d * sizeof(double));
    }
    auto fill = [&](const hessbatch::Table &T, size_t desc_at, size_t table_at) {
        HessArgs *hd = reinterpret_cast<HessArgs *>(hup + desc_at);
        for (size_t t = 0; t < T.items.size(); ++t) {
            const hessbatch::Item &it = T.items[t];
            const hessbatch::Job &S = shape[it.job];
            const mrbf_hess_job &J = jobs[it.job];
            const hessbatch::Place &at = L.at[(size_t)(it.job - first)];
            const mrbf_model *M = J.model;
            const int r = hessbatch::outputs(S);
            HessArgs A;
            std::memset(&A, 0, sizeof(A));
            A.X = (at.X == hessbatch::NONE ? J.X : base + at.X) + it.p0 * S.d;
            A.out = (at.out == hessbatch::NONE ? J.hess_out : base + at.out) + it.p0 * r * (int64_t)S.d * S.d;
            A.C = M->C, A.W = M->W;
            A.rows = reinterpret_cast<const int32_t *>(base + at.rows);
            A.part = at.part == hessbatch::NONE ? nullptr : base + at.part;
            A.n = M->n, A.d = M->d, A.k = M->k, A.r = r;
            A.nsplit = hessbatch::split(S, &A.per);
            A.npass = hess::npass(r), A.nb = hess::nblocks(M->d), A.npairs = hess::npairs(M->d);
            A.kp = M->kp;
            hd[t] = A;
        }
        if (!T.first_block.empty()) std::memcpy(hup + table_at, T.first_block.data(), T.first_block.size() * sizeof(uint32_t));
    };
    fill(mt, L.main_desc, L.main_table);
    fill(rt, L.red_desc, L.red_table);
    hipStream_t st = ctx->stream;
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    MRBF_HIP(ctx, hipMemcpyAsync(base, hup, L.up_cnt * sizeof(double), hipMemcpyHostToDevice, st));
    // ---- one main launch per group, then one combining launch per group of split jobs
    auto at_launch = [&](const hessbatch::Launch &G, size_t desc_at, size_t table_at) {
        MainLaunch ML;
        ML.descs = reinterpret_cast<const HessArgs *>(base + desc_at) + G.first;
        ML.tb = reinterpret_cast<const uint32_t *>(base + table_at) + G.table;
        ML.nd = (int)G.count;
        return ML;
    };
    for (const hessbatch::Launch &G : mt.launches) {
        launch_main(jobs[mt.items[G.first].job].model->kp, at_launch(G, L.main_desc, L.main_table), G.key & 7, G.grid, st);
        MRBF_HIP(ctx, hipGetLastError());
    }
    for (const hessbatch::Launch &G : rt.launches) {
        launch_reduce(at_launch(G, L.red_desc, L.red_table), G.key, G.grid, st);
        MRBF_HIP(ctx, hipGetLastError());
    }
    *groups += (int)mt.launches.size();
    // ---- the read-back: one block into the pinned staging where it fits; beyond that straight into the callers' buffers
    const bool staged = L.out_cnt * sizeof(double) <= staged_most;
    double *down = nullptr;
    if (staged && L.out_cnt) {
        down = reinterpret_cast<double *>(pin_take(ctx, L.out_cnt * sizeof(double)));
        if (!down) {
            own_down.resize(L.out_cnt);
            down = own_down.data();
        }
        MRBF_HIP(ctx, hipMemcpyAsync(down, base + L.out0, L.out_cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    auto result_doubles = [&](int64_t i) { return (size_t)shape[first + i].m * hessbatch::outputs(shape[first + i]) * shape[first + i].d * shape[first + i].d; };
    if (!staged)
        for (int64_t i = 0; i < count; ++i)
            if (L.at[(size_t)i].out != hessbatch::NONE)
                MRBF_HIP(ctx, hipMemcpyAsync(jobs[first + i].hess_out, base + L.at[(size_t)i].out, result_doubles(i) * sizeof(double),
                                             hipMemcpyDeviceToHost, st));
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    MRBF_HIP(ctx, hipStreamSynchronize(st));
    if (staged && L.out_cnt)
        for (int64_t i = 0; i < count; ++i)
            if (L.at[(size_t)i].out != hessbatch::NONE)
                std::memcpy(jobs[first + i].hess_out, down + (L.at[(size_t)i].out - L.out0), result_doubles(i) * sizeof(double));
    float t = 0.f;
    MRBF_HIP(ctx, hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]));
    *ms += t;
    return 0;
}

}  // namespace

namespace mrbf {

// the validated call (api.hip): stage X, upload the selected outputs, one chain per chunk of query points on the ctx stream, one
// synchronisation.  The split count is that of the whole call, so a result does not depend on how it was chunked.
int hess_call(mrbf_ctx *ctx, const mrbf_model *M, int64_t m, const double *X, const std::vector<int32_t> &rows, double *hess_out,
              mrbf_hess_info *info, int64_t stage_bytes) {
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    const int d = M->d, r = (int)rows.size();
    int64_t per = 0;
    const int ns = hess::nsplit(m, M->n, d, r, &per);
    const size_t point = (size_t)r * d * d;
    const bool out_dev = is_device_ptr(hess_out);
    std::vector<std::pair<int64_t, int64_t>> chunks;
    if (out_dev) chunks.push_back({0, m});
    else chunks = hess::chunks(m, point * sizeof(double), stage_bytes);
    int64_t widest = 0;
    for (const auto &c : chunks) widest = std::max(widest, c.second);
    // (a split call has fewer than TARGET_WGS workgroups per piece of the centre range: its partial blocks stay small)
    const hess::Layout L = hess::layout(widest, d, r, ns);
    const double *Xd;
    double *ws, *stage = nullptr;
    MRBF_TRY(stage_in(ctx, S_STAGE_C, X, (size_t)m * d, &Xd));
    MRBF_TRY(get_buf(ctx, S_HESS_WS, L.total, &ws));
    if (!out_dev) MRBF_TRY(get_buf(ctx, S_HESS_OUT, (size_t)widest * point, &stage));
    int32_t *drows = reinterpret_cast<int32_t *>(ws + L.rows);
    const size_t rbytes = (size_t)r * sizeof(int32_t);
    char *prow = pin_take(ctx, rbytes);
    if (prow) {
        std::memcpy(prow, rows.data(), rbytes);
        MRBF_HIP(ctx, hipMemcpyAsync(drows, prow, rbytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        MRBF_HIP(ctx, hipMemcpy(drows, rows.data(), rbytes, hipMemcpyHostToDevice));
    }
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    for (const auto &c : chunks) {
        double *dst = out_dev ? hess_out : stage;
        MRBF_TRY(launch_points(ctx, M, c.second, Xd + c.first * d, drows, r, ns, per, ws + L.part, dst));
        if (!out_dev)
            MRBF_HIP(ctx, hipMemcpyAsync(hess_out + (size_t)c.first * point, stage, (size_t)c.second * point * sizeof(double),
                                         hipMemcpyDeviceToHost, ctx->stream));
    }
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    if (info) {
        MRBF_HIP(ctx, hipEventElapsedTime(&info->ms_total, ctx->ev[0], ctx->ev[1]));
        info->nsplit = ns;
        info->chunks = (int32_t)chunks.size();
    }
    return MRBF_OK;
}

// mrbf_eval_hessian_batch behind the context and job-count checks (api.hip): validate every job, then chunk by chunk one upload, the
// launches of hess_batch_host.hpp's tables, one read-back, one synchronisation.  DESIGN.md section 20.
int hess_batch_call(mrbf_ctx *ctx, int64_t n_jobs, mrbf_hess_job *jobs, mrbf_hess_batch_info *info, int64_t limit_bytes) {
    if (!jobs) return fail(ctx, -3, "mrbf_eval_hessian_batch: jobs is NULL");
    (void)hipSetDevice(ctx->device);
    std::vector<hessbatch::Job> shape((size_t)n_jobs);
    for (int64_t i = 0; i < n_jobs; ++i) {
        const mrbf_hess_job &J = jobs[i];
        hessbatch::Job &S = shape[(size_t)i];
        S.has_model = J.model != nullptr, S.m = J.m;
        S.X = J.X != nullptr, S.out = J.hess_out != nullptr;
        S.n_rows = J.n_rows, S.rows = J.rows;
        if (!J.model) continue;
        S.foreign = J.model->owner != ctx;
        S.n = J.model->n, S.d = J.model->d, S.k = J.model->k;
        S.variant = variant_of(J.model->kp);
    }
    std::vector<int32_t> status((size_t)n_jobs, 0);
    int64_t bad = 0;
    if (const int rc = hessbatch::validate(shape.data(), n_jobs, status.data(), &bad)) {
        if (rc == -3)  // every job's own status: mrbf_eval_hessian's argument checks
            for (int64_t i = 0; i < n_jobs; ++i) jobs[i].status = status[(size_t)i], jobs[i].nsplit = 0;
        return fail(ctx, rc, rc == -3 ? "mrbf_eval_hessian_batch: job %lld is invalid (its status says how)"
                                      : "mrbf_eval_hessian_batch: the model of job %lld belongs to another context", (long long)bad);
    }
    std::vector<size_t> need((size_t)n_jobs, 0);
    for (int64_t i = 0; i < n_jobs; ++i) {
        hessbatch::Job &S = shape[(size_t)i];
        jobs[i].status = 0, jobs[i].nsplit = 0;
        if (!hessbatch::active(S)) continue;
        S.X_dev = is_device_ptr(jobs[i].X), S.out_dev = is_device_ptr(jobs[i].hess_out);
        jobs[i].nsplit = hessbatch::split(S);
        need[(size_t)i] = hessbatch::need_doubles(S, DESC_DOUBLES);
    }
    const size_t limit = limit_bytes > 0 ? (size_t)limit_bytes : hessbatch::ARENA_LIMIT_BYTES;
    float ms = 0.f;
    int rounds = 0, groups = 0, single_inside = 0;
    for (const hessbatch::Chunk &c : hessbatch::chunks(need, limit)) {
        bool any = false;
        for (int64_t i = c.first; i < c.first + c.count; ++i) any = any || hessbatch::active(shape[(size_t)i]);
        if (!any) continue;
        ++rounds;
        if (c.single) {  // beyond the limit on its own: the single call's chain, with its own staging rule
            const mrbf_hess_job &J = jobs[c.first];
            hess::Call one;
            one.k = J.model->k, one.n_rows = J.n_rows, one.rows = J.rows;
            mrbf_hess_info hi;
            std::memset(&hi, 0, sizeof(hi));
            MRBF_TRY(hess_call(ctx, J.model, J.m, J.X, hess::row_list(one), J.hess_out, &hi, 0));
            ms += hi.ms_total, ++single_inside;
        } else {
            MRBF_TRY(run_batch_chunk(ctx, jobs, shape.data(), c.first, c.count, &ms, &groups));
        }
    }
    if (info) info->ms_total = ms, info->chunks = rounds, info->groups = groups, info->single_inside = single_inside;
    return MRBF_OK;
}

}  // namespace mrbf
