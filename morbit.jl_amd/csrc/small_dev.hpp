// Device-side pieces the one-launch kernels of a small problem share (small.hip: the Cholesky-path fit; small_lu.hip: the LU of the
// saddle system): global-address-space accessors, the elementwise pass, the workgroup GEMM on the fp64 matrix cores, the column means
// and the centring of the sites.  One definition each, so that the kernels -- and a batch and a single call of either -- run the same
// arithmetic on the same data.
#pragma once
#include "radial.hpp"
#include "small.hpp"

namespace mrbf {
namespace smallfit {

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double phi_rt(double s, const KP &p) {
    switch (p.kid) {
        case MRBF_CUBIC: return p.fast ? rbf_phi_t<MRBF_CUBIC, true>(s, p) : rbf_phi_t<MRBF_CUBIC, false>(s, p);
        case MRBF_INV_MULTIQUADRIC: return p.fast ? rbf_phi_t<MRBF_INV_MULTIQUADRIC, true>(s, p) : rbf_phi_t<MRBF_INV_MULTIQUADRIC, false>(s, p);
        case MRBF_MULTIQUADRIC: return p.fast ? rbf_phi_t<MRBF_MULTIQUADRIC, true>(s, p) : rbf_phi_t<MRBF_MULTIQUADRIC, false>(s, p);
        case MRBF_THIN_PLATE_SPLINE: return rbf_phi_t<MRBF_THIN_PLATE_SPLINE, false>(s, p);
        default: return rbf_phi_t<MRBF_GAUSSIAN, false>(s, p);
    }
}

// epilogue accesses through explicit global-address-space pointers: the workspace pointers come out of a struct, so the compiler
// would emit flat_ instructions (both counters, the LDS aperture check) for every element
typedef __attribute__((address_space(1))) double gdbl;
__device__ __forceinline__ void gst(double *p, double v) { *(gdbl *)p = v; }
__device__ __forceinline__ double gld(const double *p) { return *(const gdbl *)p; }

// elementwise pass over [0, count): f(e, loaded...) with the loads of eight elements per thread issued before the first store
template <class Load, class Store>
__device__ __forceinline__ void batched_pass(int count, Load load, Store store, int member = 0, int nc = 1) {
    for (int e0 = threadIdx.x + 8 * 256 * member; e0 < count; e0 += 8 * 256 * nc) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = load(e0 + 256 * u < count ? e0 + 256 * u : e0);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (e0 + 256 * u < count) store(e0 + 256 * u, t[u]);
    }
}

// C(i, j) (op)= sum_k A'(i, k) B'(k, j) for one workgroup of 4 waves; A' = TA ? A^T : A, B' = TB ? B^T : B (A, B column-major with
// leading dimensions lda, ldb); M, N multiples of 16, K a multiple of 4.  Every wave takes 32 x 32 macro tiles (2 x 2 MFMA tiles)
// round-robin; the epilogue is pre(i, j) -> what it reads, then post(i, j, value, what pre returned).  LOWER: only 16 x 16 tiles on or below the diagonal.
// f64 MFMA lane maps (tests/test_gpu_parity.py::test_f64_mfma_lane_maps): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
// D[row = (l >> 4) + 4 r][col = l & 15].
template <bool TA, bool TB, bool LOWER, class Pre, class Post>
__device__ __forceinline__ void wg_gemm(int M, int N, int K, const double *__restrict__ A, int lda, const double *__restrict__ B, int ldb, Pre pre,
                                        Post post, int member = 0, int nc = 1) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int mt = M >> 4, nt = N >> 4, MT = (mt + 1) >> 1, NT2 = (nt + 1) >> 1;
    for (int idx = wave + 4 * member; idx < MT * NT2; idx += 4 * nc) {  // macro tiles dealt over the waves of the cluster's workgroups
        const int I = idx % MT, J = idx / MT;
        if (LOWER && 2 * I + 1 < 2 * J) continue;
        const int i0 = 32 * I, j0 = 32 * J;
        const bool va1 = 2 * I + 1 < mt, vb1 = 2 * J + 1 < nt;
        v4d acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
        // (explicit global address space: global_load, not flat_load; no guards on the loads -- K is a multiple of 16 at every call
        //  site and a missing second tile re-reads the first one: as `cond ? load : 0` every operand load sat in its own exec-mask
        //  branch)
        typedef const __attribute__((address_space(1))) double gcd;
        // Within a group of 16 columns of K, MFMA step s takes k = 4 l4 + s from lane group l4 (any assignment works as long as both
        // operands use the same one): an operand that is contiguous in k then gives every lane 32 contiguous bytes per burst and the
        // four lane groups one whole 128-byte line per row.  (With k = 4 s + l4 every 8-byte load took its own 32 bytes out of a line
        // that three later loads fetched again from the L2: 128 KB of line traffic per burst and CU, ~1.1 us, the pace of every
        // product here.)
        typedef const __attribute__((address_space(1))) v4d gcv4 __attribute__((aligned(8)));
        gcd *pa = (gcd *)(TA ? A + 4 * l4 + (int64_t)(i0 + l15) * lda : A + (i0 + l15) + (int64_t)(4 * l4) * lda);
        gcd *pb = (gcd *)(TB ? B + (j0 + l15) + (int64_t)(4 * l4) * ldb : B + 4 * l4 + (int64_t)(j0 + l15) * ldb);
        const int64_t oa = va1 ? (TA ? 16 * (int64_t)lda : 16) : 0, ob = vb1 ? (TB ? 16 : 16 * (int64_t)ldb) : 0;
        // Bursts of UK = 4 k-steps (one group of 16 columns) kept in a ring of NR: a memory round trip costs ~1.5 us here (a problem's
        // working set does not stay in the L2 once a batch shares it), the MFMAs of a burst 0.1 us.
        constexpr int UK = 4, NR = 4;
        double fa0[NR][UK], fa1[NR][UK], fb0[NR][UK], fb1[NR][UK];
        auto burst = [&](int buf) {
            if constexpr (TA) {
                const v4d x0 = *(gcv4 *)pa, x1 = *(gcv4 *)(pa + oa);
#pragma unroll
                for (int u = 0; u < UK; ++u) {
                    fa0[buf][u] = x0[u];
                    fa1[buf][u] = x1[u];
                }
                pa += 16;
            } else {
#pragma unroll
                for (int u = 0; u < UK; ++u) {
                    fa0[buf][u] = pa[(int64_t)u * lda];
                    fa1[buf][u] = pa[(int64_t)u * lda + oa];
                }
                pa += 16 * (int64_t)lda;
            }
            if constexpr (!TB) {
                const v4d y0 = *(gcv4 *)pb, y1 = *(gcv4 *)(pb + ob);
#pragma unroll
                for (int u = 0; u < UK; ++u) {
                    fb0[buf][u] = y0[u];
                    fb1[buf][u] = y1[u];
                }
                pb += 16;
            } else {
#pragma unroll
                for (int u = 0; u < UK; ++u) {
                    fb0[buf][u] = pb[(int64_t)u * ldb];
                    fb1[buf][u] = pb[(int64_t)u * ldb + ob];
                }
                pb += 16 * (int64_t)ldb;
            }
        };
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (4 * UK * r < K) burst(r);
        for (int k0 = 0; k0 < K; k0 += 4 * UK * NR) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (k0 + 4 * UK * r < K) {
#pragma unroll
                    for (int u = 0; u < UK; ++u) {
                        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb0[r][u], fa0[r][u], acc[0][0], 0, 0, 0);
                        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb1[r][u], fa0[r][u], acc[0][1], 0, 0, 0);
                        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb0[r][u], fa1[r][u], acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb1[r][u], fa1[r][u], acc[1][1], 0, 0, 0);
                    }
                    if (k0 + 4 * UK * (r + NR) < K) burst(r);
                }
            }
        }
        // Epilogue in two passes: everything the epilogue READS for this macro tile first (pre: one burst of loads), then the stores
        // (post).  With a per-element read-modify-write the compiler must keep every load behind the previous element's store
        // (they may alias), and a 32 x 32 tile paid sixteen dependent memory round trips per lane: the Gram matrix of a 257-site
        // problem took 260 us whatever the dimension.  The products are formed transposed (B fragment as the MFMA's A operand), so
        // that the lane index runs along i, the contiguous index of every column-major output.
        double old[2][2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                // (no branch around the reads: a missing second tile reads the first one's operands again, a tile above the diagonal
                //  is read like any other and not written -- inside a branch every read waited for memory on its own)
                const int ia = i0 + ((a == 1 && va1) ? 16 : 0), jb = j0 + ((b == 1 && vb1) ? 16 : 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) old[a][b][r] = pre(ia + l15, jb + l4 + 4 * r);
            }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if ((a == 1 && !va1) || (b == 1 && !vb1)) continue;
                if (LOWER && 2 * I + a < 2 * J + b) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) post(i0 + 16 * a + l15, j0 + 16 * b + l4 + 4 * r, acc[a][b][r], old[a][b][r]);
            }
    }
}

struct NoPre {
    __device__ __forceinline__ double operator()(int, int) const { return 0.0; }
};

// column sums of the n x d sites -> s_mean[0 .. 127] (zero beyond d): wave w takes the rows w, w + 4, ..., eight rows (independent
// loads) per step, lanes over the columns; the four partial sums meet in LDS in a fixed order.  (One thread per column walking all n
// rows paid a memory round trip per row: 80 us of a 257-site fit.)  ONE function for the fit kernels and for small_mean_kernel: a
// batch (centroid computed up front) and a single fit agree bit for bit.
__device__ __forceinline__ void column_means(const double *C, int n, int d, double *part /* 4 x 128 doubles of LDS */, double *s_mean) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const gdbl *Cg = (const gdbl *)C;
    double s0 = 0.0, s1 = 0.0;
    const int t0 = lane, t1 = lane + 64;
    for (int i0 = wave; i0 < n; i0 += 32) {
        double a0[8], a1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + 4 * u;
            a0[u] = (i < n && t0 < d) ? Cg[(int64_t)i * d + t0] : 0.0;
            a1[u] = (i < n && t1 < d) ? Cg[(int64_t)i * d + t1] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            s0 += a0[u];
            s1 += a1[u];
        }
    }
    part[wave * 128 + t0] = s0;
    part[wave * 128 + t1] = s1;
    __syncthreads();
    if (tid < 128) s_mean[tid] = tid < d ? ((part[tid] + part[128 + tid]) + (part[256 + tid] + part[384 + tid])) / (double)n : 0.0;
}

// centred + zero-padded coordinates Xc (np x dpad) and their squared norms sq (the model's own arrays: the evaluation uses them later);
// four rows per wave and step, dealt over the nc workgroups of a cluster.  The arithmetic of small_fit_kernel's own centring loop,
// statement for statement (that kernel keeps its loop inline: called from here its register allocation moved, and its allocation is
// part of what its figures were measured with).
__device__ __forceinline__ void centre_sites(const Prob &P, const double *s_mean, int member, int nc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = P.n, d = P.d, np = P.npad, dpad = P.dpad;
    const gdbl *Cg = (const gdbl *)P.C;
    gdbl *Xg = (gdbl *)P.Xc;
    for (int row0 = wave + 16 * member; row0 < np; row0 += 16 * nc) {  // four rows per wave and step
        double sacc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = row0 + 4 * u;
            double sr = 0.0;
            if (row < np) {
                for (int t = lane; t < dpad; t += 64) {
                    double v = 0.0;
                    if (row < n && t < d) v = Cg[(int64_t)row * d + t] - s_mean[t];
                    Xg[(int64_t)row * dpad + t] = v;
                    sr = fma(v, v, sr);
                }
            }
            sacc[u] = sr;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) sacc[u] += __shfl_xor(sacc[u], off);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (lane == 0 && row0 + 4 * u < np) P.sq[row0 + 4 * u] = sacc[u];
    }
}

}  // namespace smallfit
}  // namespace mrbf
