// Small problems on the LU path (n <= 512 sites, d <= 128, n >= q; the kernel's order exceeds what the tail covers, or a Cholesky gave
// up): the whole fit -- centring, the saddle matrix S = [Phi Pi; Pi' 0], LU with partial pivoting, both substitutions, the model's
// arrays -- in ONE launch, one workgroup of 256 threads per problem.  The counterpart of small.hip for the kernel / tail pairs the
// Cholesky paths do not take (thin plate spline k = 2 or cubic 5 with a linear tail, cubic 3 with a constant or no tail, multiquadric
// without a tail): solve.hip's fit_lu is a launch chain around rocSOLVER's getrf / getrs with two synchronisations per start, this is
// one grid for a batch of starts.  A single fit is a grid of one, so a batch and single calls run the same code on the same data and
// agree bit for bit.  No workgroup waits for another one: no clusters, no flags, no spins, no atomics; every reduction has a fixed
// order.  Opt-in (MRBF_OPT_SMALL_LU): with the option at 0 nothing here runs.
//
// The arithmetic is LAPACK's getrf: right-looking, blocked by 16 columns, the pivot of a column its entry of largest magnitude with
// ties to the smallest row (idamax).  S is column-major with N = n + q padded to N16, a multiple of 16 (ones on the padding diagonal);
// the right-hand sides [Y; 0] are 16 more columns of the same array, so that the row interchanges, U12 = inv(L11) A12 and the
// trailing update take them along and forward substitution needs no pass of its own.  Per panel:
//   1. the panel (rows c0 .., 16 columns) into LDS -- 656 x 16 doubles = 84 KB at most --, sixteen pivot searches + rank-1 updates
//      there (two barriers per column: thread t owns the rows t, t + 256, t + 512 in the search and in the update);
//   2. the panel back to memory, the NET permutation of its sixteen interchanges (at most 32 rows change) applied to every other
//      column -- all loads of a column before its stores -- and, in the same pass, U12 for the columns right of the panel;
//   3. A22 -= L21 U12 on the fp64 matrix cores (lu_trailing below: wg_gemm's tiling with the negated tile as the starting accumulator).
// A zero or non-finite pivot latches its 1-based column in flags[0] (getrf's info) and ends the problem's work; nothing of the model
// beyond Xc, sq and mean has been written then.  Back substitution runs block row by block row from the bottom: a 16 x 16 triangular
// solve by sixteen threads, then one product takes the block's contribution out of the rows above.
#include "small_dev.hpp"

#include <cfloat>

namespace mrbf {
namespace smalllu {

using namespace smallfit;

constexpr int NB = 16;    // panel width
constexpr int LDP = 656;  // rows of the LDS panel: round_up(512 + 129, 16)

__device__ __forceinline__ bool usable_pivot(double v) { return v != 0.0 && fabs(v) <= DBL_MAX; }  // (false for NaN as well)

// A22(i, j) -= sum_k L21(i, k) U12(k, j), k = 0 .. 15, for one workgroup of 4 waves (M, N multiples of 16; all three column-major, ld):
// wg_gemm's macro tiles and lane maps, with two differences that make the blocked factorisation cancel where the unblocked one does.
// The accumulator STARTS as the negated tile and the products are added to it in ascending k (MFMA step u takes k = 4 u + the lane
// group), so an element goes through  -a, -a + l_0 u_0, (-a + l_0 u_0) + l_1 u_1, ...: the mirror image of the fma chain that forms U12
// in the column pass (a - l_0 u_0 - l_1 u_1 ..., also ascending).  For two equal rows of S -- a duplicated site -- the row that is not
// taken as the pivot has multiplier 1 at the pivot's column and 0 behind it, its chain up to there is the pivot row's own, and the sum
// ends at exactly zero: the start meets a zero pivot and is reported singular, as by an unblocked getrf.  (With the tile subtracted
// from a sum that started at zero, in wg_gemm's k order, the two rows cancelled to rounding level only.)  All loads of a macro tile
// precede its stores; tiles are disjoint.
__device__ __forceinline__ void lu_trailing(int M, int N, const double *__restrict__ L21, const double *__restrict__ U12, double *__restrict__ A22, int ld) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int mt = M >> 4, nt = N >> 4, MT = (mt + 1) >> 1, NT2 = (nt + 1) >> 1;
    for (int idx = wave; idx < MT * NT2; idx += 4) {
        const int I = idx % MT, J = idx / MT;
        const int i0 = 32 * I, j0 = 32 * J;
        const bool va1 = 2 * I + 1 < mt, vb1 = 2 * J + 1 < nt;
        const int io[2] = {0, va1 ? 16 : 0}, jo[2] = {0, vb1 ? 16 : 0};  // (a missing second tile re-reads the first one and is not written)
        double fa[2][4], fb[2][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = 4 * u + l4;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fa[a][u] = gld(&L21[(i0 + io[a] + l15) + (int64_t)k * ld]);
                fb[a][u] = gld(&U12[k + (int64_t)(j0 + jo[a] + l15) * ld]);
            }
        }
        v4d acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[a][b][r] = -gld(&A22[(i0 + io[a] + l15) + (int64_t)(j0 + jo[b] + l4 + 4 * r) * ld]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[b][u], fa[a][u], acc[a][b], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if ((a == 1 && !va1) || (b == 1 && !vb1)) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) gst(&A22[(i0 + 16 * a + l15) + (int64_t)(j0 + 16 * b + l4 + 4 * r) * ld], -acc[a][b][r]);
            }
    }
}

__global__ __launch_bounds__(256) void small_lu_kernel(Prob one, const Prob *__restrict__ many, int count) {
    __shared__ __attribute__((aligned(16))) double panel[NB * LDP];  // [c * LDP + r]: consecutive rows on consecutive banks
    __shared__ double s_mean[128];
    __shared__ double s_rv[4];
    __shared__ int s_ri[4];
    __shared__ int s_piv[NB];                    // pivot row of column j, relative to the panel's first row
    __shared__ int s_rows[2 * NB], s_src[2 * NB], s_nrows;  // net permutation: the row s_rows[i] receives what the row s_src[i] held
    if ((int)blockIdx.x >= count) return;
    const Prob P = many ? many[blockIdx.x] : one;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n, d = P.d, k = P.k, q = P.q, np = P.npad, dpad = P.dpad;
    const int N = n + q, ld = (N + 15) & ~15;  // ld <= LDP (small_lu_applies)
    double *S = P.ws, *B = P.ws + (int64_t)ld * ld;  // B: ld x 16, the columns ld .. ld + 15 of the same array
    if (tid < 4) P.flags[tid] = 0;
    if (tid < 2) P.scal[tid] = 0.0;

    // ---- centroid, centred + zero-padded coordinates, squared norms: as the small fit does (small_dev.hpp)
    if (P.mean_given) {
        if (tid < 128) s_mean[tid] = tid < d ? gld(&P.mean[tid]) : 0.0;
    } else {
        column_means(P.C, n, d, panel, s_mean);
    }
    __syncthreads();
    if (!P.mean_given)
        for (int t = tid; t < dpad; t += 256) P.mean[t] = t < 128 ? s_mean[t] : 0.0;
    centre_sites(P, s_mean, 0, 1);

    // ---- everything of S outside the n x n kernel block: Pi = [1, x_1 .. x_d] of the sites as given (launch_poly_matrix) and its
    // transpose, the zero block, ones on the padding diagonal; the right-hand sides beside it
    for (int e = tid; e < ld * ld; e += 256) {
        const int i = e % ld, j = e / ld;
        if (i < n && j < n) continue;
        double v = 0.0;
        if (i < n && j < N)
            v = j == n ? 1.0 : gld(&P.C[(int64_t)i * d + (j - n - 1)]);
        else if (j < n && i < N)
            v = i == n ? 1.0 : gld(&P.C[(int64_t)j * d + (i - n - 1)]);
        else if (i == j && i >= N)
            v = 1.0;
        gst(&S[e], v);
    }
    for (int e = tid; e < ld * NB; e += 256) {
        const int i = e % ld, l = e / ld;
        gst(&B[e], (i < n && l < k) ? gld(&P.Y[(int64_t)i * k + l]) : 0.0);
    }
    __syncthreads();
    // ---- Phi = phi(|x_i - x_j|^2): GEMM form on the centred coordinates (squared distances first, the radial function as a pass of its own)
    // The squared norms are the product's OWN diagonal, not P.sq: two equal sites then have the same three numbers G_ii = G_jj = G_ij
    // bit for bit and a distance of exactly zero, so their rows of S are equal from the start (see lu_trailing).
    {
        const double *XcT = P.Xc;  // dpad x np column-major
        wg_gemm<true, false, false>(P.n16, P.n16, dpad, XcT, dpad, XcT, dpad, NoPre(), [&](int i, int j, double sdot, double) {
            if (i < n && j < n) gst(&S[(int64_t)j * ld + i], sdot);
        });
        __syncthreads();
        double *gd = panel;  // G_ii, i < n <= 512
        for (int i = tid; i < n; i += 256) gd[i] = gld(&S[(int64_t)i * ld + i]);
        __syncthreads();
        const KP kp = P.kp;
        for (int j0 = 8 * wave; j0 < n; j0 += 32)  // eight columns per wave and step: the loads of a step before its first store
            for (int i = lane; i < n; i += 64) {
                double t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = gld(&S[(int64_t)(j0 + u < n ? j0 + u : n - 1) * ld + i]);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (j0 + u < n) {
                        double v = fma(-2.0, t[u], gd[i] + gd[j0 + u]);
                        v = (v > 0.0 && i != j0 + u) ? v : 0.0;
                        gst(&S[(int64_t)(j0 + u) * ld + i], phi_rt(v, kp));
                    }
            }
    }
    __syncthreads();

    // ---- P S = L U, the right-hand sides riding along
    for (int c0 = 0; c0 < ld; c0 += NB) {
        const int m = ld - c0;  // rows of this panel
        for (int r = tid; r < m; r += 256) {
#pragma unroll
            for (int c = 0; c < NB; ++c) panel[c * LDP + r] = gld(&S[(c0 + r) + (int64_t)(c0 + c) * ld]);
        }
        __syncthreads();
        for (int j = 0; j < NB; ++j) {
            // pivot search over the rows j .. m - 1 of column j: largest magnitude, ties to the smallest row; a non-finite entry counts
            // as the largest of all, so that it is met as a pivot and latched
            double bv = -1.0;
            int bi = 0x7fffffff;
            for (int r = tid; r < m; r += 256) {
                if (r < j) continue;
                const double v = panel[j * LDP + r];
                const double a = fabs(v) <= DBL_MAX ? fabs(v) : HUGE_VAL;
                if (a > bv) {  // (rows ascending: the first of equals stays)
                    bv = a;
                    bi = r;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if (ov > bv || (ov == bv && oi < bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            if (lane == 0) {
                s_rv[wave] = bv;
                s_ri[wave] = bi;
            }
            __syncthreads();
            int pr = s_ri[0];
            {
                double pv = s_rv[0];
#pragma unroll
                for (int w = 1; w < 4; ++w)
                    if (s_rv[w] > pv || (s_rv[w] == pv && s_ri[w] < pr)) {
                        pv = s_rv[w];
                        pr = s_ri[w];
                    }
            }
            if (tid < NB && pr != j) {  // the interchange inside the panel (the other columns: below, all sixteen at once)
                const double a = panel[tid * LDP + j];
                panel[tid * LDP + j] = panel[tid * LDP + pr];
                panel[tid * LDP + pr] = a;
            }
            if (tid == 0) s_piv[j] = pr;
            __syncthreads();
            const double piv = panel[j * LDP + j];
            if (!usable_pivot(piv)) {  // uniform: every thread reads the same word
                if (tid == 0) P.flags[0] = c0 + j + 1;
                return;
            }
            for (int r = tid; r < m; r += 256) {
                if (r <= j) continue;
                const double l = panel[j * LDP + r] / piv;
                panel[j * LDP + r] = l;
                for (int c = j + 1; c < NB; ++c) panel[c * LDP + r] = fma(-l, panel[c * LDP + j], panel[c * LDP + r]);
            }
            // (no barrier here: the next search reads the rows this thread has just written; the interchange that touches other
            //  threads' rows sits behind the search's barrier)
        }
        __syncthreads();
        for (int r = tid; r < m; r += 256) {
#pragma unroll
            for (int c = 0; c < NB; ++c) gst(&S[(c0 + r) + (int64_t)(c0 + c) * ld], panel[c * LDP + r]);
        }
        if (tid == 0) {
            // the sixteen interchanges as one permutation of at most 32 rows: positions 0 .. 15 are the panel's own rows, the pivot rows
            // from further down follow; `cur` says whose content a position holds after the interchanges so far
            int nr = NB;
            for (int s = 0; s < NB; ++s) {
                s_rows[s] = c0 + s;
                s_src[s] = c0 + s;
            }
            for (int s = 0; s < NB; ++s) {
                const int g = c0 + s_piv[s];
                int at = -1;
                if (g < c0 + NB) {
                    at = g - c0;
                } else {
                    for (int i = NB; i < nr; ++i)
                        if (s_rows[i] == g) at = i;
                    if (at < 0) {
                        at = nr++;
                        s_rows[at] = g;
                        s_src[at] = g;
                    }
                }
                const int t = s_src[s];
                s_src[s] = s_src[at];
                s_src[at] = t;
            }
            s_nrows = nr;
        }
        __syncthreads();
        {
            const int nr = s_nrows;
            // every column but the panel's own (the factor's left part and the right-hand sides included): permute; right of the panel
            // also u = inv(L11) a for the rows of the panel (unit lower triangle, from LDS)
            for (int col0 = tid; col0 < ld; col0 += 256) {
                const int col = col0 < c0 ? col0 : col0 + NB;  // ld + 16 - 16 columns in all
                double *A = S + (int64_t)col * ld;
                double v[2 * NB];
#pragma unroll
                for (int i = 0; i < 2 * NB; ++i) v[i] = gld(&A[i < nr ? s_src[i] : s_src[0]]);
                if (col > c0) {
#pragma unroll
                    for (int i = 1; i < NB; ++i) {
#pragma unroll
                        for (int jj = 0; jj < i; ++jj) v[i] = fma(-panel[jj * LDP + i], v[jj], v[i]);
                    }
#pragma unroll
                    for (int i = 0; i < NB; ++i) gst(&A[c0 + i], v[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < NB; ++i)
                        if (s_src[i] != c0 + i) gst(&A[c0 + i], v[i]);
                }
#pragma unroll
                for (int i = NB; i < 2 * NB; ++i)
                    if (i < nr && s_src[i] != s_rows[i]) gst(&A[s_rows[i]], v[i]);
            }
        }
        __syncthreads();
        if (m > NB)
            lu_trailing(m - NB, m, S + (c0 + NB) + (int64_t)c0 * ld, S + c0 + (int64_t)(c0 + NB) * ld, S + (c0 + NB) + (int64_t)(c0 + NB) * ld, ld);
        __syncthreads();
    }

    // ---- U x = y: block rows from the bottom
    {
        double *su = panel;  // [i * 17 + j]: the 16 x 16 diagonal block of U
        for (int r0 = ld - NB; r0 >= 0; r0 -= NB) {
            su[(tid & 15) * 17 + (tid >> 4)] = gld(&S[(r0 + (tid & 15)) + (int64_t)(r0 + (tid >> 4)) * ld]);
            __syncthreads();
            if (tid < NB) {
                double *bl = B + r0 + (int64_t)tid * ld;
                double x[NB];
#pragma unroll
                for (int i = 0; i < NB; ++i) x[i] = gld(&bl[i]);
#pragma unroll
                for (int i = NB - 1; i >= 0; --i) {
                    double acc = x[i];
#pragma unroll
                    for (int jj = i + 1; jj < NB; ++jj) acc = fma(-su[i * 17 + jj], x[jj], acc);
                    x[i] = acc / su[i * 17 + i];
                }
#pragma unroll
                for (int i = 0; i < NB; ++i) gst(&bl[i], x[i]);
            }
            __syncthreads();
            if (r0 > 0)
                wg_gemm<false, false, false>(r0, NB, NB, S + (int64_t)r0 * ld, ld, B + r0, ld, [&](int i, int l) { return gld(&B[i + (int64_t)l * ld]); },
                                             [&](int i, int l, double v, double o) { gst(&B[i + (int64_t)l * ld], o - v); });
            __syncthreads();
        }
    }

    // ---- the model's arrays, in scatter_solution_kernel's layout: W (n x k row-major), Wc (npad x k column-major, zero padded), lam (q x k)
    for (int e = tid; e < np * k; e += 256) {
        const int i = e % np, l = e / np;
        const double v = i < n ? gld(&B[i + (int64_t)l * ld]) : 0.0;
        P.Wc[e] = v;
        if (i < n) P.W[(int64_t)i * k + l] = v;
    }
    for (int e = tid; e < q * k; e += 256) {
        const int t = e / k, l = e % k;
        P.lam[e] = gld(&B[n + t + (int64_t)l * ld]);
    }
}

}  // namespace smalllu

size_t small_lu_scratch_doubles(int64_t n, int q) {
    const size_t N16 = (size_t)round_up(n + q, 16);
    return N16 * N16 + 16 * N16;
}

bool small_lu_applies(const mrbf_ctx *ctx, int64_t n, int d, int k, int q, const KP &kp) {
    if (!ctx->small_lu || ctx->gram_mode != 0 || !(ctx->force_path == 0 || ctx->force_path == MRBF_PATH_LU)) return false;
    return n >= 1 && n <= 512 && d >= 1 && d <= 128 && k >= 1 && k <= 16 && n >= q && !kp_nonsmooth(kp);
}

int launch_small_lu(mrbf_ctx *ctx, const smallfit::Prob *host_probs, int count, const smallfit::Prob *dev_probs) {
    if (count <= 0) return 0;
    for (int i = 0; i < count; ++i)  // the LDS panel holds round_up(n + q, 16) <= 656 rows: nothing larger may reach the kernel
        if (round_up((int64_t)host_probs[i].n + host_probs[i].q, 16) > smalllu::LDP || host_probs[i].k > smalllu::NB)
            return fail(ctx, -3, "launch_small_lu: problem %d is outside the kernel's range", i);
    hipLaunchKernelGGL(smalllu::small_lu_kernel, dim3((unsigned)count), dim3(256), 0, ctx->stream, host_probs[0],
                       (count == 1 && !dev_probs) ? (const smallfit::Prob *)nullptr : dev_probs, count);
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace mrbf
