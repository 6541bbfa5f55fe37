// Round 4 of the training-site selection on the device, with factor reuse for the fit -- replaces _rbf_round4
// (/root/reference/src/models/RbfModel.jl:352-499, Givens helper src/utilities.jl:437-448) and, when the training set is exactly
// (start set + round-4 sites), the dense solve inside RBF.RBFInterpolationModel (RbfModel.jl:759-763) -- the reference's own TODO
// at RbfModel.jl:657-660.
//
// The reference tests candidate xi by  tau^2 = sigma - ||L^-1 v||^2 > (theta_pivot_cholesky^2)^2,  the last pivot of the Cholesky
// factorisation of Z' Phi Z when xi's null-space direction is appended to Z (Z empty at the start, RbfModel.jl:391), and keeps
// Q (by Givens rotations), Z, L, L^-1 and Phi up to date by re-concatenating dense matrices per accepted site.  The same
// quantity without Q, R, Z:  the null-space directions added this round are  w(v) = [-Pi0 G0^-1 P' v ; v]  (G0 = Pi0' Pi0, P the
// polynomial rows of the accepted sites), so with the kernel
//     kappa(xi, eta) = phi(xi, eta) - lam(xi)' phi(X0, eta) - phi(xi, X0) lam(eta) + lam(xi)' Phi00 lam(eta),   lam(xi) = Pi0 G0^-1 pi(xi)
// one has  w' Phi w = v' K v  and  w' w = v' H v,  H = I + P G0^-1 P',  hence
//     tau^2(xi | accepted) = s_K(xi) / s_H(xi),
// the ratio of the running Cholesky pivots of K = kappa(candidates, candidates) and of H when xi joins the accepted set.  That
// makes round 4 a blocked Cholesky factorisation of K in candidate order that SKIPS the columns whose pivot ratio fails the test.
// kappa is evaluated on demand, and the candidates are walked in blocks of 128: one workgroup takes the sequential decisions inside
// a block from its Schur complement w.r.t. the accepted sites (s_H from a q x q matrix updated by Sherman-Morrison), everything
// else runs on the whole device, and only ~2 us per candidate are sequential (d = 64, 10^4 candidates, 2080 accepted: 5.1 s for the
// one-workgroup walk of round 2, see profiles/).  The walk has two forms:
//   right-looking (wherever R = L_acc^-1 kappa(accepted, candidates) fits in memory): R is kept for every candidate ahead and
//     extended by the rows of each block's accepted sites (the library's own split-k product and substitution kernels, the far
//     columns on a second stream), and a block's complement is kappa(block, block) - R(:, block)' R(:, block);
//   left-looking (the memory fallback): per block kappa(accepted | block, block), the block's columns of R by a triangular solve
//     with the accepted factor and the complement by one GEMM (rocBLAS dtrsm + dgemm).
// The factor of the accepted block is exactly what the fit needs:
//     K_acc v = Y_acc - Lam_acc Y_0,   w_0 = -Lam_acc' v,   Pi0 lambda = Y_0 - Phi00 w_0 - Phi0a v        (start set unisolvent: N0 = q)
// so the fit costs two triangular solves instead of an n^3 / 3 factorisation.  Checked against an independent from-scratch
// restatement (oracle/sampling_oracle.py) in tests/test_sampling.py.
#include "radial.hpp"
#include "walk_kernel.hpp"

namespace mrbf {

int launch_cross_gram(mrbf_ctx *ctx, const double *X, int64_t m, const double *C, int64_t n, int d, const KP &kp, double *K);
int launch_poly_matrix(mrbf_ctx *ctx, const double *C, int64_t n, int d, int q, double *Pi, int64_t ldpi);
int build_model_shell(mrbf_ctx *ctx, int64_t n, int d, int k, const double *Cdev, int kid, double a, double b, int deg, mrbf_model **out);
void destroy_model(mrbf_ctx *ctx, mrbf_model *M);
int fit_check(mrbf_ctx *ctx, mrbf_model *M, const double *Y, mrbf_fit_info *info);

}  // namespace mrbf

struct mrbf_round4_state {
    int64_t n0 = 0, mc = 0;
    int d = 0, q = 0, deg = -1, kid = 0, nacc = 0, maxacc = 0;
    double a = 0, b = 0;
    void *block = nullptr;  // one device allocation carved into the arrays below
    double *C0 = nullptr, *Xc = nullptr;           // n0 x d, mc x d row-major
    double *Phi00 = nullptr, *P0c = nullptr;       // n0 x n0; phi(X0, candidates) n0 x mc column-major
    double *Pi0 = nullptr;                         // n0 x q column-major
    double *LamT = nullptr;                        // n0 x mc column-major: column j = lam(xi_j)
    double *LK = nullptr;                          // factor of the ACCEPTED block (maxacc x maxacc lower, ld maxacc)
    double *Prow = nullptr, *Ginv = nullptr;       // mc x q row-major polynomial rows; q x q
    int *acc = nullptr;                            // accepted candidate positions, acceptance order; acc[maxacc] = count
};

namespace mrbf {
namespace r4 {
constexpr int KSPLIT_MAX_R4 = 8;  // most k slices of the right-looking update's product (sizes Ppart and the memory estimate)

// Prow[i*q + t] = [1, x_i][t]
__global__ void poly_rows_kernel(const double *__restrict__ X, int64_t m, int d, int q, double *__restrict__ P) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * q) return;
    const int64_t i = idx / q;
    const int t = (int)(idx % q);
    P[idx] = (t == 0) ? 1.0 : X[i * d + (t - 1)];
}
__global__ void identity_kernel(double *__restrict__ A, int q) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < q * q) A[idx] = (idx % q == idx / q) ? 1.0 : 0.0;
}

// ---- blocked walk: per block of SB candidates --------------------------------------------------------------------------------
// (SB = 128, the block of candidates decided inside one kernel: walk_kernel.hpp)
// Round 5: kappa on demand.  Rounds 3 / 4 built K = kappa(candidates, candidates) for ALL mc candidates up front (a cross-Gram block, two
// mc x mc x n0 products, a pass over four mc x mc matrices: 4.3 of the 21 ms of a call with 10^4 candidates at d = 64, and 3.2 GB of
// buffers) although the walk only ever reads the columns of the current block at the rows (accepted so far | the block itself), and
// stops after 17 of the 79 blocks once max_points is reached.  Here one launch per block evaluates exactly those entries:
//   kappa(xi, eta) = phi(|xi - eta|) - lam(xi).p(eta) - lam(eta).p(xi) + (lam(xi).f(eta) + lam(eta).f(xi)) / 2
// with lam = LamT[:, .] (n0), p = P0c[:, .] = phi(X0, .), f = F[:, .] = Phi00 lam(.) (symmetrised in the tail terms).
// rows rr < nacc: accepted site acc[rr] -> Kab[rr + j ld]; rows nacc + r: candidate i0 + r -> S[r + j SB].  64 x 64 tiles, 4 x 4 per thread
// (the shape of cross_gram_kernel: difference-form distances, then the four n0-term sums).
// Wide k chunks (64 coordinates, 32 tail terms per round, every load of a round in flight at once): with 16-wide rounds the kernel was a
// chain of 9 (d = 64) to 17 (d = 128) load -> barrier -> sum round trips, 67 to 85 us whatever the size of the grid.  The sums run over k in
// the same order as before.
template <int KID, int TL>  // tile = 16 rows x 64 columns, 4 entries per thread; TL = 0: distances only (a third of the LDS: the tail goes through the product kernel)
__global__ __launch_bounds__(256) void kappa_block_kernel(const double *__restrict__ Xc, int d, const double *__restrict__ LamT,
                                                          const double *__restrict__ P0c, const double *__restrict__ F, int n0, int have_tail,
                                                          const int *__restrict__ acc, int nacc, int64_t i0, int b, KP kp,
                                                          double *__restrict__ Kab, int ld, double *__restrict__ S, int blockrows,
                                                          int64_t batch_total = 0, int64_t rbase = -1, int rcount = 0) {
    if (batch_total > 0) {  // blockIdx.z = block number: kappa(block, block) of every block of the walk in one launch (S: SB x SB per block)
        const int64_t off = (int64_t)blockIdx.z * SB;
        i0 += off;
        b = (int)min((int64_t)SB, batch_total - off);
        S += off * SB;
    }
    constexpr int TR = 16, NR = TR + 64, KD = 64, KT = 32;
    __shared__ double sm[TL ? 3 * NR * (KT + 1) : NR * (KD + 1)];  // distance rounds: A[NR][KD + 1]; tail rounds: L | P | F, each [NR][KT + 1]
    static_assert(NR * (KD + 1) <= 3 * NR * (KT + 1), "the distance tile fits the tail tiles' area");
    __shared__ int64_t rid[NR];  // global site of a tile row (0 .. TR-1) / column (TR ..), -1 outside
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int R0 = blockIdx.y * TR, C0 = blockIdx.x * 64;
    const int nrows = nacc + (rbase >= 0 ? rcount : (blockrows ? b : 0));  // (blockrows = 0: the listed rows only, any number of columns; rbase: rcount rows of another block)
    if (tid < TR) {
        const int rr = R0 + tid;
        rid[tid] = rr < nacc ? (int64_t)acc[rr] : (rr < nrows ? (rbase >= 0 ? rbase : i0) + (rr - nacc) : -1);  // (rbase: block rows from another block)
    } else if (tid < NR) {
        const int c = C0 + tid - TR;
        rid[tid] = c < b ? i0 + c : -1;
    }
    __syncthreads();
    double dist[4] = {}, e1[4] = {}, e2[4] = {}, q1[4] = {}, q2[4] = {};
    for (int k0 = 0; k0 < d; k0 += KD) {
        double(*A)[KD + 1] = reinterpret_cast<double(*)[KD + 1]>(sm);
        double t[NR * KD / 256];
#pragma unroll
        for (int it = 0; it < NR * KD / 256; ++it) {
            const int e = tid + 256 * it, r = e / KD, c = e % KD;
            const int64_t gr = rid[r];
            t[it] = (gr >= 0 && k0 + c < d) ? Xc[gr * d + k0 + c] : 0.0;
        }
#pragma unroll
        for (int it = 0; it < NR * KD / 256; ++it) {
            const int e = tid + 256 * it;
            A[e / KD][e % KD] = t[it];
        }
        __syncthreads();
        const int kn = min(KD, d - k0);
#pragma unroll 8
        for (int kk = 0; kk < kn; ++kk) {
            const double av = A[ty][kk];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const double df = av - A[TR + tx + 16 * v][kk];
                dist[v] = fma(df, df, dist[v]);
            }
        }
        __syncthreads();
    }
    if (TL && have_tail) {
        double(*Ls)[KT + 1] = reinterpret_cast<double(*)[KT + 1]>(sm);
        double(*Ps)[KT + 1] = Ls + NR;
        double(*Fs)[KT + 1] = Ps + NR;
        for (int k0 = 0; k0 < n0; k0 += KT) {
            double tl[NR * KT / 256], tp[NR * KT / 256], tf[NR * KT / 256];
#pragma unroll
            for (int it = 0; it < NR * KT / 256; ++it) {
                const int e = tid + 256 * it, r = e / KT, c = e % KT;
                const int64_t gr = rid[r];
                const bool in = gr >= 0 && k0 + c < n0;
                const int64_t o = gr * n0 + k0 + c;
                tl[it] = in ? LamT[o] : 0.0;
                tp[it] = in ? P0c[o] : 0.0;
                tf[it] = in ? F[o] : 0.0;
            }
#pragma unroll
            for (int it = 0; it < NR * KT / 256; ++it) {
                const int e = tid + 256 * it, r = e / KT, c = e % KT;
                Ls[r][c] = tl[it];
                Ps[r][c] = tp[it];
                Fs[r][c] = tf[it];
            }
            __syncthreads();
            const int kn = min(KT, n0 - k0);
#pragma unroll 4
            for (int kk = 0; kk < kn; ++kk) {
                const double lr = Ls[ty][kk], pr = Ps[ty][kk], fr = Fs[ty][kk];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double lc = Ls[TR + tx + 16 * v][kk], pc = Ps[TR + tx + 16 * v][kk], fc = Fs[TR + tx + 16 * v][kk];
                    e1[v] = fma(lr, pc, e1[v]);
                    e2[v] = fma(lc, pr, e2[v]);
                    q1[v] = fma(lr, fc, q1[v]);
                    q2[v] = fma(lc, fr, q2[v]);
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int rr = R0 + ty, cc = C0 + tx + 16 * v;
        if (rr >= nrows || cc >= b) continue;
        double val = rbf_phi<KID>(dist[v], kp);
        if (TL && have_tail) val = (val - e1[v]) - e2[v] + 0.5 * (q1[v] + q2[v]);
        if (rr < nacc)
            Kab[rr + (int64_t)cc * ld] = val;
        else
            S[(rr - nacc) + cc * SB] = val;
    }
}

// the sequential decisions inside one block: S = Schur complement of the block w.r.t. the accepted sites (SB x SB, global -> LDS);
// cnt[0] = accepted so far (in / out), cnt[1] = accepted in this block (out); Lblk column a = in-block factor column of the a-th site
// accepted here (rows = in-block candidate index), blkidx[a] = its in-block index
constexpr int SEL_THREADS = 1024;
__global__ __launch_bounds__(SEL_THREADS) void select_block_kernel(const double *__restrict__ Sg, int b, int64_t i0, int n0, int q, int max_points,
                                                                   int maxacc, double thr, const double *__restrict__ Prow, double *__restrict__ Ginv,
                                                                   int *__restrict__ acc, int *__restrict__ cnt, double *__restrict__ Lblk,
                                                                   int *__restrict__ blkidx) {
    extern __shared__ double smem[];  // S[SB * SB] | cs[SB] | g[q] | pi[q] | red[SEL_THREADS / 64]
    double *S = smem, *cs = S + SB * SB, *g = cs + SB, *pi = g + (q > 0 ? q : 1), *red = pi + (q > 0 ? q : 1);
    __shared__ int s_acc;
    __shared__ double s_pk, s_ph;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < SB * SB; e += SEL_THREADS) S[e] = Sg[e];
    int nacc = cnt[0], nblk = 0;
    __syncthreads();
    for (int j = 0; j < b; ++j) {
        if (n0 + nacc >= max_points || nacc >= maxacc) break;
        __syncthreads();  // the previous candidate's decision words have been read by everybody
        // s_H = 1 + pi' Ginv pi
        if (q > 0) {
            for (int t = tid; t < q; t += SEL_THREADS) pi[t] = Prow[(i0 + j) * q + t];
            __syncthreads();
            double part = 0.0;
            for (int t = tid; t < q; t += SEL_THREADS) {
                double sdot = 0.0;
                for (int u = 0; u < q; ++u) sdot = fma(Ginv[t + (int64_t)u * q], pi[u], sdot);  // Ginv symmetric: column access is coalesced
                g[t] = sdot;
                part = fma(pi[t], sdot, part);
            }
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
            if (lane == 0) red[wave] = part;
            __syncthreads();
            if (tid == 0) {
                double sdot = 0.0;
                for (int w = 0; w < SEL_THREADS / 64; ++w) sdot += red[w];
                s_ph = 1.0 + sdot;
            }
        }
        if (tid == 0) {
            const double pk = S[j + j * SB];
            if (q == 0) s_ph = 1.0;
            s_pk = pk;
            const double tau2 = pk / s_ph;
            s_acc = (pk > 0.0 && tau2 > thr && tau2 < 1e300) ? 1 : 0;  // tau^2 > (theta^2)^2, RbfModel.jl:370, :452 (NaN fails)
        }
        __syncthreads();
        if (!s_acc) continue;
        const double pk = s_pk, ph = s_ph, rs = 1.0 / sqrt(pk);
        for (int r = tid; r < SB; r += SEL_THREADS) {
            const double c = (r > j && r < b) ? S[r + j * SB] * rs : (r == j ? pk * rs : 0.0);
            cs[r] = c;
            Lblk[r + nblk * SB] = c;
        }
        __syncthreads();
        for (int e = tid; e < SB * SB; e += SEL_THREADS) {  // rank-1 update of the trailing complement (lower part)
            const int r = e % SB, c = e / SB;
            if (c > j && r >= c && r < b) S[e] = fma(-cs[r], cs[c], S[e]);
        }
        // Ginv <- Ginv - g g' / s_H   (Sherman-Morrison for G + pi pi')
        if (q > 0)
            for (int e = tid; e < q * q; e += SEL_THREADS) Ginv[e] -= g[e % q] * g[e / q] / ph;
        if (tid == 0) {
            acc[nacc] = (int)(i0 + j);
            blkidx[nblk] = j;
        }
        ++nacc;
        ++nblk;
        __threadfence();
    }
    __syncthreads();
    if (tid == 0) {
        cnt[0] = nacc;
        cnt[1] = nblk;
        acc[maxacc] = nacc;
    }
}
// The same decisions with the inverse Gram matrix of the tail IN REGISTERS (the walk instantiates <3, 12, 16>: 145 <= q <= 192).  The
// kernel above is a chain of global-memory round trips per candidate -- pi from memory, 65 dependent column loads of Ginv for Ginv pi,
// the Sherman-Morrison update written back through memory behind a __threadfence, six workgroup barriers: 13.7 us per candidate, 30 of
// the 43 ms of a round 4 with 10^4 candidates at d = 64 (profiles/r04_round4_kernel_stats.csv) -- although the arithmetic per candidate
// is 4 q^2 + SB^2 flops.  Here
// thread (lane, wave) owns Ginv[t][u] for t = lane + 64 a, u = wave + 16 b (at most NA x NB_ entries), the product Ginv pi is formed as
// 16 partial sums per row through LDS, every thread takes the accept / reject decision itself from the same sums (same order: same
// result), the factor column is read off S's column j, pi of the next candidate is fetched one candidate ahead: three barriers and
// no global round trip per candidate.  Same arithmetic per entry as above except for the order of the q-term sums.
template <int NA, int NB_, int TW>  // TW waves: thread (lane, wave) owns Ginv[lane + 64 a][wave + TW bb]
__global__ __launch_bounds__(64 * TW) void select_block_reg_kernel(const double *__restrict__ Sg, int b, int64_t i0, int n0, int q,
                                                                       int max_points, int maxacc, double thr, const double *__restrict__ Prow,
                                                                       double *__restrict__ Ginv, int *__restrict__ acc, int *__restrict__ cnt,
                                                                       double *__restrict__ Lblk, int *__restrict__ blkidx) {
    // Round 5: the Schur complement S lives in REGISTERS as well -- thread tid owns column c = tid & 127, rows (tid >> 7) + 8 k, k = 0 .. 15.
    // With S in LDS the rank-1 update of an accepted candidate moved 32 bytes per entry of the whole 128 x 128 block through the LDS
    // (~1.8 us of the 4.7 us per candidate, LDS bandwidth); now the owners of column j publish it (128 values, double buffered) with
    // the candidate's pi and every thread updates its 16 entries from two broadcast reads each.
    extern __shared__ double smem[];  // colj[2][SB] | pi[q] | g[q] | part[TW * q] | red[TW]   (sized by the host for S[SB * SB] + ...: plenty)
    double *colj = smem, *pi = colj + 2 * SB, *g = pi + q, *part = g + q, *red = part + TW * q;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    static_assert(SB == 128 && (TW == 16 || TW == 8), "thread -> (row, column) map of the register copy of S");
    constexpr int TT = 64 * TW, RS = TT / 128, RK = 128 / RS;  // threads, row stride and rows per thread of the register copy of S
    const int sc = tid & 127, sr0 = tid >> 7;
    double Sr[RK];
#pragma unroll
    for (int k = 0; k < RK; ++k) Sr[k] = Sg[(sr0 + RS * k) + sc * SB];
    double G[NA][NB_];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int bb = 0; bb < NB_; ++bb) {
            const int t = lane + 64 * a, u = wave + TW * bb;
            G[a][bb] = (t < q && u < q) ? Ginv[t + (int64_t)u * q] : 0.0;
        }
    int nacc = cnt[0], nblk = 0;
    double pnext = (tid < q && b > 0) ? Prow[i0 * q + tid] : 0.0;
    __syncthreads();
    for (int j = 0; j < b; ++j) {
        if (n0 + nacc >= max_points || nacc >= maxacc) break;
        if (tid < q) pi[tid] = pnext;
        if (tid < q && j + 1 < b) pnext = Prow[(i0 + j + 1) * q + tid];  // in flight under this candidate's work
        double *cj = colj + (j & 1) * SB;  // (the previous candidate's column may still be read by a slow wave: two buffers)
        if (sc == j) {
#pragma unroll
            for (int k = 0; k < RK; ++k) cj[sr0 + RS * k] = Sr[k];
        }
        __syncthreads();
        // partial sums of Ginv pi over this wave's columns
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const int t = lane + 64 * a;
            double sp = 0.0;
#pragma unroll
            for (int bb = 0; bb < NB_; ++bb) {
                const int u = wave + TW * bb;
                if (u < q) sp = fma(G[a][bb], pi[u], sp);
            }
            if (t < q) part[wave * q + t] = sp;
        }
        __syncthreads();
        double pp = 0.0;
        if (tid < q) {
            double sg = 0.0;
#pragma unroll
            for (int w = 0; w < TW; ++w) sg += part[w * q + tid];
            g[tid] = sg;
            pp = pi[tid] * sg;
        }
        for (int off = 32; off > 0; off >>= 1) pp += __shfl_xor(pp, off);
        if (lane == 0) red[wave] = pp;
        __syncthreads();
        // every thread: the same sum in the same order (four interleaved chains instead of one of sixteen dependent additions)
        double p4[4] = {1.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int w = 0; w < TW; ++w) p4[w & 3] += red[w];
        const double ph = (p4[0] + p4[1]) + (p4[2] + p4[3]);
        const double pk = cj[j];
        const double tau2 = pk / ph;
        const bool accept = pk > 0.0 && tau2 > thr && tau2 < 1e300;  // tau^2 > (theta^2)^2, RbfModel.jl:370, :452 (NaN fails)
        if (!accept) continue;
        // 1 / sqrt(pk) and 1 / ph from the hardware estimates + Newton steps (relative error <= ~2e-16): the IEEE sqrt + two divisions
        // were ~150 dependent instructions on the critical path of every accepted candidate
        double sq_, rs;
        fast_sqrt_rsqrt(pk, sq_, rs);
        (void)sq_;
        for (int r = tid; r < SB; r += TT) Lblk[r + nblk * SB] = (r > j && r < b) ? cj[r] * rs : (r == j ? pk * rs : 0.0);
        if (sc > j) {  // rank-1 update of the trailing complement (lower part); column j is not touched
            const double lc = cj[sc] * rs;
#pragma unroll
            for (int k = 0; k < RK; ++k) {
                const int r = sr0 + RS * k;
                if (r >= sc && r < b) Sr[k] = fma(-(cj[r] * rs), lc, Sr[k]);
            }
        }
        // Ginv <- Ginv - g g' / s_H   (Sherman-Morrison for G + pi pi').  ONE reciprocal per candidate: g g' (1 / s_H) differs from
        // g g' / s_H in the last bit of an update that is itself O(eps) accurate -- the accept test keeps its exact quotient pk / s_H
        double rph = __builtin_amdgcn_rcp(ph);
        rph = fma(fma(-ph, rph, 1.0), rph, rph);
        rph = fma(fma(-ph, rph, 1.0), rph, rph);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const int t = lane + 64 * a;
            const double gt = t < q ? g[t] * rph : 0.0;
#pragma unroll
            for (int bb = 0; bb < NB_; ++bb) {
                const int u = wave + TW * bb;
                if (t < q && u < q) G[a][bb] = fma(-gt, g[u], G[a][bb]);
            }
        }
        if (tid == 0) {
            acc[nacc] = (int)(i0 + j);
            blkidx[nblk] = j;
        }
        ++nacc;
        ++nblk;
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int bb = 0; bb < NB_; ++bb) {
            const int t = lane + 64 * a, u = wave + TW * bb;
            if (t < q && u < q) Ginv[t + (int64_t)u * q] = G[a][bb];
        }
    if (tid == 0) {
        cnt[0] = nacc;
        cnt[1] = nblk;
        acc[maxacc] = nacc;
    }
}

// rows nacc0 .. nacc0 + nblk - 1 of the accepted factor: [ R(:, j_a)' | in-block factor entries | 0 ]
__global__ void append_rows_kernel(const double *__restrict__ R, int ldr, int nacc0, const double *__restrict__ Lblk, const int *__restrict__ blkidx,
                                   const int *__restrict__ cnt, double *__restrict__ L, int ldl) {
    const int nblk = cnt[1];
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int width = nacc0 + SB;
    if (idx >= (int64_t)SB * width) return;
    const int a = (int)(idx / width), c = (int)(idx % width);
    if (a >= nblk) return;
    const int jb = blkidx[a];
    double v = 0.0;
    if (c < nacc0)
        v = R[c + (int64_t)jb * ldr];
    else if (c - nacc0 <= a)
        v = Lblk[jb + (c - nacc0) * SB];
    else if (c - nacc0 >= nblk)
        return;
    L[(nacc0 + a) + (int64_t)c * ldl] = v;
}
// ---- right-looking form of the walk (round 5): R(:, j) = L_acc^-1 kappa(acc, j) is kept for EVERY candidate still ahead and extended by
// the rows of a block's accepted sites as soon as they are known, so that no block ever needs a triangular solve against the whole
// accepted factor (rocBLAS dtrsm: a chain of ~25 small launches per block, 4 of the 16.5 ms at d = 64 / 10^4 candidates and all of the
// 226 ms at d = 128 with 6000 accepted).  Per block:  Kn = kappa(new, ahead) - R(old, new)' R(old, ahead)  (one fat GEMM),
// R(new, ahead) = L_bb^-1 Kn  (a 128-row triangular solve) -- the blocked right-looking Cholesky with skipped
// columns that the walk is.  Same quantities as the left-looking form, summed in a different order.

// The tail part of kappa as a product: kappa(xi, eta) = phi - TA(:, xi)' TB(:, eta) with the stacked vectors
//   TA(:, s) = [lam_s; p_s; -lam_s / 2; -f_s / 2],  TB(:, s) = [p_s; lam_s; f_s; lam_s]   (4 n0 entries per site)
// so that the update of the far columns takes it as one more k slice of the product kernel (MFMA) instead of 4 n0 multiply-adds per
// entry in kappa_block_kernel, which was latency-bound at two workgroups per compute unit (92 us per block at d = 64, 25 without).
__global__ void tail_forms_kernel(const double *__restrict__ LamT, const double *__restrict__ P0c, const double *__restrict__ F, int n0, int64_t mc,
                                  double *__restrict__ TA, double *__restrict__ TB) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n0 * mc) return;
    const int k = (int)(idx % n0);
    const int64_t site = idx / n0, o = site * 4 * n0;
    const double l = LamT[idx], pv = P0c[idx], f = F[idx];
    TA[o + k] = l;
    TA[o + n0 + k] = pv;
    TA[o + 2 * n0 + k] = -0.5 * l;
    TA[o + 3 * n0 + k] = -0.5 * f;
    TB[o + k] = pv;
    TB[o + n0 + k] = l;
    TB[o + 2 * n0 + k] = f;
    TB[o + 3 * n0 + k] = l;
}

// ---- the right-looking walk's own kernels (round 5, second half): rocBLAS ran the fat product at ~6 TFLOP/s (m = 128: one workgroup per 64
// columns, no split over k) and the substitution took one thread per candidate (267 us per block).
// P[s](a, j) = sum over the k slice s of  A(k, a) B(k, j):  A = the new sites' columns of R (K x nblk), B = R(old rows, candidates
// ahead) (K x ncols); both operands are contiguous along k, so a lane fetches 32 contiguous bytes per 16-deep k group (k = 16 g + 4 (l >> 4)
// + s for MFMA step s: the same permutation on both sides).  Workgroup = 128 rows a x 64 columns j (wave w: 32 rows), grid (ncols / 64,
// ksplit); fragments double buffered in registers, no LDS.  lda, ldb multiples of 4 (32-byte aligned fragments).
__global__ __launch_bounds__(256, 2) void r4_tn_gemm_kernel(const double *__restrict__ A, int lda, const double *__restrict__ B, int64_t ldb, int K,
                                                            int64_t ncols, int kchunk, double *__restrict__ P, int64_t pstride,
                                                            const int *__restrict__ aidx = nullptr, int na = 0) {
    typedef double v4d __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    const int k0 = blockIdx.y * kchunk, k1 = min(K, k0 + kchunk);
    const double *ap[2], *bp[4];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        // (aidx: column a of the left operand is column aidx[a] of A -- the new sites' columns of R, read in place -- for a < na)
        const int a = 32 * wave + 16 * it + l15;
        const int64_t col = aidx ? (a < na ? aidx[a] : 0) : a;
        ap[it] = A + col * lda + 4 * l4;
    }
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        int64_t j = j0 + 16 * jt + l15;
        j = j < ncols ? j : ncols - 1;  // (a ragged last tile re-reads the last column; its results are not stored)
        bp[jt] = B + j * ldb + 4 * l4;
    }
    v4d acc[4][2];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int it = 0; it < 2; ++it) acc[jt][it] = (v4d){0.0, 0.0, 0.0, 0.0};
    auto load = [&](int k, v4d (&a)[2], v4d (&b)[4]) {  // one 16-deep group at k (k + 15 < K checked by the caller, or the masked tail below)
#pragma unroll
        for (int it = 0; it < 2; ++it) a[it] = *(const v4d *)(ap[it] + k);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) b[jt] = *(const v4d *)(bp[jt] + k);
    };
    auto mma = [&](const v4d (&a)[2], const v4d (&b)[4]) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int it = 0; it < 2; ++it) acc[jt][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[jt][s4], a[it][s4], acc[jt][it], 0, 0, 0);
    };
    v4d a0[2], b0[4], a1[2], b1[4];
    int k = k0;
    const int kfull = k0 + ((k1 - k0) & ~15);
    if (k < kfull) load(k, a0, b0);
    for (; k + 32 <= kfull; k += 32) {
        load(k + 16, a1, b1);
        mma(a0, b0);
        if (k + 32 < kfull) load(k + 32, a0, b0);
        mma(a1, b1);
    }
    if (k < kfull) {
        mma(a0, b0);
        k += 16;
    }
    if (k < k1) {  // the ragged end of the k range: element-wise guards (rows >= K of R are not written yet)
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int e = 0; e < 4; ++e) a0[it][e] = (k + 4 * l4 + e < k1) ? ap[it][k + e] : 0.0;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int e = 0; e < 4; ++e) b0[jt][e] = (k + 4 * l4 + e < k1) ? bp[jt][k + e] : 0.0;
        mma(a0, b0);
    }
    // D(row = j within the tile = (l >> 4) + 4 r, col = a = l & 15): consecutive lanes write consecutive a of one column j
    double *Ps = P + (int64_t)blockIdx.y * pstride;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t j = j0 + 16 * jt + l4 + 4 * r;
            if (j < ncols) {
#pragma unroll
                for (int it = 0; it < 2; ++it) Ps[(32 * wave + 16 * it + l15) + j * SB] = acc[jt][it][r];
            }
        }
}
// X = L_bb^-1 (Kn - sum_s P[s]) on the matrix cores (one thread per candidate took 267 us per block; four threads per candidate out of LDS
// 370 us, both latency-bound).  Workgroup = 64 candidates, one wave per 16.  L_bb is cut into 8 x 8 blocks of 16:
// X_s = inv(L_ss) (rhs_s - sum_{t < s} L_st X_t).  A block X_t in the f64 MFMA's C/D layout (row = (l >> 4) + 4 r, column = l & 15) IS the B
// operand of the k slice r of the next product, so the blocks never leave the registers; the A operands (-L_st, inv(L_ss)) come from LDS;
// the 16 x 16 inverses of the diagonal blocks are formed once per workgroup by forward substitution on the identity (rocBLAS's trsm
// inverts its diagonal blocks the same way).  Rows >= nblk of the padded system are identity rows with zero right-hand sides.  The
// right-hand sides (the k slices of the product summed in a fixed order: deterministic) are staged through LDS by all four waves with the
// lanes along a -- 32 independent loads in flight per thread and slice -- and the solution leaves through the same tile, coalesced.
constexpr int FWM_LDR = 132;  // row pitch of the right-hand-side tile: 4 j + (l >> 4) covers the 64 banks once per 16 x 4 lanes
constexpr size_t fwm_shm_bytes(int ncol) { return ((size_t)SB * (SB + 1) / 2 + (size_t)8 * 16 * 17 + (size_t)ncol * FWM_LDR) * sizeof(double) + SB * sizeof(int); }
template <int NCOL>  // candidates per workgroup: 64 (one wave per 16) or 16 (few columns: more workgroups, every load of a thread in flight at once)
__global__ __launch_bounds__(256) void block_forward_mfma_kernel(const double *__restrict__ Kn, const double *__restrict__ P, int ksplit, int64_t pstride,
                                                                const double *__restrict__ Lblk, const int *__restrict__ blkidx, int nblk, int64_t ncols,
                                                                double *__restrict__ Rout, int64_t ldr, int kn_by_idx = 0) {
    // (kn_by_idx: Kn holds kappa(every candidate of the block, .), row a of the system is its row blkidx[a])
    typedef double v4d __attribute__((ext_vector_type(4)));
    extern __shared__ double fwm_smem[];  // Lt[SB (SB + 1) / 2] | Iv[8][16][17] | Xt[NCOL][FWM_LDR] | bi[SB]
    double *Lt = fwm_smem, *Iv = Lt + SB * (SB + 1) / 2, *Xt = Iv + 8 * 16 * 17;
    int *bi = reinterpret_cast<int *>(Xt + NCOL * FWM_LDR);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int64_t jbase = (int64_t)blockIdx.x * NCOL;
    if (tid < SB) bi[tid] = tid < nblk ? blkidx[tid] : 0;
    __syncthreads();
    {  // L_bb(a, a') = Lblk[blkidx[a] + a' SB] (a' <= a < nblk), identity beyond nblk; thread -> row a (the accepted rows are near-contiguous)
        const int a = tid & 127;
        const double *src = Lblk + bi[a];
        double *dst = Lt + a * (a + 1) / 2;
        for (int a2 = tid >> 7; a2 <= a; a2 += 64) {  // 32 loads in flight (one at a time is an L2 round trip per element: 50 us)
            double t[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) t[u] = (a2 + 2 * u <= a && a < nblk) ? src[(a2 + 2 * u) * SB] : (a == a2 + 2 * u ? 1.0 : 0.0);
#pragma unroll
            for (int u = 0; u < 32; ++u)
                if (a2 + 2 * u <= a) dst[a2 + 2 * u] = t[u];
        }
    }
    {  // right-hand sides: thread -> row a, every second column; eight columns x eight slices of the product in flight per round, the
       // slices subtracted in their fixed order
        const int a = tid & 127, c0 = tid >> 7;
        const bool ain = a < nblk;
        const int ka = kn_by_idx ? bi[a] : a;
#pragma unroll 1
        for (int u0 = 0; u0 < NCOL / 2; u0 += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t j = jbase + c0 + 2 * (u0 + u);
                v[u] = (j < ncols && ain) ? Kn[ka + j * SB] : 0.0;
            }
#pragma unroll 1
            for (int s0 = 0; s0 < ksplit; s0 += 8) {
                double t[8][8];
#pragma unroll
                for (int s2 = 0; s2 < 8; ++s2)
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int64_t j = jbase + c0 + 2 * (u0 + u);
                        t[s2][u] = (s0 + s2 < ksplit && j < ncols && ain) ? P[(int64_t)(s0 + s2) * pstride + a + j * SB] : 0.0;
                    }
#pragma unroll
                for (int s2 = 0; s2 < 8; ++s2)
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] -= t[s2][u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) Xt[(c0 + 2 * (u0 + u)) * FWM_LDR + a] = v[u];
        }
    }
    __syncthreads();
    if (tid < SB) {  // inverses of the eight diagonal 16 x 16 blocks: thread -> (block, column)
        const int blk = tid >> 4, col = tid & 15;
        double x[16];
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            const int ga = 16 * blk + a;
            const double *Lrow = Lt + ga * (ga + 1) / 2 + 16 * blk;
            double acc = (a == col) ? 1.0 : 0.0;
#pragma unroll
            for (int a2 = 0; a2 < a; ++a2) acc = fma(-Lrow[a2], x[a2], acc);
            x[a] = acc / Lrow[a];
        }
#pragma unroll
        for (int a = 0; a < 16; ++a) Iv[(blk * 16 + a) * 17 + col] = x[a];  // inv(L_ss)(a, col)
    }
    __syncthreads();
    if (16 * wave < NCOL) {
        double *xcol = Xt + (16 * wave + l15) * FWM_LDR + l4;  // this lane's column; rows l4 + 4 r of a block
        v4d X[8];
#pragma unroll
        for (int sb = 0; sb < 8; ++sb) {
            v4d D;
#pragma unroll
            for (int r = 0; r < 4; ++r) D[r] = xcol[16 * sb + 4 * r];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (t < sb) {
                    const int ga = 16 * sb + l15;
                    const double *Lrow = Lt + ga * (ga + 1) / 2 + 16 * t + l4;
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) D = __builtin_amdgcn_mfma_f64_16x16x4f64(-Lrow[4 * r4], X[t][r4], D, 0, 0, 0);
                }
            }
            v4d Xs = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) Xs = __builtin_amdgcn_mfma_f64_16x16x4f64(Iv[(sb * 16 + l15) * 17 + 4 * r4 + l4], D[r4], Xs, 0, 0, 0);
            X[sb] = Xs;
#pragma unroll
            for (int r = 0; r < 4; ++r) xcol[16 * sb + 4 * r] = Xs[r];
        }
    }
    __syncthreads();
    {
        const int a = tid & 127, c0 = tid >> 7;
        if (a < nblk) {
#pragma unroll 8
            for (int u = 0; u < NCOL / 2; ++u) {
                const int64_t j = jbase + c0 + 2 * u;
                if (j < ncols) Rout[a + j * ldr] = Xt[(c0 + 2 * u) * FWM_LDR + a];
            }
        }
    }
}
// Sb = kappa(block, block) - sum of the k slices of R(:, block)' R(:, block), zero outside the block's b rows and columns (the decision
// kernel is one workgroup: it must not be the one to read 33 x 128 KB)
__global__ void schur_reduce_kernel(const double *__restrict__ Kbb, const double *__restrict__ Spart, int ksplit, int b, double *__restrict__ Sb) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= SB * SB) return;
    const int r = e % SB, c = e / SB;
    double x = Kbb[e];
    for (int s0 = 0; s0 < ksplit; s0 += 8) {
        double t[8];
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) t[s2] = (s0 + s2 < ksplit) ? Spart[(size_t)(s0 + s2) * SB * SB + e] : 0.0;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) x -= t[s2];
    }
    Sb[e] = (r < b && c < b) ? x : 0.0;
}

// Gp (SB x SB) = [G (q x q) 0; 0 I]
__global__ void pad_identity_kernel(const double *__restrict__ G, int q, double *__restrict__ Gp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= SB * SB) return;
    const int i = idx % SB, j = idx / SB;
    Gp[idx] = (i < q && j < q) ? G[i + j * q] : (i == j ? 1.0 : 0.0);
}

// dense j x j copy of the accepted factor
__global__ void copy_factor_kernel(const double *__restrict__ L, int ldl, int j, double *__restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= j * j) return;
    const int p = idx % j, a2 = idx / j;
    out[idx] = (p >= a2) ? L[p + (int64_t)a2 * ldl] : 0.0;
}

// gathers for the fit: LaT (n0 x j) = columns acc of LamT; P0a (n0 x j) = columns acc of P0c; Lacc (j x j lower) = rows acc of LK
__global__ void gather_cols_kernel(const double *__restrict__ src, int64_t rows, const int *__restrict__ acc, int j, double *__restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * j) return;
    const int64_t r = idx % rows;
    const int c = (int)(idx / rows);
    dst[idx] = src[r + (int64_t)acc[c] * rows];
}
__global__ void gather_factor_kernel(const double *__restrict__ LK, int64_t mc, const int *__restrict__ acc, int j, double *__restrict__ L) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= j * j) return;
    const int p = idx % j, a2 = idx / j;
    L[idx] = (p >= a2) ? LK[acc[p] + (int64_t)a2 * mc] : 0.0;
}
// values (n0 + j) x k row-major -> Y0 (n0 x k), Ya (j x k) column-major
__global__ void split_values_kernel(const double *__restrict__ Y, int n0, int j, int k, double *__restrict__ Y0, double *__restrict__ Ya) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (n0 + j) * k) return;
    const int i = idx / k, l = idx % k;
    if (i < n0)
        Y0[i + l * n0] = Y[idx];
    else
        Ya[(i - n0) + l * j] = Y[idx];
}
// W row-major (n0 + j) x k and Wc (npad x k column-major, zero padded) from w0 (n0 x k), v (j x k) column-major; lam (q x k row-major) from lamc
__global__ void pack_solution_kernel(const double *__restrict__ w0, const double *__restrict__ v, const double *__restrict__ lamc, int n0, int j,
                                     int k, int q, int64_t npad, double *__restrict__ W, double *__restrict__ Wc, double *__restrict__ lam) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < npad * k) {
        const int64_t i = idx % npad;
        const int l = (int)(idx / npad);
        const double val = (i < n0) ? w0[i + (int64_t)l * n0] : ((i < n0 + j) ? v[(i - n0) + (int64_t)l * j] : 0.0);
        Wc[idx] = val;
        if (i < n0 + j) W[i * k + l] = val;
    } else if (idx < npad * k + (int64_t)q * k) {
        const int64_t e = idx - npad * k;
        const int t = (int)(e % q), l = (int)(e / q);
        lam[(int64_t)t * k + l] = lamc[t + (int64_t)l * q];
    }
}
__global__ void concat_sites_kernel(const double *__restrict__ C0, const double *__restrict__ Xc, const int *__restrict__ acc, int n0, int j, int d,
                                    double *__restrict__ S) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (n0 + j) * d) return;
    const int i = idx / d, t = idx % d;
    S[idx] = (i < n0) ? C0[idx] : Xc[(int64_t)acc[i - n0] * d + t];
}

static inline unsigned nb(int64_t c) { return (unsigned)((c + 255) / 256); }

}  // namespace r4
}  // namespace mrbf

using namespace mrbf;

extern "C" int32_t mrbf_free_round4(mrbf_ctx *ctx, mrbf_round4_state *st) {
    if (!ctx) return -1;
    if (!st) return MRBF_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (st->block) (void)hipFree(st->block);
    delete st;
    --ctx->live_round4;
    return MRBF_OK;
}

extern "C" int32_t mrbf_round4(mrbf_ctx *ctx, int64_t n0, int32_t d, const double *start_sites, int64_t mc, const double *cand_sites,
                               int32_t kernel_id, double a, double b, int32_t poly_deg, int32_t max_points, double theta_pivot_cholesky,
                               int32_t *accepted_out, int32_t *n_accepted, mrbf_round4_state **state_out) {
    using namespace r4;
    if (!ctx) return -1;
    if (n0 < 1 || n0 > 8192) return fail(ctx, -2, "n0 = %lld out of range", (long long)n0);
    if (d < 1 || d > 1024) return fail(ctx, -3, "d = %d out of range", d);
    if (!start_sites) return fail(ctx, -4, "start_sites is NULL");
    if (mc < 0 || mc > 30000) return fail(ctx, -5, "mc = %lld out of range", (long long)mc);
    if (mc > 0 && !cand_sites) return fail(ctx, -6, "cand_sites is NULL");
    if (kernel_id < 0 || kernel_id > 4) return fail(ctx, -7, "kernel_id out of range");
    if (poly_deg < -1 || poly_deg > 1) return fail(ctx, -10, "polynomial_degree must be -1, 0 or 1");
    if (!n_accepted) return fail(ctx, -14, "n_accepted is NULL");
    if (state_out) *state_out = nullptr;
    *n_accepted = 0;
    (void)hipSetDevice(ctx->device);
    const int q = poly_dim(d, poly_deg);
    if (max_points <= 0) max_points = (d + 1) * (d + 2) / 2;  // RbfModel.jl:356
    if (n0 < q)
        return fail(ctx, -2, "round 4 on the device needs a start set that carries the polynomial tail (n0 = %lld < q = %d): use the host mirror",
                    (long long)n0, q);
    if (mc == 0 || n0 >= max_points) return MRBF_OK;  // nothing to select (RbfModel.jl:368)
    const int maxacc = (int)std::min<int64_t>(mc, (int64_t)max_points - n0);
    // one allocation for everything that outlives the call
    auto *st = new mrbf_round4_state();
    st->n0 = n0; st->mc = mc; st->d = d; st->q = q; st->deg = poly_deg; st->kid = kernel_id; st->a = a; st->b = b; st->maxacc = maxacc;
    const size_t cnt[9] = {(size_t)n0 * d, (size_t)mc * d, (size_t)n0 * n0, (size_t)n0 * mc, (size_t)n0 * std::max(q, 1), (size_t)n0 * mc,
                           (size_t)maxacc * maxacc, (size_t)mc * std::max(q, 1), (size_t)std::max(q, 1) * std::max(q, 1)};
    size_t off[10];
    off[0] = 0;
    for (int i = 0; i < 9; ++i) off[i + 1] = off[i] + ((cnt[i] * sizeof(double) + 255) & ~size_t(255));
    const size_t total = off[9] + ((size_t)(maxacc + 1) * sizeof(int) + 255);
    if (hipMalloc(&st->block, total) != hipSuccess) {
        delete st;
        return fail(ctx, MRBF_ENOMEM, "round 4 state allocation of %zu bytes failed", total);
    }
    char *base = (char *)st->block;
    st->C0 = (double *)(base + off[0]); st->Xc = (double *)(base + off[1]); st->Phi00 = (double *)(base + off[2]);
    st->P0c = (double *)(base + off[3]); st->Pi0 = (double *)(base + off[4]); st->LamT = (double *)(base + off[5]);
    st->LK = (double *)(base + off[6]); st->Prow = (double *)(base + off[7]); st->Ginv = (double *)(base + off[8]); st->acc = (int *)(base + off[9]);
    auto run = [&]() -> int {
        const KP kp = make_kp(kernel_id, a, b);
        const double one = 1.0, zero = 0.0;
        hipStream_t s = ctx->stream;
        MRBF_HIP(ctx, hipMemcpyAsync(st->C0, start_sites, (size_t)n0 * d * sizeof(double), hipMemcpyDefault, s));
        MRBF_HIP(ctx, hipMemcpyAsync(st->Xc, cand_sites, (size_t)mc * d * sizeof(double), hipMemcpyDefault, s));
        // kernel blocks (difference-form arithmetic, like norm(x - c)): Phi00, phi(candidates, X0) (= P0c as n0 x mc column-major)
        double *F = nullptr, *T;
        MRBF_TRY(launch_cross_gram(ctx, st->C0, n0, st->C0, n0, d, kp, st->Phi00));
        MRBF_TRY(launch_cross_gram(ctx, st->Xc, mc, st->C0, n0, d, kp, st->P0c));
        int *dinfo = nullptr;  // info word of the start set's factorisation (read with the first block's counts)
        if (q > 0) {
            MRBF_TRY(get_buf(ctx, S_W1, (size_t)n0 * mc, &F));
            MRBF_TRY(get_buf(ctx, S_T1, (size_t)q * std::max<int64_t>(mc, q), &T));
            MRBF_TRY(get_buf(ctx, S_INFO, (size_t)4, &dinfo));
            MRBF_TRY(launch_poly_matrix(ctx, st->C0, n0, d, q, st->Pi0, n0));
            hipLaunchKernelGGL(poly_rows_kernel, dim3(nb(mc * q)), dim3(256), 0, s, st->Xc, mc, d, q, st->Prow);
            // G0 = Pi0' Pi0 (q x q), its Cholesky factor, Ginv = G0^-1, T = G0^-1 P' (q x mc), LamT = Pi0 T (n0 x mc)
            double *G0;
            MRBF_TRY(get_buf(ctx, S_G, (size_t)q * q, &G0));
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_transpose, rocblas_operation_none, q, q, (int)n0, &one, st->Pi0, (int)n0,
                                         st->Pi0, (int)n0, &zero, G0, q));
            // (the factorisation's info word is read with the first block's counts -- no host round trip of its own; a rank-deficient start
            // set fills the walk with NaNs, which accept nothing, and the call then returns MRBF_ESINGULAR)
            if (q <= SB) {
                // q <= 128: the library's own diagonal-block kernel on G0 padded with the identity -- factor and inverse of the factor in one
                // launch -- and G0^-1 = inv(L)' inv(L)  (rocSOLVER: potf2 59 us + two substitution launches on the identity 94 us)
                double *Gp, *Li;
                MRBF_TRY(get_buf(ctx, S_R, (size_t)SB * SB, &Gp));
                MRBF_TRY(get_buf(ctx, S_PI, (size_t)SB * SB, &Li));
                hipLaunchKernelGGL(pad_identity_kernel, dim3(nb(SB * SB)), dim3(256), 0, s, G0, q, Gp);
                MRBF_TRY(potrf_blocked_tall(ctx, SB, SB, Gp, SB, dinfo, Li));
                MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_transpose, rocblas_operation_none, q, q, q, &one, Li, SB, Li, SB, &zero, st->Ginv, q));
            } else {
                MRBF_BLAS(ctx, rocsolver_dpotrf(ctx->blas, rocblas_fill_lower, q, G0, q, dinfo));
                hipLaunchKernelGGL(identity_kernel, dim3(nb(q * q)), dim3(256), 0, s, st->Ginv, q);
                MRBF_BLAS(ctx, rocsolver_dpotrs(ctx->blas, rocblas_fill_lower, q, q, G0, q, st->Ginv, q));
            }
            // T = G0^-1 P' as a product with the inverse the decision kernel starts from anyway (rocSOLVER's potrs on mc right-hand sides
            // is a chain of ~ mc / 640 substitution + GEMM launches: 0.2 ms at mc = 10^4); Prow (mc x q row-major) is P' (q x mc) column-major
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, q, (int)mc, q, &one, st->Ginv, q, st->Prow, q, &zero, T,
                                         q));
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, (int)n0, (int)mc, q, &one, st->Pi0, (int)n0, T, q,
                                         &zero, st->LamT, (int)n0));
            // F = Phi00 LamT (n0 x mc): with lam and p = phi(X0, .) all the tail of kappa needs (kappa_block_kernel, tail_forms_kernel)
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, (int)n0, (int)mc, (int)n0, &one, st->Phi00, (int)n0,
                                         st->LamT, (int)n0, &zero, F, (int)n0));
        }
        const double thr = (theta_pivot_cholesky * theta_pivot_cholesky) * (theta_pivot_cholesky * theta_pivot_cholesky);
        // The decision kernel, by q.  q <= 80: the two halves of a step on different waves (select_block_duo_kernel: same bits; 119 against
        // 140 us per block at q = 65).  q <= 144: the one-barrier walk with every wave doing both halves -- beyond q = 80 the G waves' share
        // (2 q^2 / 256 entries per thread + q / 16 row sums) outweighs the S waves' -- and beyond q = 144 its <8, 6, 12> shape spills.
        // q <= 192: the register kernel, three rows x twelve columns of Ginv per thread.  q = 0 and q > 192: S and Ginv through memory.
        // The walk kernels ask for (nearly) the whole LDS of their compute unit: no workgroup of the side stream's kappa / substitution
        // kernels then fits beside them (sharing the unit's VALUs cost the one sequential kernel of the walk 40 us per block).
        constexpr size_t R4_SEL_LDS = 152 * 1024;
        auto walk_lds = [&](int nbw) { return std::max<size_t>((size_t)SB * 16 * nbw * sizeof(double), R4_SEL_LDS); };
        const size_t shm = ((size_t)SB * SB + SB + 2 * (size_t)std::max(q, 1) + SEL_THREADS / 64) * sizeof(double);
        const size_t shm_reg = ((size_t)SB * SB + 2 * (size_t)std::max(q, 1) + 16 * (size_t)std::max(q, 1) + 16) * sizeof(double);
        // The right-looking walk (see block_forward_mfma_kernel) wherever R for every candidate fits: with its own product and substitution
        // kernels and the far columns' update on a second stream it wins at every shape measured (d = 64, 2080 of 10^4 accepted, where the
        // walk stops after 17 of 79 blocks and most of R(:, ahead) is never used, as well as d = 128, 6000 of 6000).
        //  it keeps R for every candidate plus (KSPLIT_MAX + 2) 128-row panels over all candidates in the context's pool for the
        // life of the process: only while that is at most 2 GB of R and all of it fits into half of the card's free memory -- beyond, the
        // left-looking walk (maxacc x 128 per block) does the same walk.  MRBF_R4_EAGER=0 forces the left-looking walk (read per call: the
        // tests switch it).
        const char *eager_env = mrbf_env("MRBF_R4_EAGER");
        bool eager = !(eager_env && atoi(eager_env) == 0) && (int64_t)round_up(maxacc, 4) * mc <= ((int64_t)1 << 28);
        if (eager) {
            size_t free_b = 0, total_b = 0;
            const size_t need = ((size_t)round_up(maxacc, 4) * (mc + 2 * SB) + (size_t)(KSPLIT_MAX_R4 + 2) * SB * mc) * sizeof(double);
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b / 2) eager = false;
        }
        const int ldr = eager ? (int)round_up(maxacc, 4) : maxacc;  // leading dimension of R (32-byte aligned columns for the right-looking kernels)
        constexpr int KSPLIT_MAX = KSPLIT_MAX_R4;
        // the block's own Schur complement (right-looking walk): kappa(block, block) of every block in one launch up front,
        // R(:, block)' R(:, block) by the split-k product kernel (rocBLAS ran this 128 x 128 x nacc product on two workgroups: 165 us at
        // nacc = 5000), slices summed by schur_reduce_kernel
        constexpr int KSPLIT_NEAR = 32;
        const int64_t nblocks = (mc + SB - 1) / SB;
        const int L4 = 4 * (int)n0;
        double *Rb, *Sb, *Rfull = nullptr, *Kn = nullptr, *Ppart = nullptr;
        double *KbbAll = nullptr, *Spart = nullptr, *Pnear = nullptr, *Kpre = nullptr, *TA = nullptr, *TB = nullptr;
        int *cnt;
        if (eager) {
            MRBF_TRY(get_buf(ctx, S_PHI, (size_t)ldr * (mc + SB), &Rfull));  // R(:, j) for every candidate j (+ one block: the products read whole 128-column tiles)
            MRBF_TRY(get_buf(ctx, S_STAGE_D, (size_t)SB * mc, &Kn));         // kappa(new, ahead), ld = SB
            MRBF_TRY(get_buf(ctx, S_STAGE_A, (size_t)(KSPLIT_MAX + 1) * SB * mc, &Ppart));  // the k slices of R(old, new)' R(old, ahead) (+ the tail's)
            MRBF_TRY(get_buf(ctx, S_OUT_A, (size_t)SB * SB * nblocks, &KbbAll));
            MRBF_TRY(get_buf(ctx, S_STAGE_B, (size_t)(2 * KSPLIT_NEAR + 2) * SB * SB, &Spart));
            Pnear = Spart + (size_t)KSPLIT_NEAR * SB * SB;       // the k slices of the next block's update (few columns: split 32 ways; + the tail's)
            Kpre = Pnear + (size_t)(KSPLIT_NEAR + 1) * SB * SB;  // kappa(every candidate of the block, the next block's columns)
            if (q > 0) {
                MRBF_TRY(get_buf(ctx, S_T2, (size_t)4 * n0 * mc, &TA));
                MRBF_TRY(get_buf(ctx, S_OUT_B, (size_t)4 * n0 * mc, &TB));
            }
        }
        MRBF_TRY(get_buf(ctx, S_Q1, (size_t)maxacc * SB, &Rb));          // R = L_acc^-1 K[acc, block] (left-looking walk)
        MRBF_TRY(get_buf(ctx, S_RHS, (size_t)3 * SB * SB, &Sb));          // Schur complement of the block | in-block factor columns (two: see below)
        double *const Lblk2[2] = {Sb + (size_t)SB * SB, Sb + (size_t)2 * SB * SB};
        MRBF_TRY(get_buf(ctx, S_IPIV, (size_t)2 * SB + 8, &cnt));
        int *const blkidx2[2] = {cnt + 8, cnt + 8 + SB};
        // two streams (right-looking walk): after a block's decisions only the NEXT block's columns of R are needed at once; they are
        // extended on the main stream, the far columns on the side stream while the next block's decision kernel -- one workgroup, 0.46
        // to 0.8 ms -- runs.  The side stream reads the block's factor columns and indices while the next decision kernel writes its own:
        // two copies, by block parity; the main stream waits for the side stream's previous update before it touches what that one
        // reads or writes (Kn, Ppart, the next block's columns of R).
        // The side stream's work is released by an event recorded just before the decision kernel's launch: the decision kernel's one
        // workgroup is then placed at about the same time as the side stream's first workgroups, and with (nearly) the whole LDS of its
        // compute unit asked for, none of them joins it there.  (Tried and dropped: a stream of its own for the walk, with or without the
        // lowest priority -- the process's fifth stream lands on a hardware queue it shares with the main stream, and every small kernel
        // of the walk became 2 to 4 times slower, 5.4 -> 11.3 ms at d = 64.  The context's bulk stream has a queue of its own.)
        // kappa(block, next block) for ALL the block's candidates goes on the side stream while they are being decided: the update of the
        // next block's columns then starts from rows picked out of it instead of a kappa launch of its own on the critical path.
        hipStream_t sfar = ctx->bulk_stream;
        bool far_pending = false, prek_any = false;
        int64_t far_from = 0;  // first candidate of the side stream's pending update
        if (eager) {
            // (per call: the attribute is per device, and one process may drive several)
            MRBF_HIP(ctx, hipFuncSetAttribute((const void *)block_forward_mfma_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwm_shm_bytes(64)));
            MRBF_HIP(ctx, hipFuncSetAttribute((const void *)block_forward_mfma_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwm_shm_bytes(16)));
            MRBF_HIP(ctx, hipMemsetAsync(KbbAll + (size_t)SB * SB * (nblocks - 1), 0, (size_t)SB * SB * sizeof(double), s));  // (the last block may be partial)
            const dim3 kgrid(2, SB / 16, (unsigned)nblocks);
            MRBF_DISPATCH_KID(kp.kid, hipLaunchKernelGGL((kappa_block_kernel<KID, 1>), kgrid, dim3(256), 0, s, st->Xc, d, st->LamT, st->P0c, F, (int)n0,
                                                         q > 0 ? 1 : 0, st->acc, 0, (int64_t)0, SB, kp, (double *)nullptr, 0, KbbAll, 1, mc));
            if (q > 0) hipLaunchKernelGGL(tail_forms_kernel, dim3(nb((int64_t)n0 * mc)), dim3(256), 0, s, st->LamT, st->P0c, F, (int)n0, mc, TA, TB);
        }
        // rows nacc_old .. nacc_old + nblk - 1 of R for the candidates [j0, j0 + ncols) on stream su (Kn, Ppart by absolute candidate index)
        struct ExtJob {
            int64_t i0, j0, ncols;
            int nacc_old, nblk;
            double *Lblk;
            int *blkidx;
            bool is_near, pre, valid;
        };
        const int64_t pstride = (int64_t)SB * mc;
        // (is_near: the next block's columns, on the critical path: the product split 32 ways into its own small slice buffer and the
        // substitution in 16-column workgroups)
        auto extend = [&](const ExtJob &J, hipStream_t su) -> int {
            const int64_t i0 = J.i0, j0 = J.j0, ncols = J.ncols;
            const int nacc_old = J.nacc_old, nblk = J.nblk;
            double *const Lblk = J.Lblk;
            int *const blkidx = J.blkidx;
            const bool small = J.is_near && ncols <= SB;
            const bool pre = small && J.pre;  // kappa(block, these columns) is there already, for every candidate of the block
            if (pre) {
                MRBF_HIP(ctx, hipStreamWaitEvent(su, ctx->evx[2], 0));
            } else {
                const dim3 kgrid((unsigned)((ncols + 63) / 64), (unsigned)((nblk + 15) / 16));
                if (q > 0) {  // (the tail goes through the product below)
                    MRBF_DISPATCH_KID(kp.kid, hipLaunchKernelGGL((kappa_block_kernel<KID, 0>), kgrid, dim3(256), 0, su, st->Xc, d, st->LamT, st->P0c, F,
                                                                 (int)n0, 0, st->acc + nacc_old, nblk, j0, (int)ncols, kp, Kn + j0 * SB, SB,
                                                                 (double *)nullptr, 0));
                } else {
                    MRBF_DISPATCH_KID(kp.kid, hipLaunchKernelGGL((kappa_block_kernel<KID, 1>), kgrid, dim3(256), 0, su, st->Xc, d, st->LamT, st->P0c, F,
                                                                 (int)n0, 0, st->acc + nacc_old, nblk, j0, (int)ncols, kp, Kn + j0 * SB, SB,
                                                                 (double *)nullptr, 0));
                }
            }
            const double *const Kin = pre ? Kpre : Kn + j0 * SB;
            int ksplit = 0;
            double *const Pb = small ? Pnear : Ppart + j0 * SB;
            const int64_t ps = small ? (int64_t)SB * SB : pstride;
            if (nacc_old > 0) {
                // enough (column tile, k slice) workgroups to fill the device twice over, slices of whole 16-deep groups
                const int ntile = (int)((ncols + 63) / 64);
                ksplit = std::max(1, std::min({small ? KSPLIT_NEAR : KSPLIT_MAX, (512 + ntile - 1) / ntile, (nacc_old + 63) / 64}));
                const int kchunk = (int)round_up((nacc_old + ksplit - 1) / ksplit, 16);
                ksplit = (nacc_old + kchunk - 1) / kchunk;
                // (left operand: the new sites' columns of R in place, through the block's index list)
                hipLaunchKernelGGL(r4_tn_gemm_kernel, dim3((unsigned)ntile, (unsigned)ksplit), dim3(256), 0, su, Rfull + i0 * (int64_t)ldr, ldr,
                                   Rfull + j0 * (int64_t)ldr, (int64_t)ldr, nacc_old, ncols, kchunk, Pb, ps, blkidx, nblk);
            }
            if (q > 0 && !pre) {  // the tail of kappa(new, these columns): one more slice, TA(:, new)' TB(:, columns)
                hipLaunchKernelGGL(r4_tn_gemm_kernel, dim3((unsigned)((ncols + 63) / 64), 1), dim3(256), 0, su, TA + i0 * (int64_t)L4, L4, TB + j0 * (int64_t)L4,
                                   (int64_t)L4, L4, ncols, (int)round_up(L4, 16), Pb + (int64_t)ksplit * ps, ps, blkidx, nblk);
                ++ksplit;
            }
            if (ncols <= 1024)
                hipLaunchKernelGGL(block_forward_mfma_kernel<16>, dim3((unsigned)((ncols + 15) / 16)), dim3(256), fwm_shm_bytes(16), su, Kin, Pb, ksplit, ps,
                                   Lblk, blkidx, nblk, ncols, Rfull + j0 * (int64_t)ldr + nacc_old, (int64_t)ldr, pre ? 1 : 0);
            else
                hipLaunchKernelGGL(block_forward_mfma_kernel<64>, dim3((unsigned)((ncols + 63) / 64)), dim3(256), fwm_shm_bytes(64), su, Kin, Pb, ksplit, ps,
                                   Lblk, blkidx, nblk, ncols, Rfull + j0 * (int64_t)ldr + nacc_old, (int64_t)ldr, 0);
            return 0;
        };
        ExtJob far_job{};  // the far columns' update of the block before: issued after this block's decision kernel is on its way
        int blkno = 0;
        bool info_checked = false;
        if (eager) {  // the side stream's first kernel reads what the main stream has just set up (lambda, F, the candidates' coordinates)
            MRBF_HIP(ctx, hipEventRecord(ctx->evx[0], s));
            MRBF_HIP(ctx, hipStreamWaitEvent(sfar, ctx->evx[0], 0));
        }
        MRBF_HIP(ctx, hipMemsetAsync(cnt, 0, 8 * sizeof(int), s));
        MRBF_HIP(ctx, hipMemsetAsync(st->LK, 0, (size_t)maxacc * maxacc * sizeof(double), s));
        int nacc = 0;
        for (int64_t i0 = 0; i0 < mc && (int64_t)n0 + nacc < max_points && nacc < maxacc; i0 += SB) {
            const int bsz = (int)std::min<int64_t>(SB, mc - i0);
            const double mone = -1.0;
            if (far_pending && i0 >= far_from) {  // (a block without accepted sites in between: this block's columns were last touched by the side stream)
                MRBF_HIP(ctx, hipStreamWaitEvent(s, ctx->evx[1], 0));
                far_pending = false;
            }
            double *const Lblk = Lblk2[blkno & 1];
            int *const blkidx = blkidx2[blkno & 1];
            ++blkno;
            const int64_t near_next = std::min<int64_t>(SB, mc - (i0 + bsz));
            const bool have_prek = eager && near_next > 0;
            if (eager) {
                Rb = Rfull + i0 * (int64_t)ldr;  // this block's columns of R are up to date: every earlier block extended them
                int ks = 0;
                if (nacc > 0) {
                    const int ntile = (bsz + 63) / 64;
                    ks = std::max(1, std::min(KSPLIT_NEAR, (nacc + 63) / 64));
                    const int kchunk = (int)round_up((nacc + ks - 1) / ks, 16);
                    ks = (nacc + kchunk - 1) / kchunk;
                    hipLaunchKernelGGL(r4_tn_gemm_kernel, dim3((unsigned)ntile, (unsigned)ks), dim3(256), 0, s, Rb, ldr, Rb, (int64_t)ldr, nacc, (int64_t)bsz,
                                       kchunk, Spart, (int64_t)SB * SB);
                }
                hipLaunchKernelGGL(schur_reduce_kernel, dim3(SB * SB / 256), dim3(256), 0, s, KbbAll + (size_t)(i0 / SB) * SB * SB, Spart, ks, bsz, Sb);
            } else {
                // left-looking walk: kappa(accepted | block, block), the block's columns of R by a triangular solve with the accepted factor
                if (bsz < SB) MRBF_HIP(ctx, hipMemsetAsync(Sb, 0, (size_t)SB * SB * sizeof(double), s));
                const dim3 kgrid((unsigned)((bsz + 63) / 64), (unsigned)((nacc + bsz + 15) / 16));
                MRBF_DISPATCH_KID(kp.kid, hipLaunchKernelGGL((kappa_block_kernel<KID, 1>), kgrid, dim3(256), 0, s, st->Xc, d, st->LamT, st->P0c, F, (int)n0,
                                                             q > 0 ? 1 : 0, st->acc, nacc, i0, bsz, kp, Rb, maxacc, Sb, 1));
                if (nacc > 0) {
                    MRBF_BLAS(ctx, rocblas_dtrsm(ctx->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, nacc,
                                                 bsz, &one, st->LK, maxacc, Rb, ldr));
                    MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_transpose, rocblas_operation_none, bsz, bsz, nacc, &mone, Rb, ldr, Rb, ldr,
                                                 &one, Sb, SB));
                }
            }
            if (far_job.valid) MRBF_HIP(ctx, hipEventRecord(ctx->evx[0], s));  // (releases the side stream's update: see the two streams above)
#define R4_DECIDE(KERNEL_, THREADS_, SHM_, ...)                                                                                                  \
    do {                                                                                                                                         \
        if (blkno == 1) MRBF_HIP(ctx, hipFuncSetAttribute((const void *)KERNEL_, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SHM_)));      \
        hipLaunchKernelGGL(KERNEL_, dim3(1), dim3(THREADS_), SHM_, s, Sb, bsz, i0, (int)n0, q, (int)max_points, maxacc, thr, st->Prow, st->Ginv, \
                           st->acc, cnt, Lblk, blkidx, ##__VA_ARGS__);                                                                              \
    } while (0)
            if (q == 0 || q > 192)
                R4_DECIDE(select_block_kernel, SEL_THREADS, shm);
            else if (q <= 32)
                R4_DECIDE((select_block_duo_kernel<2>), 512, walk_lds(2), (unsigned long long *)nullptr);
            else if (q <= 64)
                R4_DECIDE((select_block_duo_kernel<4>), 512, walk_lds(4), (unsigned long long *)nullptr);
            else if (q <= 80)
                R4_DECIDE((select_block_duo_kernel<5>), 512, walk_lds(5), (unsigned long long *)nullptr);
            else if (q <= 128)
                R4_DECIDE((select_block_walk_kernel<8, 4, 8>), 512, walk_lds(8), (unsigned long long *)nullptr);
            else if (q <= 144)
                R4_DECIDE((select_block_walk_kernel<8, 5, 9>), 512, walk_lds(9), (unsigned long long *)nullptr);
            else
                R4_DECIDE((select_block_reg_kernel<3, 12, 16>), SEL_THREADS, shm_reg);
#undef R4_DECIDE
            // side stream, issued only now (the host calls cost ~40 us; ahead of the Schur product and the decision kernel they delayed the
            // critical path by as much): the far columns' update of the block before, then kappa(this block, next block)
            auto issue_side = [&]() -> int {
                if (far_job.valid) {
                    MRBF_HIP(ctx, hipStreamWaitEvent(sfar, ctx->evx[0], 0));
                    MRBF_TRY(extend(far_job, sfar));
                    MRBF_HIP(ctx, hipEventRecord(ctx->evx[1], sfar));
                    far_job.valid = false;
                }
                if (have_prek) {
                    const dim3 kgrid((unsigned)((near_next + 63) / 64), (unsigned)((bsz + 15) / 16));
                    MRBF_DISPATCH_KID(kp.kid, hipLaunchKernelGGL((kappa_block_kernel<KID, 1>), kgrid, dim3(256), 0, sfar, st->Xc, d, st->LamT, st->P0c, F, (int)n0,
                                                                 q > 0 ? 1 : 0, st->acc, 0, i0 + bsz, (int)near_next, kp, (double *)nullptr, 0, Kpre, 1,
                                                                 (int64_t)0, i0, bsz));
                    MRBF_HIP(ctx, hipEventRecord(ctx->evx[2], sfar));
                    prek_any = true;
                }
                return 0;
            };
            int hc_local[3] = {0, 0, 0};
            int *hc = ctx->hpin ? reinterpret_cast<int *>(ctx->hpin + HPIN_R4_COUNT) : hc_local;  // (pinned: the download does not cost a round trip of its own)
            MRBF_HIP(ctx, hipMemcpyAsync(hc, cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
            const bool check_info = blkno == 1 && q > 0;   // (with or without the pinned block: a rank-deficient start set must be reported)
            info_checked = info_checked || check_info;
            if (check_info) MRBF_HIP(ctx, hipMemcpyAsync(hc + 2, dinfo, sizeof(int), hipMemcpyDeviceToHost, s));
            // the next block's shapes depend on the number accepted so far: the host waits for the counts only, the factor's new rows are
            // appended under the round trip
            if (ctx->evx[3]) MRBF_HIP(ctx, hipEventRecord(ctx->evx[3], s));
            hipLaunchKernelGGL(append_rows_kernel, dim3(nb((int64_t)SB * (nacc + SB))), dim3(256), 0, s, Rb, ldr, nacc, Lblk, blkidx, cnt, st->LK, maxacc);
            MRBF_TRY(issue_side());
            if (ctx->evx[3])
                MRBF_HIP(ctx, hipEventSynchronize(ctx->evx[3]));
            else
                MRBF_HIP(ctx, hipStreamSynchronize(s));
            if (check_info && hc[2] != 0)
                return fail(ctx, MRBF_ESINGULAR, "the start set's polynomial matrix is rank deficient (potrf info %d): use the host mirror", hc[2]);
            const int nacc_old = nacc, nblk = hc[1];
            nacc = hc[0];
            const int64_t i1 = i0 + bsz, ahead = mc - i1;
            if (eager && nblk > 0 && ahead > 0 && (int64_t)n0 + nacc < max_points && nacc < maxacc) {
                if (far_pending) MRBF_HIP(ctx, hipStreamWaitEvent(s, ctx->evx[1], 0));  // the side stream's update of the block before
                // the next block's columns first, alone on the device (started together, the far update's 150 workgroups doubled the
                // duration of these few); the far columns then run under the next block's Schur product and decisions
                const int64_t near = std::min<int64_t>(SB, ahead);
                MRBF_TRY(extend(ExtJob{i0, i1, near, nacc_old, nblk, Lblk, blkidx, true, have_prek, true}, s));
                if (ahead > near) {
                    far_job = ExtJob{i0, i1 + near, ahead - near, nacc_old, nblk, Lblk, blkidx, false, false, true};
                    far_pending = true;  // (its event is recorded when it is issued: before the next host wait)
                    far_from = i1 + near;
                } else {
                    far_pending = false;
                }
            }
        }
        // (the buffers go back to the pool after this stream's work; a far update that was never issued -- the walk ended -- is dropped)
        if (far_pending && !far_job.valid) MRBF_HIP(ctx, hipStreamWaitEvent(s, ctx->evx[1], 0));
        if (prek_any) MRBF_HIP(ctx, hipStreamWaitEvent(s, ctx->evx[2], 0));
        MRBF_HIP(ctx, hipGetLastError());
        std::vector<int> hacc((size_t)maxacc + 1);
        MRBF_HIP(ctx, hipMemcpyAsync(hacc.data(), st->acc, hacc.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        int hinfo = 0;
        if (!info_checked && q > 0) MRBF_HIP(ctx, hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, s));  // (no block ran)
        MRBF_HIP(ctx, hipStreamSynchronize(s));
        if (hinfo != 0)
            return fail(ctx, MRBF_ESINGULAR, "the start set's polynomial matrix is rank deficient (potrf info %d): use the host mirror", hinfo);
        st->nacc = hacc[maxacc];
        *n_accepted = st->nacc;
        if (accepted_out)
            for (int i = 0; i < st->nacc; ++i) accepted_out[i] = hacc[i];
        return 0;
    };
    const int rc = run();
    if (rc != 0 || !state_out) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->bulk_stream) (void)hipStreamSynchronize(ctx->bulk_stream);  // (an error return may leave the side stream's update in flight)
        (void)hipFree(st->block);
        delete st;
        return rc;
    }
    *state_out = st;
    ++ctx->live_round4;
    return MRBF_OK;
}

extern "C" int32_t mrbf_fit_from_round4(mrbf_ctx *ctx, const mrbf_round4_state *st, int32_t k, const double *values, mrbf_model **model,
                                        double *weights_out, double *poly_out, mrbf_fit_info *info) {
    using namespace r4;
    if (!ctx) return -1;
    if (!st) return fail(ctx, -2, "state is NULL");
    if (k < 1 || k > 1024) return fail(ctx, -3, "k = %d out of range", k);
    if (!values) return fail(ctx, -4, "values is NULL");
    if (!model) return fail(ctx, -5, "model is NULL");
    *model = nullptr;
    if (st->n0 != st->q)
        return fail(ctx, -2, "factor reuse needs a unisolvent start set (n0 = %lld, q = %d): the start set's own null-space directions are not "
                             "part of the round-4 factor; use mrbf_fit", (long long)st->n0, st->q);
    (void)hipSetDevice(ctx->device);
    const int n0 = (int)st->n0, j = st->nacc, q = st->q, d = st->d;
    const int64_t n = n0 + j;
    mrbf_fit_info local;
    if (!info) info = &local;
    std::memset(info, 0, sizeof(*info));
    info->n = (int32_t)n;
    info->q = q;
    info->path = MRBF_PATH_ROUND4;
    info->rel_residual = NAN;
    info->max_pitw = NAN;
    hipStream_t s = ctx->stream;
    const double one = 1.0, zero = 0.0, mone = -1.0;
    const double *Y;
    MRBF_TRY(stage_in(ctx, S_STAGE_B, values, (size_t)n * k, &Y));
    double *S;
    MRBF_TRY(get_buf(ctx, S_STAGE_A, (size_t)n * d, &S));
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[5], s));
    hipLaunchKernelGGL(concat_sites_kernel, dim3(nb(n * d)), dim3(256), 0, s, st->C0, st->Xc, st->acc, n0, j, d, S);
    mrbf_model *M = nullptr;
    MRBF_TRY(build_model_shell(ctx, n, d, k, S, st->kid, st->a, st->b, st->deg, &M));
    auto run = [&]() -> int {
        double *Y0, *Ya, *LaT, *P0a, *Lacc, *w0, *rhs, *PiLU;
        int *ipiv, *dinfo;
        MRBF_TRY(get_buf(ctx, S_RHS, (size_t)n * k + (size_t)n0 * k * 2 + k, &Y0));
        Ya = Y0 + (size_t)n0 * k;
        w0 = Ya + (size_t)std::max(j, 1) * k;
        rhs = w0 + (size_t)n0 * k;
        MRBF_TRY(get_buf(ctx, S_Q1, (size_t)n0 * std::max(j, 1) * 2, &LaT));
        P0a = LaT + (size_t)n0 * std::max(j, 1);
        MRBF_TRY(get_buf(ctx, S_G, (size_t)std::max(j, 1) * std::max(j, 1) + (size_t)q * q, &Lacc));
        PiLU = Lacc + (size_t)std::max(j, 1) * std::max(j, 1);
        MRBF_TRY(get_buf(ctx, S_IPIV, (size_t)q + 4, &ipiv));
        MRBF_TRY(get_buf(ctx, S_INFO, (size_t)4, &dinfo));
        hipLaunchKernelGGL(split_values_kernel, dim3(nb(n * k)), dim3(256), 0, s, Y, n0, j, k, Y0, Ya);
        MRBF_HIP(ctx, hipMemcpyAsync(rhs, Y0, (size_t)n0 * k * sizeof(double), hipMemcpyDeviceToDevice, s));
        MRBF_HIP(ctx, hipMemsetAsync(w0, 0, (size_t)n0 * k * sizeof(double), s));
        if (j > 0) {
            hipLaunchKernelGGL(gather_cols_kernel, dim3(nb((int64_t)n0 * j)), dim3(256), 0, s, st->LamT, (int64_t)n0, st->acc, j, LaT);
            hipLaunchKernelGGL(gather_cols_kernel, dim3(nb((int64_t)n0 * j)), dim3(256), 0, s, st->P0c, (int64_t)n0, st->acc, j, P0a);
            hipLaunchKernelGGL(copy_factor_kernel, dim3(nb((int64_t)j * j)), dim3(256), 0, s, st->LK, st->maxacc, j, Lacc);
            // Ya <- Ya - Lam_acc Y0 ;  v = K_acc^-1 (..) by the two triangular solves with the round-4 factor
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_transpose, rocblas_operation_none, j, k, n0, &mone, LaT, n0, Y0, n0, &one, Ya, j));
            MRBF_BLAS(ctx, rocblas_dtrsm(ctx->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, j, k, &one,
                                         Lacc, j, Ya, j));
            MRBF_BLAS(ctx, rocblas_dtrsm(ctx->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit, j, k,
                                         &one, Lacc, j, Ya, j));
            // w0 = -Lam_acc' v ;  rhs = Y0 - Phi00 w0 - Phi0a v
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, n0, k, j, &mone, LaT, n0, Ya, j, &zero, w0, n0));
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, n0, k, n0, &mone, st->Phi00, n0, w0, n0, &one, rhs, n0));
            MRBF_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, n0, k, j, &mone, P0a, n0, Ya, j, &one, rhs, n0));
        }
        // Pi0 lambda = rhs  (Pi0 square, unisolvent start set)
        if (q > 0) {
            MRBF_HIP(ctx, hipMemcpyAsync(PiLU, st->Pi0, (size_t)q * q * sizeof(double), hipMemcpyDeviceToDevice, s));
            MRBF_BLAS(ctx, rocsolver_dgesv(ctx->blas, q, k, PiLU, q, ipiv, rhs, q, dinfo));
            int hinfo = 0;
            MRBF_HIP(ctx, hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, s));
            MRBF_HIP(ctx, hipStreamSynchronize(s));
            info->factor_info = hinfo;
            if (hinfo != 0) return fail(ctx, MRBF_ESINGULAR, "start set is not unisolvent (gesv info %d)", hinfo);
        }
        hipLaunchKernelGGL(pack_solution_kernel, dim3(nb(M->npad * k + (int64_t)q * k)), dim3(256), 0, s, w0, Ya, rhs, n0, j, k, q, M->npad, M->W,
                           M->Wc, M->lam);
        MRBF_HIP(ctx, hipGetLastError());
        MRBF_HIP(ctx, hipEventRecord(ctx->ev[6], s));
        if (ctx->residual) {
            MRBF_TRY(fit_check(ctx, M, Y, info));
            // The kept factor is only as good as the start set it was built on: kappa is formed with cancellation against the start set's
            // polynomial interpolant, and a start set that barely passes the affine filter's pivot test (a shrunken trust region over
            // far-apart database sites; seen in the iteration rehearsal: residual 7e-8) takes the fit outside the 1e-8 value tolerance.
            // The interpolation residual is the tripwire: beyond 1e-9 the caller is told to take the ordinary fit (the decision table
            // maps MRBF_ENOTPD of this entry point to it) -- accuracy is never traded for the two triangular solves.
            if (!(info->rel_residual <= 1e-9))
                return fail(ctx, MRBF_ENOTPD, "kept round-4 factor too inaccurate for this training set (relative residual %.2e): use mrbf_fit",
                            info->rel_residual);
        }
        if (weights_out) MRBF_HIP(ctx, hipMemcpyAsync(weights_out, M->W, (size_t)n * k * sizeof(double), hipMemcpyDefault, s));
        if (poly_out && q > 0) MRBF_HIP(ctx, hipMemcpyAsync(poly_out, M->lam, (size_t)q * k * sizeof(double), hipMemcpyDefault, s));
        MRBF_HIP(ctx, hipStreamSynchronize(s));
        MRBF_HIP(ctx, hipEventElapsedTime(&info->ms_solve, ctx->ev[5], ctx->ev[6]));
        info->ms_total = info->ms_solve;
        return 0;
    };
    const int rc = run();
    if (rc != 0) {
        (void)hipStreamSynchronize(s);
        destroy_model(ctx, M);
        return rc;
    }
    *model = M;
    return MRBF_OK;
}

extern "C" int32_t mrbf_round4_sites(const mrbf_round4_state *st, int64_t *n0, int64_t *n_candidates, int32_t *n_accepted) {
    if (!st) return -1;
    if (n0) *n0 = st->n0;
    if (n_candidates) *n_candidates = st->mc;
    if (n_accepted) *n_accepted = st->nacc;
    return MRBF_OK;
}
