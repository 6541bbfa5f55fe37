// Directed search on the device with constraint rows: the direction QP of the reference's parked compute_descent_step(::Val{:ds}, ...)
// (src/descent.jl:598-645) extended by the rows of get_criticality (src/descent.jl:196-236), and the criticality call around it.
//
// One workgroup solves one QP:
//   minimise 1/2 ||G d - r||^2  s.t.  l <= d <= u,  G d <= 0,  A_eq d = b_eq,  A_in d <= b_in
// by ds_qp.hip's primal active-set method, generalised.  W = [G; A_eq; A_in] has K <= 16 rows, c = W d, h = (0, b_eq, b_in).  The step is
// p_N = W_N' a with a supported on the universe U = (objective rows) + S: the K x K work of ds_dev.hpp runs on M[U, U] with M = W_N W_N',
// the rows of S move to their right-hand side (dc_S = h_S - c_S), the objective rows outside S towards rho = r - z.  A constraint row
// outside S has coefficient zero and is seen by the ratio test alone.  Equality rows start in S and are never dropped; one that the
// factorisation leaves out as dependent on the free variables blocks a step that would move it on either side and joins S again through
// the ratio test, so that steps and multipliers always belong to one working set.  The factorisation takes at most |N| pivots.  The
// start d = 0 must satisfy the rows (ds_rows_host.hpp: START_TOL); there is no phase 1.  Without constraint rows every operation is
// ds_qp_kernel's, in its order: the same bits.  Every sum runs in an order fixed by the shape; no atomics.
#include "descent_call.hpp"
#include "ds.hpp"
#include "ds_dev.hpp"
#include "ds_rows_host.hpp"
#include "lp_dev.hpp"

namespace mrbf {
namespace ds {
namespace rows {

static_assert(THREADS == lp::THREADS, "row_pass runs on a workgroup of lp::THREADS");

struct Args {
    int n, k, meq, min;
    int64_t xs, bs;  // QP p reads x at x + p xs and its bounds at lb / ub + p bs (0: one box for every QP)
    const double *G, *r, *x, *lb, *ub, *Aeq, *beq, *Ain, *bin;
    double *d_out, *c_out, *omega_out, *mult_out;
    int *status_out, *iters_out;
    double *ws;  // per QP 4 n doubles: d, p, l, u
    int *wsi;    // per QP n ints: 0 free, -1 on the lower bound, +1 on the upper bound, 2 fixed (l = u)
};

enum { I_NFREE = I_ROWHIT + 1 };
static_assert(I_NFREE < NISC, "scalar words");
// the full-length vectors of the K rows, after the compact ones of the K x K work (ds_dev.hpp: V_*; those of them that the K x K work
// does not touch -- V_DZ, V_ROWSUM, V_RSCALE, V_R, V_Y, V_YSC, V_AR -- are full-length here as they are in ds_qp.hip)
enum { F_C = V_NVEC, F_RHO, F_AV, F_MU, F_H, F_NVEC };
static_assert(F_NVEC <= NVEC, "carve too small");

// one QP's rows: entry (i, j) of W
struct Rows {
    int n, k, meq;
    const double *G, *Aeq, *Ain;
    __device__ double operator()(int i, int j) const {
        if (i < k) return G[(size_t)j * k + i];
        return i < k + meq ? Aeq[(size_t)(i - k) * n + j] : Ain[(size_t)(i - k - meq) * n + j];
    }
};

// M = W_N W_N' from W, whenever N changes (ds_qp.hip: refresh_M), and |N|
__device__ void refresh_M(const Rows &W, const int *flag, int n, int K, double *part, int *ipart, double *M, int *nfree) {
    lp::row_pass(n, K * K, [&](int e, int j) { return flag[j] == 0 ? W(e / K, j) * W(e % K, j) : 0.0; }, part, M);
    const int t = threadIdx.x;
    int cnt = 0;
    for (int j = t; j < n; j += THREADS) cnt += flag[j] == 0 ? 1 : 0;
    ipart[t] = cnt;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) ipart[t] += ipart[t + s];
        __syncthreads();
    }
    if (t == 0) *nfree = ipart[0];
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void ds_qp_rows_kernel(Args a, int64_t qp0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t qp = qp0 + blockIdx.x;
    const int t = threadIdx.x, n = a.n, k = a.k, meq = a.meq, K = a.k + a.meq + a.min;
    const Carve cv = carve(K);
    Small sm;  // the K x K work on the universe U: sm.k = |U|, sm.M = M[U, U]
    sm.k = K;
    double *M = (double *)(smem + cv.M);
    sm.M = (double *)(smem + cv.MU), sm.L = (double *)(smem + cv.L), sm.A = (double *)(smem + cv.A), sm.v = (double *)(smem + cv.vec);
    sm.piv = (int *)(smem + cv.ivec), sm.done = sm.piv + MAXK, sm.inS = sm.piv + 2 * MAXK;
    int *inS = sm.piv + 3 * MAXK, *U = sm.piv + 4 * MAXK;
    double *part = (double *)(smem + cv.part), *dsc = (double *)(smem + cv.dsc);
    int *ipart = (int *)(smem + cv.ipart), *isc = (int *)(smem + cv.isc);
    double *dc = sm.vec(V_DZ), *rowsum = sm.vec(V_ROWSUM), *rscale = sm.vec(V_RSCALE), *rv = sm.vec(V_R), *yv = sm.vec(V_Y);
    double *ysc = sm.vec(V_YSC), *ar = sm.vec(V_AR);
    double *c = sm.vec(F_C), *rho = sm.vec(F_RHO), *av = sm.vec(F_AV), *mu = sm.vec(F_MU), *h = sm.vec(F_H);

    Rows W;
    W.n = n, W.k = k, W.meq = meq;
    W.G = a.G + qp * (int64_t)k * n, W.Aeq = a.Aeq + qp * (int64_t)meq * n, W.Ain = a.Ain + qp * (int64_t)a.min * n;
    const double *x = a.x + qp * a.xs, *lb = a.lb + qp * a.bs, *ub = a.ub + qp * a.bs;
    double *dv = a.ws + (size_t)blockIdx.x * WS_DOUBLES_PER_VAR * n, *pv = dv + n, *lo = dv + 2 * n, *hi = dv + 3 * n;
    int *flag = a.wsi + (size_t)blockIdx.x * n;
    const double INF = __builtin_huge_val(), QNAN = __builtin_nan("");

    // ---- the box, the start, the row scales
    int empty = 0, outside = 0;
    for (int j = t; j < n; j += THREADS) {
        const double l = fmax(-1.0, lb[j] - x[j]), u = fmin(1.0, ub[j] - x[j]);
        if (!(l <= u)) empty = 1;
        else if (!(l <= 0.0 && u >= 0.0)) outside = 1;
        lo[j] = l, hi[j] = u, dv[j] = 0.0, pv[j] = 0.0;
        flag[j] = l == u ? 2 : (l == 0.0 ? -1 : (u == 0.0 ? 1 : 0));
    }
    empty = __syncthreads_or(empty);
    outside = __syncthreads_or(outside);
    lp::row_pass(n, K, [&](int i, int j) { return fabs(W(i, j)); }, part, rowsum);
    if (t == 0) {
        int critical = 0, no_start = 0;
        for (int i = 0; i < K; ++i) {
            const int kind = kind_of(i, k, meq);
            double ri = 0.0, hv = 0.0;
            if (kind == OBJECTIVE) {
                ri = a.r[qp * k + i];
                if (!(ri < 0.0)) critical = 1;  // some r_i >= 0, or a NaN (descent.jl:615-617)
            } else {
                hv = kind == EQUALITY ? a.beq[qp * meq + (i - k)] : a.bin[qp * a.min + (i - k - meq)];
                // the start d = 0 must satisfy the row: a miss within START_TOL of the row's scale is clamped, a larger one (or a NaN) is
                // no start
                const double miss = kind == EQUALITY ? fabs(hv) : -hv;
                if (!(miss <= 0.0)) {
                    if (!(miss <= START_TOL * rowsum[i])) no_start = 1;
                    hv = 0.0;
                }
            }
            rv[i] = ri, h[i] = hv, rscale[i] = rowsum[i] + fabs(ri) + fabs(hv), mu[i] = 0.0, inS[i] = kind == EQUALITY ? 1 : 0;
        }
        // the start d = 0 outside a non-empty box (x outside [lb, ub] by less than one): the method has no feasible start
        isc[I_BAD] = critical ? MRBF_DS_CRITICAL
                              : (empty ? MRBF_DS_INFEASIBLE : (outside ? MRBF_DS_GAVE_UP : (no_start ? MRBF_DS_NO_START : MRBF_DS_OK)));
    }
    __syncthreads();
    int status = isc[I_BAD];
    int iters = 0, dropped = 0, full = 0, degen = 0;
    if (status == MRBF_DS_OK) {
        refresh_M(W, flag, n, K, part, ipart, M, &isc[I_NFREE]);
        const int cap = iteration_cap(n, K);
        for (;;) {
            if (iters >= cap) {
                status = MRBF_DS_GAVE_UP;
                break;
            }
            ++iters;
            lp::row_pass(n, K, [&](int i, int j) { return W(i, j) * dv[j]; }, part, c);
            // ---- the K x K problem on the universe U: the coefficients a of the step
            if (t == 0) {
                int ku = 0;
                for (int i = 0; i < K; ++i) {
                    rho[i] = i < k ? rv[i] - c[i] : 0.0;
                    if (i < k || inS[i]) U[ku++] = i;
                }
                sm.k = ku;
                double *cz = sm.vec(V_Z), *crho = sm.vec(V_RHO);
                for (int p = 0; p < ku; ++p) {
                    const int i = U[p];
                    for (int q = 0; q < ku; ++q) sm.M[p * ku + q] = M[i * K + U[q]], sm.L[p * ku + q] = 0.0;
                    cz[p] = i < k ? c[i] : c[i] - h[i], crho[p] = rho[i], sm.inS[p] = inS[i];
                }
                int n_s = 0;
                // with constraint rows the rank is at most |N|; without them ds_qp_kernel's factorisation, to the bit
                isc[I_BAD] = step_coeffs(sm, n_s, K > k ? isc[I_NFREE] : MAXK) ? 0 : 1;
                isc[I_KIND] = n_s;
                const double *cav = sm.vec(V_AV);
                for (int i = 0; i < K; ++i) av[i] = 0.0;
                for (int p = 0; p < ku; ++p) av[U[p]] = cav[p], inS[U[p]] = sm.inS[p];
            }
            __syncthreads();
            if (isc[I_BAD]) {
                status = MRBF_DS_GAVE_UP;
                break;
            }
            for (int j = t; j < n; j += THREADS) {
                double acc = 0.0;
                if (flag[j] == 0)
                    for (int i = 0; i < K; ++i) acc += W(i, j) * av[i];
                pv[j] = acc;
            }
            __syncthreads();
            lp::row_pass(n, K, [&](int i, int j) { return W(i, j) * pv[j]; }, part, dc);
            // ---- has the step vanished?  then the multipliers; else the rows' part of the ratio test
            if (t == 0) {
                bool vanish = true;
                for (int i = 0; i < K; ++i) vanish = vanish && fabs(dc[i]) <= VANISH_TOL * rscale[i];
                if (full >= 2 || vanish) {
                    const int ku = sm.k;
                    multipliers(sm, isc[I_KIND]);
                    const double *cmu = sm.vec(V_MU);
                    for (int i = 0; i < K; ++i) mu[i] = 0.0;
                    for (int p = 0; p < ku; ++p) mu[U[p]] = cmu[p];
                    double mscale = 0.0;
                    for (int i = 0; i < K; ++i) {
                        const double zi = i < k ? c[i] : 0.0;
                        yv[i] = mu[i] - rho[i];
                        ysc[i] = fabs(rv[i]) + fabs(zi) + fabs(mu[i]);
                        if (i < k) mscale = fmax(mscale, fabs(rv[i]) + fabs(zi));
                    }
                    double best = 0.0;
                    int idx = -1;
                    for (int i = 0; i < K; ++i) {
                        const double v = inS[i] && droppable(kind_of(i, k, meq)) ? -mu[i] / mscale : 0.0;
                        if (v > DUAL_TOL && v > best && !(degen && idx >= 0)) best = v, idx = i;  // degenerate: the least index
                    }
                    isc[I_MODE] = MODE_MULT, isc[I_KIND] = idx >= 0 ? 1 : 0, isc[I_IDX] = idx;
                    dsc[D_BEST] = best;
                } else {
                    double amin = INF;
                    for (int i = 0; i < K; ++i) {
                        const double move = two_sided(kind_of(i, k, meq)) ? fabs(dc[i]) : dc[i];
                        ar[i] = (!inS[i] && move > VANISH_TOL * rscale[i]) ? fmax(0.0, (i < k ? -c[i] : h[i] - c[i]) / dc[i]) : INF;
                        amin = fmin(amin, ar[i]);
                    }
                    isc[I_MODE] = MODE_STEP;
                    dsc[D_ALPHA] = fmin(1.0, amin);
                }
            }
            __syncthreads();
            if (isc[I_MODE] == MODE_MULT) {
                // ---- s = W' y on the variables that sit on a bound: the most violating sign, lowest index on ties
                double bestv = 0.0;
                int bestj = 0x7fffffff;
                for (int j = t; j < n; j += THREADS) {
                    const int f = flag[j];
                    if (f != -1 && f != 1) continue;
                    double sj = 0.0, sc = 0.0;
                    for (int i = 0; i < K; ++i) {
                        const double g = W(i, j);
                        sj += g * yv[i], sc += fabs(g) * ysc[i];
                    }
                    const double viol = f < 0 ? -sj : sj;
                    const double ratio = sc > 0.0 ? viol / sc : 0.0;
                    if (degen ? (ratio > DUAL_TOL && bestj == 0x7fffffff) : ratio > bestv) bestv = ratio, bestj = j;
                }
                // degenerate: the least index that violates (a row goes first); else the largest ratio
                block_argmin(degen ? (double)bestj : -bestv, bestj, part, ipart);
                if (t == 0 && ipart[0] != 0x7fffffff) {
                    if (degen ? isc[I_KIND] == 0 : (-part[0] > DUAL_TOL && -part[0] > dsc[D_BEST])) isc[I_KIND] = 2, isc[I_IDX] = ipart[0];
                }
                __syncthreads();
                const int kind = isc[I_KIND], idx = isc[I_IDX];
                if (kind == 0) break;  // no multiplier violates: optimal
                ++dropped;
                full = 0;
                if (kind == 1) {
                    if (t == 0) inS[idx] = 0;
                    __syncthreads();
                } else {
                    if (t == 0) flag[idx] = 0;
                    __syncthreads();
                    refresh_M(W, flag, n, K, part, ipart, M, &isc[I_NFREE]);
                }
                continue;
            }
            // ---- ratio test over the free variables' bounds
            {
                double amin = INF;
                int aj = 0x7fffffff;
                for (int j = t; j < n; j += THREADS) {
                    if (flag[j] != 0) continue;
                    const double p = pv[j];
                    double al = p < 0.0 ? (lo[j] - dv[j]) / p : (p > 0.0 ? (hi[j] - dv[j]) / p : INF);
                    if (al < 0.0) al = 0.0;
                    if (al < amin) amin = al, aj = j;
                }
                block_argmin(amin, aj, part, ipart);
            }
            const double alpha = fmin(dsc[D_ALPHA], part[0]);
            // a step of length zero adds one constraint: the least index that blocks, a row first (then variable `only`)
            degen = !(alpha > 0.0);
            const int only = degen ? (dsc[D_ALPHA] <= 0.0 ? -1 : ipart[0]) : -2;
            __syncthreads();
            // ---- the step: a variable that blocks takes its bound's bits; the others stay inside the box
            int nh = 0, hj = 0x7fffffff;
            for (int j = t; j < n; j += THREADS) {
                if (flag[j] != 0) continue;
                const double p = pv[j];
                double al = p < 0.0 ? (lo[j] - dv[j]) / p : (p > 0.0 ? (hi[j] - dv[j]) / p : INF);
                if (al < 0.0) al = 0.0;
                if (al <= alpha && (only == -2 || only == j)) {
                    dv[j] = p < 0.0 ? lo[j] : hi[j];
                    flag[j] = p < 0.0 ? -1 : 1;
                    if (!nh) hj = j;
                    ++nh;
                } else {
                    dv[j] = fmin(fmax(dv[j] + alpha * p, lo[j]), hi[j]);
                }
            }
            part[t] = (double)nh, ipart[t] = hj;
            __syncthreads();
            for (int s = THREADS / 2; s > 0; s >>= 1) {
                if (t < s) part[t] += part[t + s], ipart[t] = min(ipart[t], ipart[t + s]);
                __syncthreads();
            }
            if (t == 0) {
                int rows_hit = 0;
                for (int i = 0; i < K; ++i)
                    if (ar[i] <= alpha && !(degen && rows_hit)) inS[i] = 1, rows_hit = 1;
                isc[I_NHIT] = (int)part[0], isc[I_IDX] = ipart[0], isc[I_ROWHIT] = rows_hit;
            }
            __syncthreads();
            const int nhit = isc[I_NHIT];
            full = (nhit == 0 && !isc[I_ROWHIT]) ? full + 1 : 0;
            if (nhit >= 1) refresh_M(W, flag, n, K, part, ipart, M, &isc[I_NFREE]);
        }
    }
    // ---- outputs: c = W d from the returned d, in row_pass's order
    double *dout = a.d_out + qp * n, *cout = a.c_out + qp * K;
    if (status == MRBF_DS_OK) {
        lp::row_pass(n, K, [&](int i, int j) { return W(i, j) * dv[j]; }, part, c);
        if (t == 0) {
            int bad = 0;
            double mx = -INF;
            for (int i = 0; i < K; ++i) {
                const double miss = i < k ? c[i] : (two_sided(kind_of(i, k, meq)) ? fabs(c[i] - h[i]) : c[i] - h[i]);
                if (!(miss <= FEAS_TOL * (rowsum[i] + fabs(h[i])))) bad = 1;  // a row beyond its tolerance, or a NaN
                if (i < k) mx = fmax(mx, c[i]);
            }
            isc[I_BAD] = bad;
            dsc[D_ALPHA] = fmax(0.0, -mx);
        }
        __syncthreads();
        if (isc[I_BAD]) status = MRBF_DS_GAVE_UP;
    }
    if (status == MRBF_DS_OK) {
        for (int j = t; j < n; j += THREADS) dout[j] = dv[j];
        if (t < K) {
            cout[t] = c[t];
            if (a.mult_out) a.mult_out[qp * K + t] = mu[t];
        }
        if (t == 0) a.omega_out[qp] = dsc[D_ALPHA];
    } else {
        const bool nan_out = status == MRBF_DS_GAVE_UP || status == MRBF_DS_NO_START;
        const double fill = nan_out ? QNAN : 0.0;
        for (int j = t; j < n; j += THREADS) dout[j] = fill;
        if (t < K) {
            cout[t] = fill;
            if (a.mult_out) a.mult_out[qp * K + t] = fill;
        }
        if (t == 0) a.omega_out[qp] = nan_out ? QNAN : (status == MRBF_DS_INFEASIBLE ? -INF : 0.0);
    }
    if (t == 0) {
        a.status_out[qp] = status;
        if (a.iters_out) a.iters_out[2 * qp] = iters, a.iters_out[2 * qp + 1] = dropped;
    }
}

// all device pointers; QPs in chunks so that the per-QP workspaces stay below dcall::WS_LIMIT_BYTES.  QP p reads x at x + p x_stride and its
// bounds at lb / ub + p bound_stride (0: one box for every QP); everything else lies in consecutive per-QP blocks.
int launch(mrbf_ctx *ctx, int64_t n_qp, int n, int k, int meq, int min, const double *G, const double *r, const double *x, int64_t x_stride,
           const double *lb, const double *ub, int64_t bound_stride, const double *Aeq, const double *beq, const double *Ain,
           const double *bin, double *d_out, double *c_out, double *omega_out, double *mult_out, int *status_out, int *iters_out) {
    Args a;
    a.n = n, a.k = k, a.meq = meq, a.min = min, a.xs = x_stride, a.bs = bound_stride;
    a.G = G, a.r = r, a.x = x, a.lb = lb, a.ub = ub, a.Aeq = Aeq, a.beq = beq, a.Ain = Ain, a.bin = bin;
    a.d_out = d_out, a.c_out = c_out, a.omega_out = omega_out, a.mult_out = mult_out, a.status_out = status_out, a.iters_out = iters_out;
    const int64_t per = dcall::chunk(n_qp, ws_bytes(n));
    MRBF_TRY(get_buf(ctx, S_DS_WS, (size_t)per * ws_doubles(n), &a.ws));
    MRBF_TRY(get_buf(ctx, S_DS_WSI, (size_t)per * ws_ints(n), &a.wsi));
    const size_t shm = carve(k + meq + min).total;
    for (int64_t q0 = 0; q0 < n_qp; q0 += per) {
        const unsigned grid = (unsigned)std::min<int64_t>(per, n_qp - q0);
        hipLaunchKernelGGL(ds_qp_rows_kernel, dim3(grid), dim3(THREADS), shm, ctx->stream, a, q0);
        MRBF_HIP(ctx, hipGetLastError());
    }
    return 0;
}

}  // namespace rows
}  // namespace ds
}  // namespace mrbf

using namespace mrbf;

// descent.jl:196-236 and :598-645: the direction QP of directed search with constraint rows for n_qp starts in one launch
extern "C" int32_t mrbf_ds_direction_rows(mrbf_ctx *ctx, int64_t n_qp, int32_t d, int32_t k, int32_t m_eq, int32_t m_in, const double *G,
                                          const double *r, const double *x, const double *lb, const double *ub, const double *A_eq,
                                          const double *b_eq, const double *A_in, const double *b_in, double *d_out, double *c_out,
                                          double *omega_out, double *mult_out, int32_t *status_out, int32_t *iters_out) {
    ds::rows::Call c;
    c.has_ctx = ctx != nullptr, c.n_qp = n_qp, c.d = d, c.k = k, c.m_eq = m_eq, c.m_in = m_in;
    c.G = G != nullptr, c.r = r != nullptr, c.x = x != nullptr, c.lb = lb != nullptr, c.ub = ub != nullptr;
    c.A_eq = A_eq != nullptr, c.b_eq = b_eq != nullptr, c.A_in = A_in != nullptr, c.b_in = b_in != nullptr;
    c.d_out = d_out != nullptr, c.c_out = c_out != nullptr, c.omega_out = omega_out != nullptr, c.status_out = status_out != nullptr;
    if (const int rc = ds::rows::validate(c))
        return rc == -1 ? -1 : fail(ctx, rc, "mrbf_ds_direction_rows: invalid argument (n_qp = %lld, d = %d (1..%d), k = %d, m_eq = %d, m_in = %d (k >= 1, at most %d rows), or a NULL array)", (long long)n_qp, d, ds::MAXD, k, m_eq, m_in, ds::MAXK);
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    const size_t N = (size_t)n_qp, K = (size_t)k + m_eq + m_in;
    double *arena;
    MRBF_TRY(get_buf(ctx, S_DS_IN, N * ds::rows::input_doubles(d, k, m_eq, m_in), &arena));
    const double *dG, *dr, *dx, *dlb, *dub, *dAeq, *dbeq, *dAin, *dbin;
    MRBF_TRY(input_view(ctx, G, N * k * d, arena, &dG));
    MRBF_TRY(input_view(ctx, r, N * k, arena, &dr));
    MRBF_TRY(input_view(ctx, x, N * d, arena, &dx));
    MRBF_TRY(input_view(ctx, lb, N * d, arena, &dlb));
    MRBF_TRY(input_view(ctx, ub, N * d, arena, &dub));
    MRBF_TRY(input_view(ctx, A_eq, N * m_eq * d, arena, &dAeq));
    MRBF_TRY(input_view(ctx, b_eq, N * m_eq, arena, &dbeq));
    MRBF_TRY(input_view(ctx, A_in, N * m_in * d, arena, &dAin));
    MRBF_TRY(input_view(ctx, b_in, N * m_in, arena, &dbin));
    dcall::Outputs out;  // d, c, omega, mult, status, iterations
    MRBF_TRY(out.open(ctx, S_DS_OUT, {{d_out, N * d, false}, {c_out, N * K, false}, {omega_out, N, false}, {mult_out, N * K, false}, {status_out, N, true}, {iters_out, 2 * N, true}}));
    MRBF_TRY(ds::rows::launch(ctx, n_qp, d, k, m_eq, m_in, dG, dr, dx, d, dlb, dub, d, dAeq, dbeq, dAin, dbin, out.at<double>(0), out.at<double>(1), out.at<double>(2), out.at<double>(3), out.at<int>(4), out.at<int>(5)));
    MRBF_TRY(out.copy_back(ctx));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    return MRBF_OK;
}

// descent.jl:196-236 and :598-645: the criticality of directed search for a container with constraint rows -- values and Jacobians at
// [x_n; x] through the evaluation kernels, the rows of get_criticality by sd_lp.hip's assembly, one direction QP, one read-back
extern "C" int32_t mrbf_ds_criticality_rows(mrbf_ctx *ctx, const mrbf_ps_problem *prob, const double *x, const double *x_n, const double *lb,
                                            const double *ub, const double *r, double *d_out, double *mult_out, mrbf_ds_info *info) {
    if (!ctx) return -1;
    if (!prob) return fail(ctx, -3, "problem is NULL");
    if (!x) return fail(ctx, -4, "x is NULL");
    if (!x_n) return fail(ctx, -5, "x_n is NULL");
    if (!lb) return fail(ctx, -6, "lb is NULL");
    if (!ub) return fail(ctx, -7, "ub is NULL");
    if (!r) return fail(ctx, -8, "r is NULL");
    if (!d_out) return fail(ctx, -9, "d_out is NULL");
    if (!info) return fail(ctx, -11, "info is NULL");
    std::memset(info, 0, sizeof(*info));
    if (prob->n_models < 1 || !prob->models || !prob->roles) return fail(ctx, -2, "mrbf_ds_criticality_rows: grouped models with a roles table are required");
    std::vector<descent::SlotShape> slots;
    descent::Layout lay;
    if (descent::Defect D = descent::read(descent_shape(prob, prob->models, 1, slots), {true, descent::Centres::UNCHECKED}, lay))
        return fail(ctx, -2, "mrbf_ds_criticality_rows: %s", D.msg.c_str());
    const int d = lay.d, k = prob->n_objectives, n_lin = prob->n_lin_eq + prob->n_lin_ineq;
    if (mrbf_dispatch_ds_rows(d, k, prob->n_models, lay.n_nl, n_lin, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_ds_criticality_rows: d = %d / k = %d / %d constraint rows outside the device path (ask mrbf_dispatch_ds_rows first)", d, k, lay.n_nl + n_lin);
    const descent::Offsets at = lay.offsets(2, descent::Slots::USED);
    const int64_t jtot = at.jtot, vtot = at.vtot;
    const int meq = lay.meq, min = lay.min, m = k + meq + min;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- host inputs, packed: [x_n; x] (the two evaluation sites), lb, ub, r, linear rows (eq, then ineq), their b
    dcall::PackedIn in;
    const size_t axn = in.fetch(ctx, x_n, d), ax = in.fetch(ctx, x, d), alb = in.fetch(ctx, lb, d), aub = in.fetch(ctx, ub, d);
    const size_t ar = in.fetch(ctx, r, k);
    const auto [aA, ab] = in.fetch_linear_rows(ctx, prob, d);
    MRBF_TRY(in.rc);
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, ctx->stream));
    // device arena: inputs | Jacobians | values | QP data (G, A_eq, b_eq, A_ineq, b_ineq) | outputs (d, c, omega, mult, 3 int words)
    const size_t qp_cnt = (size_t)k * d + (size_t)(meq + min) * (d + 1), out_dbl = (size_t)d + 2 * (size_t)m + 1, out_cnt = out_dbl + 2;
    double *base;
    MRBF_TRY(get_buf(ctx, S_DS_IN, in.total + jtot + vtot + qp_cnt + out_cnt, &base));
    double *dJ = base + in.total, *dV = dJ + jtot, *dG = dV + vtot, *dAeq = dG + (size_t)k * d, *dbeq = dAeq + (size_t)meq * d;
    double *dAin = dbeq + meq, *dbin = dAin + (size_t)min * d, *dout = dbin + min;
    MRBF_TRY(in.upload(ctx, base));
    const double *dxn = in.dev(axn), *dx = in.dev(ax), *dlb = in.dev(alb), *dub = in.dev(aub), *dr = in.dev(ar), *dA = in.dev(aA), *db = in.dev(ab);
    // ---- values and Jacobians of every used model at x_n and x: one sweep per model
    for (int j = 0; j < prob->n_models; ++j)
        if (lay.chosen(j, descent::Slots::USED)) MRBF_TRY(eval_model(ctx, prob->models[j], 2, dxn, dV + at.val[j], dJ + at.jac[j], nullptr));
    // ---- G, A_eq / b_eq (linear, then modelled), A_ineq / b_ineq (likewise): the assembly of mrbf_sd_criticality
    sd::AsmArgs aa;
    aa.n = d, aa.k = k, aa.rows = m, aa.meq = meq, aa.min = min;
    aa.sJ = aa.sV = aa.sx = 0;  // one start
    aa.J = dJ, aa.V = dV, aa.xn = dxn, aa.x = dx, aa.Alin = dA, aa.blin = db;
    aa.G = dG, aa.Aeq = dAeq, aa.beq = dbeq, aa.Ain = dAin, aa.bin = dbin;
    descent::fill_sources(lay, at, true, aa.src);
    MRBF_TRY(sd::launch_assemble(ctx, aa, 1));
    int *oi = reinterpret_cast<int *>(dout + out_dbl);
    MRBF_TRY(ds::rows::launch(ctx, 1, d, k, meq, min, dG, dr, dxn, 0, dlb, dub, 0, dAeq, dbeq, dAin, dbin, dout, dout + d, dout + d + m,
                              dout + d + m + 1, oi, oi + 1));
    // ---- one read-back
    std::vector<double> hout(out_cnt);
    MRBF_HIP(ctx, hipMemcpyAsync(hout.data(), dout, out_cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MRBF_HIP(ctx, hipEventRecord(e1, ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    MRBF_HIP(ctx, hipEventElapsedTime(&info->ms_total, e0, e1));
    dcall::read_status(hout.data() + out_dbl, &info->status, &info->iterations, &info->dropped);
    info->omega = hout[d + m];
    MRBF_TRY(output_put(ctx, d_out, hout.data(), d));
    if (mult_out) MRBF_TRY(output_put(ctx, mult_out, hout.data() + d + m + 1, m));
    if (info->status == MRBF_DS_GAVE_UP) return fail(ctx, -2, "mrbf_ds_criticality_rows: the direction QP gave up (take the host method)");
    if (info->status == MRBF_DS_NO_START) return fail(ctx, -2, "mrbf_ds_criticality_rows: d = 0 misses a constraint row (take the host method)");
    return MRBF_OK;
}
