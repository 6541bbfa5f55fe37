// Steepest-descent criticality on the device: the direction LP of _steepest_descent_direction (src/descent.jl:91-135) and the whole
// get_criticality(::SteepestDescentConfig, ...) (descent.jl:187-241) around it.
//
// One workgroup solves one LP:
//   minimise alpha  s.t.  g_i . d - w_i alpha + s_i = 0 (i < k, s_i >= 0),  A_eq d + s = b_eq (s = 0),  A_ineq d + s = b_ineq (s >= 0),
//   l <= d <= u, alpha free
// by a dual simplex with the bound-flipping ratio test.  Columns: the d structural ones, alpha (column d), one slack per row (d + 1 + i).
// Start basis: alpha basic in the first objective row i0 with w_i0 > 0, every other slack basic, each d_j at the bound its reduced
// cost g_i0,j / w_i0 prefers -- dual feasible, so there is no phase I.  alpha is free, so it never leaves: the row duals are the row
// of B^-1 at alpha's position.  B^-1 (m x m, m <= 64) lives in LDS, takes a rank-1 update per pivot and is refactored (Gauss-Jordan
// with partial pivoting) every 16 pivots and before optimality is accepted.  The basic values and reduced costs are recomputed from
// B^-1 every iteration (one pass over the rows, one over the columns), so no update error accumulates in them.  Every sum runs in a
// fixed order that depends on the shape alone: an LP's result does not depend on its position in the batch, and no atomics touch
// values (the one LDS atomic only compacts the ratio-test candidates, which are then sorted by (breakpoint, column)).
#include "descent_call.hpp"
#include "lp_dev.hpp"
#include "sd.hpp"

namespace mrbf {
namespace sd {

static_assert(THREADS == lp::THREADS, "row_pass and invert run on a workgroup of lp::THREADS");

constexpr int REFACTOR_EVERY = 16;
constexpr double FEAS_TOL = 1e-13;   // relative to the row's magnitude sum |b_i| + sum_j |A_ij| (|d_j| <= 1)
constexpr double PIVOT_TOL = 1e-9;   // ratio-test candidates: |alpha_pj| > PIVOT_TOL * max_j |alpha_pj|
constexpr double SNAP_TOL = 1e-12;   // a basic d_j this close to a bound is returned on it

struct Args {
    int n, k, meq, min, m, normalize, nc, p2;
    int64_t xs, bs;  // LP p reads x at x + p xs and its bounds at lb / ub + p bs (0: one box for every LP)
    const double *G, *x, *lb, *ub, *Aeq, *beq, *Ain, *bin;
    double *d_out, *omega_out, *dual_out;
    int *status_out, *iters_out;
    double *ws;  // per LP 5 nc doubles: nonbasic values, lower, upper bounds, pivot row, reduced costs
    int *wsi;    // per LP nc ints: basis position of each column (-1: nonbasic)
};

struct Lp {
    const double *G, *Aeq, *Ain;
    int n, k, meq;
    __device__ double a(int i, int j) const {  // entry (row i, structural column j)
        if (i < k) return G[(size_t)j * k + i];
        if (i < k + meq) return Aeq[(size_t)(i - k) * n + j];
        return Ain[(size_t)(i - k - meq) * n + j];
    }
};

// LDS carve (host and device agree through this one function); offsets in bytes, each a multiple of 16
struct Carve {
    size_t binv, vec, part, dsc, head, isc, uni, total;
};
__host__ __device__ inline Carve carve(int m, int p2) {
    Carve c;
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    c.binv = 0;
    c.vec = up(c.binv + (size_t)m * m * sizeof(double));
    c.part = up(c.vec + (size_t)10 * MAXM * sizeof(double));
    c.dsc = up(c.part + (size_t)THREADS * sizeof(double));
    c.head = up(c.dsc + 8 * sizeof(double));
    c.isc = up(c.head + MAXM * sizeof(int));
    c.uni = up(c.isc + 16 * sizeof(int));
    const size_t sort = (size_t)p2 * (sizeof(double) + sizeof(int)), aug = (size_t)m * 2 * m * sizeof(double);
    c.total = up(c.uni + (sort > aug ? sort : aug));
    return c;
}

enum { I_ACT = 0, I_P, I_DIR, I_CNT, I_TE, I_PIV, I_BAD, I_I0 };
enum { A_PIVOT = 0, A_DONE, A_REFACTOR, A_GIVEUP, A_INFEASIBLE };
enum { D_SLOPE = 0, D_AMAX };

__device__ inline double col_entry(const Lp &L, const double *w, int col, int i) {
    if (col < L.n) return L.a(i, col);
    if (col == L.n) return i < L.k ? -w[i] : 0.0;
    return i == col - L.n - 1 ? 1.0 : 0.0;
}

// B^-1 from scratch: Gauss-Jordan with partial pivoting on [B | I] (m x 2m in the union area).  false: B is singular.
__device__ bool refactor(const Lp &L, int m, const double *w, const int *head, double *Binv, double *aug, double *rowbuf, double *fac,
                         double *cmax, int *isc) {
    const int t = threadIdx.x, W = 2 * m;
    for (int e = t; e < m * W; e += THREADS) {
        const int r = e / W, c = e % W;
        aug[e] = c < m ? col_entry(L, w, head[c], r) : (c - m == r ? 1.0 : 0.0);
    }
    __syncthreads();
    return lp::invert(m, aug, Binv, rowbuf, fac, cmax, isc + I_PIV);
}

__global__ __launch_bounds__(THREADS) void sd_lp_kernel(Args a, int64_t lp0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t lp = lp0 + blockIdx.x;
    const int t = threadIdx.x, n = a.n, k = a.k, m = a.m, nc = a.nc, meq = a.meq;
    const Carve cv = carve(m, a.p2);
    double *Binv = (double *)(smem + cv.binv), *vec = (double *)(smem + cv.vec), *part = (double *)(smem + cv.part);
    double *rho = vec, *yv = vec + MAXM, *aq = vec + 2 * MAXM, *rhs = vec + 3 * MAXM, *beta = vec + 4 * MAXM, *w = vec + 5 * MAXM;
    double *bt = vec + 6 * MAXM, *ftol = vec + 7 * MAXM, *colq = vec + 8 * MAXM, *cmax = vec + 9 * MAXM;
    double *dsc = (double *)(smem + cv.dsc);
    int *head = (int *)(smem + cv.head), *isc = (int *)(smem + cv.isc);
    double *skey = (double *)(smem + cv.uni), *aug = skey;
    int *sidx = (int *)(smem + cv.uni + (size_t)a.p2 * sizeof(double));

    const Lp L{a.G + lp * k * n, a.Aeq ? a.Aeq + lp * meq * n : nullptr, a.Ain ? a.Ain + lp * a.min * n : nullptr, n, k, meq};
    const double *x = a.x + lp * a.xs, *lb = a.lb + lp * a.bs, *ub = a.ub + lp * a.bs;
    double *xv = a.ws + (size_t)blockIdx.x * 5 * nc, *lo = xv + nc, *hi = xv + 2 * nc, *ap = xv + 3 * nc, *dj = xv + 4 * nc;
    int *pos = a.wsi + (size_t)blockIdx.x * nc;
    const double INF = __builtin_huge_val();

    // ---- bounds, row weights, right-hand sides, row tolerances
    int bad = 0;
    for (int j = t; j < nc; j += THREADS) {
        double l, u;
        if (j < n) {
            l = fmax(-1.0, lb[j] - x[j]);
            u = fmin(1.0, ub[j] - x[j]);
            if (!(l <= u)) bad = 1;
        } else if (j == n) {
            l = -INF, u = INF;
        } else {
            const int i = j - n - 1;
            l = 0.0, u = (i >= k && i < k + meq) ? 0.0 : INF;
        }
        lo[j] = l, hi[j] = u, pos[j] = -1, xv[j] = 0.0;
    }
    bad = __syncthreads_or(bad);
    lp::row_pass(n, k, [&](int i, int j) { const double g = L.G[(size_t)j * k + i]; return g * g; }, part, w);
    lp::row_pass(n, m, [&](int i, int j) { return fabs(L.a(i, j)); }, part, ftol);
    if (t < m) {
        if (t < k) w[t] = a.normalize ? sqrt(w[t]) : 1.0;
        bt[t] = t < k ? 0.0 : (t < k + meq ? a.beq[lp * meq + t - k] : a.bin[lp * a.min + t - k - meq]);
        ftol[t] = FEAS_TOL * fmax(1.0, fabs(bt[t]) + ftol[t] + (t < k ? ftol[t] : 0.0));
    }
    __syncthreads();
    if (t == 0) {
        int i0 = -1;
        for (int i = 0; i < k && i0 < 0; ++i)
            if (w[i] > 0.0) i0 = i;
        isc[I_I0] = i0;
        isc[I_BAD] = bad ? MRBF_SD_INFEASIBLE : (i0 < 0 ? MRBF_SD_NO_OBJECTIVE : MRBF_SD_OK);
    }
    __syncthreads();
    int status = isc[I_BAD];
    const int i0 = isc[I_I0];
    int iters = 0, flips = 0;
    if (status == MRBF_SD_OK) {
        // ---- start basis (dual feasible)
        for (int j = t; j < n; j += THREADS) {
            const double r = L.G[(size_t)j * k + i0];
            xv[j] = r > 0.0 ? lo[j] : (r < 0.0 ? hi[j] : (fabs(lo[j]) <= fabs(hi[j]) ? lo[j] : hi[j]));
        }
        if (t < m) {
            head[t] = t == i0 ? n : n + 1 + t;
            pos[head[t]] = t;
        }
        __syncthreads();
        if (!refactor(L, m, w, head, Binv, aug, part, colq, cmax, isc)) status = MRBF_SD_GAVE_UP;
        const int cap = 8 * (m + n);
        int since = 0;
        while (status == MRBF_SD_OK) {
            // ---- basic values beta = B^-1 (b - N x_N): only structural columns carry non-zero nonbasic values
            lp::row_pass(n, m, [&](int i, int j) { return pos[j] < 0 ? L.a(i, j) * xv[j] : 0.0; }, part, rhs);
            if (t < m) {
                double acc = 0.0;
                for (int q = 0; q < m; ++q) acc += Binv[t * m + q] * (bt[q] - rhs[q]);
                beta[t] = acc;
            }
            __syncthreads();
            // ---- pricing: the largest violation, ties to the lowest basis position
            if (t == 0) {
                int best = -1, dir = 0;
                double bv = 0.0;
                for (int p = 0; p < m; ++p) {
                    const int v = head[p];
                    const double tol = v < n ? FEAS_TOL : (v == n ? INF : ftol[v - n - 1]);
                    double viol = 0.0;
                    int dd = 0;
                    if (beta[p] < lo[v] - tol) viol = lo[v] - beta[p], dd = -1;
                    else if (beta[p] > hi[v] + tol) viol = beta[p] - hi[v], dd = 1;
                    if (viol > bv) bv = viol, best = p, dir = dd;
                }
                int act = A_PIVOT;
                if (best < 0) act = since > 0 ? A_REFACTOR : A_DONE;
                else if (iters >= cap) act = A_GIVEUP;
                isc[I_ACT] = act, isc[I_P] = best, isc[I_DIR] = dir, isc[I_CNT] = 0;
                dsc[D_SLOPE] = bv;
            }
            __syncthreads();
            const int act = isc[I_ACT];
            if (act == A_DONE) break;
            if (act == A_GIVEUP) {
                status = MRBF_SD_GAVE_UP;
                break;
            }
            if (act == A_REFACTOR) {
                since = 0;
                if (!refactor(L, m, w, head, Binv, aug, part, colq, cmax, isc)) status = MRBF_SD_GAVE_UP;
                continue;
            }
            ++iters;
            const int p = isc[I_P], dir = isc[I_DIR];
            const double slope0 = dsc[D_SLOPE];
            if (t < m) rho[t] = Binv[p * m + t], yv[t] = Binv[i0 * m + t];
            __syncthreads();
            // ---- pivot row alpha_p = e_p' B^-1 A and reduced costs d_j = c_j - y' A_j over all nonbasic columns
            double amax = 0.0;
            for (int j = t; j < nc; j += THREADS) {
                if (pos[j] >= 0) continue;
                double sy = 0.0, sr = 0.0;
                if (j < n) {
                    for (int i = 0; i < m; ++i) {
                        const double aij = L.a(i, j);
                        sy += aij * yv[i], sr += aij * rho[i];
                    }
                } else if (j == n) {
                    for (int i = 0; i < k; ++i) sy -= w[i] * yv[i], sr -= w[i] * rho[i];
                } else {
                    sy = yv[j - n - 1], sr = rho[j - n - 1];
                }
                const double ah = dir < 0 ? -sr : sr;
                ap[j] = ah, dj[j] = (j == n ? 1.0 : 0.0) - sy;
                if (lo[j] < hi[j]) amax = fmax(amax, fabs(ah));
            }
            part[t] = amax;
            __syncthreads();
            for (int s = THREADS / 2; s > 0; s >>= 1) {
                if (t < s) part[t] = fmax(part[t], part[t + s]);
                __syncthreads();
            }
            const double ptol = PIVOT_TOL * part[0];
            // ---- breakpoints of the dual step: compacted (index only), then sorted by (breakpoint, column)
            for (int j = t; j < nc; j += THREADS) {
                if (pos[j] >= 0 || !(lo[j] < hi[j])) continue;
                const double ah = ap[j];
                const bool at_lo = xv[j] == lo[j];
                if (at_lo ? ah > ptol : ah < -ptol) {
                    const int slot = atomicAdd(&isc[I_CNT], 1);
                    skey[slot] = at_lo ? fmax(dj[j], 0.0) / ah : fmin(dj[j], 0.0) / ah;
                    sidx[slot] = j;
                }
            }
            __syncthreads();
            const int cnt = isc[I_CNT];
            if (cnt == 0) {
                status = MRBF_SD_INFEASIBLE;  // dual unbounded
                break;
            }
            int P2 = 1;
            while (P2 < cnt) P2 <<= 1;
            for (int e = cnt + t; e < P2; e += THREADS) skey[e] = INF, sidx[e] = 0x7fffffff;
            __syncthreads();
            for (int size = 2; size <= P2; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int e = t; e < P2 / 2; e += THREADS) {
                        const int i = (e / stride) * 2 * stride + e % stride, jj = i + stride;
                        const bool up = (i & size) == 0;
                        const double ka = skey[i], kb = skey[jj];
                        const int ia = sidx[i], ib = sidx[jj];
                        const bool gt = ka > kb || (ka == kb && ia > ib);
                        if (gt == up) skey[i] = kb, skey[jj] = ka, sidx[i] = ib, sidx[jj] = ia;
                    }
                    __syncthreads();
                }
            // ---- the slope walk: every boxed breakpoint passed is flipped; the one that turns the slope enters
            const int chunk = (cnt + THREADS - 1) / THREADS;
            {
                double acc = 0.0;
                for (int e = t * chunk; e < min(cnt, (t + 1) * chunk); ++e) {
                    const int j = sidx[e];
                    acc += fabs(ap[j]) * (hi[j] - lo[j]);
                }
                part[t] = acc;
            }
            __syncthreads();
            if (t == 0) {
                double run = 0.0;
                int te = -1;
                for (int c = 0; c < THREADS && te < 0; ++c) {
                    if (run + part[c] < slope0) {
                        run += part[c];
                        continue;
                    }
                    for (int e = c * chunk; e < min(cnt, (c + 1) * chunk); ++e) {
                        const int j = sidx[e];
                        run += fabs(ap[j]) * (hi[j] - lo[j]);
                        if (run >= slope0) {
                            te = e;
                            break;
                        }
                    }
                }
                isc[I_TE] = te;
            }
            __syncthreads();
            const int te = isc[I_TE];
            if (te < 0) {
                status = MRBF_SD_INFEASIBLE;
                break;
            }
            for (int e = t; e < te; e += THREADS) {
                const int j = sidx[e];
                xv[j] = xv[j] == lo[j] ? hi[j] : lo[j];
            }
            flips += te;
            const int q = sidx[te];
            // ---- FTRAN of the entering column and the rank-1 update of B^-1
            if (t < m) colq[t] = col_entry(L, w, q, t);
            __syncthreads();
            if (t < m) {
                double acc = 0.0;
                for (int c = 0; c < m; ++c) acc += Binv[t * m + c] * colq[c];
                aq[t] = acc;
            }
            __syncthreads();
            const double piv = aq[p];
            if (!(fabs(piv) > 0.0)) {
                status = MRBF_SD_GAVE_UP;
                break;
            }
            if (t < m) part[t] = Binv[p * m + t] / piv;
            __syncthreads();
            for (int e = t; e < m * m; e += THREADS) {
                const int i = e / m, c = e % m;
                Binv[e] = i == p ? part[c] : Binv[e] - aq[i] * part[c];
            }
            if (t == 0) {
                const int v = head[p];
                xv[v] = dir < 0 ? lo[v] : hi[v];
                pos[v] = -1;
                pos[q] = p;
                head[p] = q;
            }
            __syncthreads();
            if (++since >= REFACTOR_EVERY) {
                since = 0;
                if (!refactor(L, m, w, head, Binv, aug, part, colq, cmax, isc)) status = MRBF_SD_GAVE_UP;
            }
        }
    }
    // ---- outputs
    double *dout = a.d_out + lp * n;
    if (status == MRBF_SD_OK || status == MRBF_SD_GAVE_UP) {
        for (int j = t; j < n; j += THREADS) {
            double v = xv[j];
            if (pos[j] >= 0) {
                v = fmin(fmax(beta[pos[j]], lo[j]), hi[j]);
                if (v - lo[j] <= SNAP_TOL) v = lo[j];
                if (hi[j] - v <= SNAP_TOL) v = hi[j];
            }
            dout[j] = v;
            dj[j] = v;
        }
        __syncthreads();
        lp::row_pass(n, k, [&](int i, int j) { return L.G[(size_t)j * k + i] * dj[j]; }, part, rhs);
        if (t == 0) {
            double mx = -INF;
            for (int i = 0; i < k; ++i)
                if (w[i] > 0.0) mx = fmax(mx, rhs[i] / w[i]);
            a.omega_out[lp] = -mx;
        }
        if (a.dual_out && t < m) a.dual_out[lp * m + t] = -Binv[i0 * m + t];
    } else {
        for (int j = t; j < n; j += THREADS) dout[j] = 0.0;
        if (t == 0) a.omega_out[lp] = -INF;
        if (a.dual_out && t < m) a.dual_out[lp * m + t] = 0.0;
    }
    if (t == 0) {
        a.status_out[lp] = status;
        if (a.iters_out) a.iters_out[2 * lp] = iters, a.iters_out[2 * lp + 1] = flips;
    }
}

// ---- get_criticality's right-hand sides (RowSrc, AsmArgs: sd.hpp): one workgroup per LP row and start
__global__ __launch_bounds__(THREADS) void sd_assemble_kernel(AsmArgs a) {
    __shared__ double part[THREADS];
    const RowSrc s = a.src[blockIdx.x];
    const int t = threadIdx.x, n = a.n;
    // ---- this start's arrays (the linear rows are shared)
    const int64_t p = blockIdx.y;
    a.J += p * a.sJ, a.V += p * a.sV, a.xn += p * a.sx, a.x += p * a.sx;
    a.G += p * a.k * n, a.Aeq += p * a.meq * n, a.beq += p * a.meq, a.Ain += p * a.min * n, a.bin += p * a.min;
    if (s.kind == 0) {
        for (int j = t; j < n; j += THREADS) a.G[(size_t)j * a.k + s.dst] = a.J[s.jac + (int64_t)j * s.stride];
        return;
    }
    double *row = (s.eq ? a.Aeq : a.Ain) + (size_t)s.dst * n;
    const double *src = s.kind == 1 ? a.Alin + s.val * n : a.J + s.jac + (int64_t)s.stride * n;  // modelled: point 1 (x)
    const int64_t step = s.kind == 1 ? 1 : s.stride;
    double acc = 0.0;
    for (int j = t; j < n; j += THREADS) {
        const double v = src[j * step];
        row[j] = v;
        acc += v * (s.kind == 1 ? a.xn[j] : a.xn[j] - a.x[j]);
    }
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int i = 0; i < THREADS; ++i) sum += part[i];
        (s.eq ? a.beq : a.bin)[s.dst] = s.kind == 1 ? a.blin[s.val] - sum : -a.V[s.val] - sum;
    }
}

int launch_assemble(mrbf_ctx *ctx, const AsmArgs &a, int64_t n_starts) {
    hipLaunchKernelGGL(sd_assemble_kernel, dim3((unsigned)a.rows, (unsigned)n_starts), dim3(THREADS), 0, ctx->stream, a);
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}

// all device pointers; LPs in chunks so that the per-LP workspace stays below 256 MB (strides: sd.hpp)
int launch(mrbf_ctx *ctx, int64_t n_lp, int n, int k, int meq, int min, int normalize, const double *G, const double *x, int64_t x_stride,
           const double *lb, const double *ub, int64_t bound_stride, const double *Aeq, const double *beq, const double *Ain,
           const double *bin, double *d_out, double *omega_out, double *dual_out, int *status_out, int *iters_out) {
    Args a;
    a.xs = x_stride, a.bs = bound_stride;
    a.n = n, a.k = k, a.meq = meq, a.min = min, a.m = k + meq + min, a.normalize = normalize != 0;
    a.nc = n + 1 + a.m;
    a.p2 = 1;
    while (a.p2 < a.nc) a.p2 <<= 1;
    a.G = G, a.x = x, a.lb = lb, a.ub = ub, a.Aeq = Aeq, a.beq = beq, a.Ain = Ain, a.bin = bin;
    a.d_out = d_out, a.omega_out = omega_out, a.dual_out = dual_out, a.status_out = status_out, a.iters_out = iters_out;
    const int64_t chunk = dcall::chunk(n_lp, (size_t)a.nc * (5 * sizeof(double) + sizeof(int)));
    MRBF_TRY(get_buf(ctx, S_SD_WS, (size_t)chunk * a.nc * 5, &a.ws));
    MRBF_TRY(get_buf(ctx, S_SD_OUT, (size_t)chunk * a.nc, &a.wsi));
    const size_t shm = carve(a.m, a.p2).total;
    MRBF_HIP(ctx, hipFuncSetAttribute((const void *)sd_lp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    for (int64_t lp0 = 0; lp0 < n_lp; lp0 += chunk) {
        const unsigned grid = (unsigned)std::min<int64_t>(chunk, n_lp - lp0);
        hipLaunchKernelGGL(sd_lp_kernel, dim3(grid), dim3(THREADS), shm, ctx->stream, a, lp0);
        MRBF_HIP(ctx, hipGetLastError());
    }
    return 0;
}

}  // namespace sd
}  // namespace mrbf

using namespace mrbf;

extern "C" int32_t mrbf_sd_direction(mrbf_ctx *ctx, int64_t n_lp, int32_t d, int32_t k, int32_t m_eq, int32_t m_ineq, const double *G,
                                     const double *x, const double *lb, const double *ub, const double *A_eq, const double *b_eq,
                                     const double *A_ineq, const double *b_ineq, int32_t normalize, double *d_out, double *omega_out,
                                     double *dual_out, int32_t *status_out, int32_t *iters_out) {
    if (!ctx) return -1;
    if (n_lp < 0) return fail(ctx, -2, "n_lp < 0");
    if (d < 1 || d > sd::MAXD) return fail(ctx, -3, "d = %d out of range (1..%d)", d, sd::MAXD);
    if (k < 1) return fail(ctx, -4, "k = %d: at least one objective row", k);
    if (m_eq < 0) return fail(ctx, -5, "m_eq < 0");
    if (m_ineq < 0) return fail(ctx, -6, "m_ineq < 0");
    if ((int64_t)k + m_eq + m_ineq > sd::MAXM) return fail(ctx, -4, "k + m_eq + m_ineq = %d rows (at most %d)", k + m_eq + m_ineq, sd::MAXM);
    if (!G) return fail(ctx, -7, "G is NULL");
    if (!x) return fail(ctx, -8, "x is NULL");
    if (!lb) return fail(ctx, -9, "lb is NULL");
    if (!ub) return fail(ctx, -10, "ub is NULL");
    if (m_eq && !A_eq) return fail(ctx, -11, "A_eq is NULL");
    if (m_eq && !b_eq) return fail(ctx, -12, "b_eq is NULL");
    if (m_ineq && !A_ineq) return fail(ctx, -13, "A_ineq is NULL");
    if (m_ineq && !b_ineq) return fail(ctx, -14, "b_ineq is NULL");
    if (!d_out) return fail(ctx, -16, "d_out is NULL");
    if (!omega_out) return fail(ctx, -17, "omega_out is NULL");
    if (!status_out) return fail(ctx, -19, "status_out is NULL");
    if (n_lp == 0) return MRBF_OK;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    const int m = k + m_eq + m_ineq;
    const size_t N = (size_t)n_lp;
    const size_t in_cnt = N * ((size_t)k * d + 3 * (size_t)d + (size_t)(m_eq + m_ineq) * (d + 1));
    double *arena;
    MRBF_TRY(get_buf(ctx, S_SD_IN, in_cnt, &arena));
    const double *dG, *dx, *dlb, *dub, *dAeq, *dbeq, *dAin, *dbin;
    MRBF_TRY(input_view(ctx, G, N * k * d, arena, &dG));
    MRBF_TRY(input_view(ctx, x, N * d, arena, &dx));
    MRBF_TRY(input_view(ctx, lb, N * d, arena, &dlb));
    MRBF_TRY(input_view(ctx, ub, N * d, arena, &dub));
    MRBF_TRY(input_view(ctx, A_eq, N * m_eq * d, arena, &dAeq));
    MRBF_TRY(input_view(ctx, b_eq, N * m_eq, arena, &dbeq));
    MRBF_TRY(input_view(ctx, A_ineq, N * m_ineq * d, arena, &dAin));
    MRBF_TRY(input_view(ctx, b_ineq, N * m_ineq, arena, &dbin));
    dcall::Outputs out;  // d, omega, dual, status, iterations
    MRBF_TRY(out.open(ctx, S_STAGE_D, {{d_out, N * d, false}, {omega_out, N, false}, {dual_out, N * m, false}, {status_out, N, true}, {iters_out, 2 * N, true}}));
    MRBF_TRY(sd::launch(ctx, n_lp, d, k, m_eq, m_ineq, normalize, dG, dx, d, dlb, dub, d, dAeq, dbeq, dAin, dbin, out.at<double>(0), out.at<double>(1), out.at<double>(2), out.at<int>(3), out.at<int>(4)));
    MRBF_TRY(out.copy_back(ctx));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    return MRBF_OK;
}

extern "C" int32_t mrbf_sd_criticality(mrbf_ctx *ctx, const mrbf_ps_problem *prob, const double *x, const double *x_n, const double *lb,
                                       const double *ub, int32_t normalize, double *d_out, double *dual_out, mrbf_sd_info *info) {
    if (!ctx) return -1;
    if (!prob) return fail(ctx, -2, "problem is NULL");
    if (!x) return fail(ctx, -3, "x is NULL");
    if (!x_n) return fail(ctx, -4, "x_n is NULL");
    if (!lb) return fail(ctx, -5, "lb is NULL");
    if (!ub) return fail(ctx, -6, "ub is NULL");
    if (!d_out) return fail(ctx, -8, "d_out is NULL");
    if (!info) return fail(ctx, -10, "info is NULL");
    std::memset(info, 0, sizeof(*info));
    if (prob->n_models < 1 || !prob->models || !prob->roles) return fail(ctx, -2, "mrbf_sd_criticality: grouped models with a roles table are required");
    // ---- the rows of the LP from the roles table; the evaluations at [x_n; x] of every used model
    std::vector<descent::SlotShape> slots;
    descent::Layout lay;
    if (descent::Defect D = descent::read(descent_shape(prob, prob->models, 1, slots), {true, descent::Centres::UNCHECKED}, lay))
        return fail(ctx, -2, "mrbf_sd_criticality: %s", D.msg.c_str());
    const int d = lay.d, k = prob->n_objectives, n_lin = prob->n_lin_eq + prob->n_lin_ineq;
    if (mrbf_dispatch_sd(d, k, prob->n_models, lay.n_nl, n_lin, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_sd_criticality: d = %d / k = %d / %d rows outside the device path (ask mrbf_dispatch_sd first)", d, k, k + lay.n_nl + n_lin);
    const descent::Offsets at = lay.offsets(2, descent::Slots::USED);
    const int64_t jtot = at.jtot, vtot = at.vtot;
    const int meq = lay.meq, min = lay.min, m = k + meq + min;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- host inputs, packed: [x_n; x] (the two evaluation sites), lb, ub, linear rows (eq, then ineq), their b
    dcall::PackedIn in;
    const size_t axn = in.fetch(ctx, x_n, d), ax = in.fetch(ctx, x, d), alb = in.fetch(ctx, lb, d), aub = in.fetch(ctx, ub, d);
    const auto [aA, ab] = in.fetch_linear_rows(ctx, prob, d);
    MRBF_TRY(in.rc);
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, ctx->stream));
    // device arena: inputs | Jacobians | values | LP data (G, A_eq, b_eq, A_ineq, b_ineq) | outputs (d, omega, dual, 3 int words)
    const size_t lp_cnt = (size_t)k * d + (size_t)(meq + min) * (d + 1), out_dbl = (size_t)d + 1 + m, out_cnt = out_dbl + 2;
    double *base;
    MRBF_TRY(get_buf(ctx, S_SD_IN, in.total + jtot + vtot + lp_cnt + out_cnt, &base));
    double *dJ = base + in.total, *dV = dJ + jtot, *dG = dV + vtot, *dAeq = dG + (size_t)k * d, *dbeq = dAeq + (size_t)meq * d;
    double *dAin = dbeq + meq, *dbin = dAin + (size_t)min * d, *dout = dbin + min;
    MRBF_TRY(in.upload(ctx, base));
    const double *dxn = in.dev(axn), *dx = in.dev(ax), *dlb = in.dev(alb), *dub = in.dev(aub), *dA = in.dev(aA), *db = in.dev(ab);
    // ---- values and Jacobians of every model at x_n and x: one sweep per model
    for (int j = 0; j < prob->n_models; ++j)
        if (lay.chosen(j, descent::Slots::USED)) MRBF_TRY(eval_model(ctx, prob->models[j], 2, dxn, dV + at.val[j], dJ + at.jac[j], nullptr));
    // ---- assemble G, A_eq / b_eq (linear, then modelled), A_ineq / b_ineq (likewise) on the device
    sd::AsmArgs aa;
    aa.n = d, aa.k = k, aa.rows = m, aa.meq = meq, aa.min = min;
    aa.sJ = aa.sV = aa.sx = 0;  // one start
    aa.J = dJ, aa.V = dV, aa.xn = dxn, aa.x = dx, aa.Alin = dA, aa.blin = db;
    aa.G = dG, aa.Aeq = dAeq, aa.beq = dbeq, aa.Ain = dAin, aa.bin = dbin;
    descent::fill_sources(lay, at, true, aa.src);
    MRBF_TRY(sd::launch_assemble(ctx, aa, 1));
    int *oi = reinterpret_cast<int *>(dout + out_dbl);
    MRBF_TRY(sd::launch(ctx, 1, d, k, meq, min, normalize, dG, dxn, 0, dlb, dub, 0, meq ? dAeq : nullptr, meq ? dbeq : nullptr,
                        min ? dAin : nullptr, min ? dbin : nullptr, dout, dout + d, dout + d + 1, oi, oi + 1));
    // ---- one read-back
    std::vector<double> hout(out_cnt);
    MRBF_HIP(ctx, hipMemcpyAsync(hout.data(), dout, out_cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MRBF_HIP(ctx, hipEventRecord(e1, ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    MRBF_HIP(ctx, hipEventElapsedTime(&info->ms_total, e0, e1));
    dcall::read_status(hout.data() + out_dbl, &info->status, &info->iterations, &info->bound_flips);
    info->omega = hout[d];
    MRBF_TRY(output_put(ctx, d_out, hout.data(), d));
    if (dual_out) MRBF_TRY(output_put(ctx, dual_out, hout.data() + d + 1, m));
    if (info->status == MRBF_SD_GAVE_UP) return fail(ctx, -2, "mrbf_sd_criticality: the direction LP gave up (take the reference method)");
    return MRBF_OK;
}
