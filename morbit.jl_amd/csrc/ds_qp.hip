// Directed search on the device: the direction QP of the reference's parked compute_descent_step(::Val{:ds}, ...) (src/descent.jl:583-664)
// and the criticality call around it.
//
// One workgroup solves one QP:
//   minimise 1/2 ||G d - r||^2  s.t.  l <= d <= u (the box of sd_lp.hip),  G d <= 0 (descent.jl:635-639)
// by a primal active-set method with minimum-norm steps.  d starts at 0 with an empty row set S and every variable whose box ends at 0 on
// that bound.  With N the free variables, M = G_N G_N' (k x k) and rho = r - G d, a step is p_N = G_N' a with dz = M a: zero on the rows
// of S (exactly: -z_S, so that the rows of S do not drift) and nearest to rho on the others.  M is factorised by a Cholesky whose pivots
// come from S first, so that "dz_S = 0" fixes the leading coefficients and the rest is a triangular solve (or, where a row outside S
// depends on others, the normal equations of the remaining columns): nothing larger than k x k is factorised, by one thread, in LDS.  A
// row of S that the factorisation finds dependent leaves S, so the working set stays independent.  The ratio test runs over the free
// variables' bounds and the rows outside S; what blocks joins the working set, a variable with its bound's bits.  Where the step
// vanishes, or after two unblocked full steps (the second refines the first), the multipliers mu_S and s = G' (z - r + mu) are formed
// and the most violating one is dropped (a row on ties with a variable, then the lowest index); none: optimal.  After a step of length
// zero -- a degenerate point, where more constraints meet than the working set holds -- the least index decides instead, rows before
// variables, for the one constraint that is added and the one that is dropped (Bland's rule), until a step moves again.  M is
// recomputed from G whenever N changes.  Every sum runs in an order fixed by the shape; no atomics.
#include "descent_call.hpp"
#include "ds.hpp"
#include "ds_dev.hpp"
#include "lp_dev.hpp"

namespace mrbf {
namespace ds {

static_assert(THREADS == lp::THREADS, "row_pass runs on a workgroup of lp::THREADS");

struct Args {
    int n, k;
    int64_t xs, bs;  // QP p reads x at x + p xs and its bounds at lb / ub + p bs (0: one box for every QP)
    const double *G, *r, *x, *lb, *ub;
    double *d_out, *z_out, *omega_out, *mult_out;
    int *status_out, *iters_out;
    double *ws;  // per QP 4 n doubles: d, p, l, u
    int *wsi;    // per QP n ints: 0 free, -1 on the lower bound, +1 on the upper bound, 2 fixed (l = u)
};

// M = G_N G_N' from G, whenever N changes: a rank-one downdate would cancel against the columns that have left (an entry of M falls by
// orders of magnitude while its error stays), and a pass over the free columns costs k times a pass for p.  Entry (i, i2) and entry
// (i2, i) add the same products in the same order: M is symmetric to the bit.
__device__ void refresh_M(const double *G, const int *flag, int n, int k, double *part, double *M) {
    lp::row_pass(n, k * k, [&](int e, int j) { return flag[j] == 0 ? G[(size_t)j * k + e / k] * G[(size_t)j * k + e % k] : 0.0; }, part, M);
}

__global__ __launch_bounds__(THREADS) void ds_qp_kernel(Args a, int64_t qp0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t qp = qp0 + blockIdx.x;
    const int t = threadIdx.x, n = a.n, k = a.k;
    const Carve cv = carve(k);
    Small sm;
    sm.k = k;
    sm.M = (double *)(smem + cv.M), sm.L = (double *)(smem + cv.L), sm.A = (double *)(smem + cv.A), sm.v = (double *)(smem + cv.vec);
    sm.piv = (int *)(smem + cv.ivec), sm.done = sm.piv + MAXK, sm.inS = sm.piv + 2 * MAXK;
    double *part = (double *)(smem + cv.part), *dsc = (double *)(smem + cv.dsc);
    int *ipart = (int *)(smem + cv.ipart), *isc = (int *)(smem + cv.isc);
    double *z = sm.vec(V_Z), *rho = sm.vec(V_RHO), *dz = sm.vec(V_DZ), *av = sm.vec(V_AV), *mu = sm.vec(V_MU), *rowsum = sm.vec(V_ROWSUM);
    double *rscale = sm.vec(V_RSCALE), *rv = sm.vec(V_R), *yv = sm.vec(V_Y), *ysc = sm.vec(V_YSC), *ar = sm.vec(V_AR);

    const double *G = a.G + qp * (int64_t)k * n, *x = a.x + qp * a.xs, *lb = a.lb + qp * a.bs, *ub = a.ub + qp * a.bs;
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
    lp::row_pass(n, k, [&](int i, int j) { return fabs(G[(size_t)j * k + i]); }, part, rowsum);
    if (t == 0) {
        int critical = 0;
        for (int i = 0; i < k; ++i) {
            const double ri = a.r[qp * k + i];
            if (!(ri < 0.0)) critical = 1;  // some r_i >= 0, or a NaN (descent.jl:615-617)
            rv[i] = ri, rscale[i] = rowsum[i] + fabs(ri), mu[i] = 0.0, sm.inS[i] = 0;
        }
        // the start d = 0 outside a non-empty box (x outside [lb, ub] by less than one): the method has no feasible start
        isc[I_BAD] = critical ? MRBF_DS_CRITICAL : (empty ? MRBF_DS_INFEASIBLE : (outside ? MRBF_DS_GAVE_UP : MRBF_DS_OK));
    }
    __syncthreads();
    int status = isc[I_BAD];
    int iters = 0, dropped = 0, full = 0, degen = 0;
    if (status == MRBF_DS_OK) {
        refresh_M(G, flag, n, k, part, sm.M);
        const int cap = iteration_cap(n, k);
        for (;;) {
            if (iters >= cap) {
                status = MRBF_DS_GAVE_UP;
                break;
            }
            ++iters;
            for (int e = t; e < k * k; e += THREADS) sm.L[e] = 0.0;
            lp::row_pass(n, k, [&](int i, int j) { return G[(size_t)j * k + i] * dv[j]; }, part, z);
            // ---- the k x k problem: the coefficients a of the step
            if (t == 0) {
                for (int i = 0; i < k; ++i) rho[i] = rv[i] - z[i];
                int n_s = 0;
                isc[I_BAD] = step_coeffs(sm, n_s) ? 0 : 1;
                isc[I_KIND] = n_s;
            }
            __syncthreads();
            if (isc[I_BAD]) {
                status = MRBF_DS_GAVE_UP;
                break;
            }
            for (int j = t; j < n; j += THREADS) {
                double acc = 0.0;
                if (flag[j] == 0)
                    for (int i = 0; i < k; ++i) acc += G[(size_t)j * k + i] * av[i];
                pv[j] = acc;
            }
            __syncthreads();
            lp::row_pass(n, k, [&](int i, int j) { return G[(size_t)j * k + i] * pv[j]; }, part, dz);
            // ---- has the step vanished?  then the multipliers; else the rows' part of the ratio test
            if (t == 0) {
                bool vanish = true;
                for (int i = 0; i < k; ++i) vanish = vanish && fabs(dz[i]) <= VANISH_TOL * rscale[i];
                if (full >= 2 || vanish) {
                    multipliers(sm, isc[I_KIND]);
                    double mscale = 0.0;
                    for (int i = 0; i < k; ++i) {
                        yv[i] = mu[i] - rho[i];
                        ysc[i] = fabs(rv[i]) + fabs(z[i]) + fabs(mu[i]);
                        mscale = fmax(mscale, fabs(rv[i]) + fabs(z[i]));
                    }
                    double best = 0.0;
                    int idx = -1;
                    for (int i = 0; i < k; ++i) {
                        const double v = sm.inS[i] ? -mu[i] / mscale : 0.0;
                        if (v > DUAL_TOL && v > best && !(degen && idx >= 0)) best = v, idx = i;  // degenerate: the least index
                    }
                    isc[I_MODE] = MODE_MULT, isc[I_KIND] = idx >= 0 ? 1 : 0, isc[I_IDX] = idx;
                    dsc[D_BEST] = best;
                } else {
                    double amin = INF;
                    for (int i = 0; i < k; ++i) {
                        ar[i] = (!sm.inS[i] && dz[i] > VANISH_TOL * rscale[i]) ? fmax(0.0, -z[i] / dz[i]) : INF;
                        amin = fmin(amin, ar[i]);
                    }
                    isc[I_MODE] = MODE_STEP;
                    dsc[D_ALPHA] = fmin(1.0, amin);
                }
            }
            __syncthreads();
            if (isc[I_MODE] == MODE_MULT) {
                // ---- s = G' y on the variables that sit on a bound: the most violating sign, lowest index on ties
                double bestv = 0.0;
                int bestj = 0x7fffffff;
                for (int j = t; j < n; j += THREADS) {
                    const int f = flag[j];
                    if (f != -1 && f != 1) continue;
                    double sj = 0.0, sc = 0.0;
                    for (int i = 0; i < k; ++i) {
                        const double g = G[(size_t)j * k + i];
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
                    if (t == 0) sm.inS[idx] = 0;
                    __syncthreads();
                } else {
                    if (t == 0) flag[idx] = 0;
                    __syncthreads();
                    refresh_M(G, flag, n, k, part, sm.M);
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
                for (int i = 0; i < k; ++i)
                    if (ar[i] <= alpha && !(degen && rows_hit)) sm.inS[i] = 1, rows_hit = 1;
                isc[I_NHIT] = (int)part[0], isc[I_IDX] = ipart[0], isc[I_ROWHIT] = rows_hit;
            }
            __syncthreads();
            const int nhit = isc[I_NHIT];
            full = (nhit == 0 && !isc[I_ROWHIT]) ? full + 1 : 0;
            if (nhit >= 1) refresh_M(G, flag, n, k, part, sm.M);
        }
    }
    // ---- outputs: z = G d from the returned d, in row_pass's order
    double *dout = a.d_out + qp * n, *zout = a.z_out + qp * k;
    if (status == MRBF_DS_OK) {
        lp::row_pass(n, k, [&](int i, int j) { return G[(size_t)j * k + i] * dv[j]; }, part, z);
        if (t == 0) {
            int bad = 0;
            double mx = -INF;
            for (int i = 0; i < k; ++i) {
                if (!(z[i] <= FEAS_TOL * rowsum[i])) bad = 1;  // a row above zero beyond its tolerance, or a NaN
                mx = fmax(mx, z[i]);
            }
            isc[I_BAD] = bad;
            dsc[D_ALPHA] = fmax(0.0, -mx);
        }
        __syncthreads();
        if (isc[I_BAD]) status = MRBF_DS_GAVE_UP;
    }
    if (status == MRBF_DS_OK) {
        for (int j = t; j < n; j += THREADS) dout[j] = dv[j];
        if (t < k) {
            zout[t] = z[t];
            if (a.mult_out) a.mult_out[qp * k + t] = mu[t];
        }
        if (t == 0) a.omega_out[qp] = dsc[D_ALPHA];
    } else {
        const double fill = status == MRBF_DS_GAVE_UP ? QNAN : 0.0;
        for (int j = t; j < n; j += THREADS) dout[j] = fill;
        if (t < k) {
            zout[t] = fill;
            if (a.mult_out) a.mult_out[qp * k + t] = fill;
        }
        if (t == 0) a.omega_out[qp] = status == MRBF_DS_GAVE_UP ? QNAN : (status == MRBF_DS_INFEASIBLE ? -INF : 0.0);
    }
    if (t == 0) {
        a.status_out[qp] = status;
        if (a.iters_out) a.iters_out[2 * qp] = iters, a.iters_out[2 * qp + 1] = dropped;
    }
}

// all device pointers; QPs in chunks so that the per-QP workspaces stay below dcall::WS_LIMIT_BYTES
int launch(mrbf_ctx *ctx, int64_t n_qp, int n, int k, const double *G, const double *r, const double *x, int64_t x_stride, const double *lb,
           const double *ub, int64_t bound_stride, double *d_out, double *z_out, double *omega_out, double *mult_out, int *status_out,
           int *iters_out) {
    Args a;
    a.n = n, a.k = k, a.xs = x_stride, a.bs = bound_stride;
    a.G = G, a.r = r, a.x = x, a.lb = lb, a.ub = ub;
    a.d_out = d_out, a.z_out = z_out, a.omega_out = omega_out, a.mult_out = mult_out, a.status_out = status_out, a.iters_out = iters_out;
    const int64_t per = dcall::chunk(n_qp, ws_bytes(n));
    MRBF_TRY(get_buf(ctx, S_DS_WS, (size_t)per * ws_doubles(n), &a.ws));
    MRBF_TRY(get_buf(ctx, S_DS_WSI, (size_t)per * ws_ints(n), &a.wsi));
    const size_t shm = carve(k).total;
    for (int64_t q0 = 0; q0 < n_qp; q0 += per) {
        const unsigned grid = (unsigned)std::min<int64_t>(per, n_qp - q0);
        hipLaunchKernelGGL(ds_qp_kernel, dim3(grid), dim3(THREADS), shm, ctx->stream, a, q0);
        MRBF_HIP(ctx, hipGetLastError());
    }
    return 0;
}

}  // namespace ds
}  // namespace mrbf

using namespace mrbf;

// descent.jl:583-664: the direction QP of directed search for n_qp starts in one launch
extern "C" int32_t mrbf_ds_direction(mrbf_ctx *ctx, int64_t n_qp, int32_t d, int32_t k, const double *G, const double *r, const double *x,
                                     const double *lb, const double *ub, double *d_out, double *z_out, double *omega_out, double *mult_out,
                                     int32_t *status_out, int32_t *iters_out) {
    ds::Call c;
    c.has_ctx = ctx != nullptr, c.n_qp = n_qp, c.d = d, c.k = k;
    c.G = G != nullptr, c.r = r != nullptr, c.x = x != nullptr, c.lb = lb != nullptr, c.ub = ub != nullptr;
    c.d_out = d_out != nullptr, c.z_out = z_out != nullptr, c.omega_out = omega_out != nullptr, c.status_out = status_out != nullptr;
    if (const int rc = ds::validate(c)) return rc == -1 ? -1 : fail(ctx, rc, "mrbf_ds_direction: invalid argument (n_qp = %lld, d = %d (1..%d), k = %d (1..%d), or a NULL array)", (long long)n_qp, d, ds::MAXD, k, ds::MAXK);
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    const size_t N = (size_t)n_qp;
    double *arena;
    MRBF_TRY(get_buf(ctx, S_DS_IN, N * ((size_t)k * d + k + 3 * (size_t)d), &arena));
    const double *dG, *dr, *dx, *dlb, *dub;
    MRBF_TRY(input_view(ctx, G, N * k * d, arena, &dG));
    MRBF_TRY(input_view(ctx, r, N * k, arena, &dr));
    MRBF_TRY(input_view(ctx, x, N * d, arena, &dx));
    MRBF_TRY(input_view(ctx, lb, N * d, arena, &dlb));
    MRBF_TRY(input_view(ctx, ub, N * d, arena, &dub));
    dcall::Outputs out;  // d, z, omega, mult, status, iterations
    MRBF_TRY(out.open(ctx, S_DS_OUT, {{d_out, N * d, false}, {z_out, N * k, false}, {omega_out, N, false}, {mult_out, N * k, false}, {status_out, N, true}, {iters_out, 2 * N, true}}));
    MRBF_TRY(ds::launch(ctx, n_qp, d, k, dG, dr, dx, d, dlb, dub, d, out.at<double>(0), out.at<double>(1), out.at<double>(2), out.at<double>(3), out.at<int>(4), out.at<int>(5)));
    MRBF_TRY(out.copy_back(ctx));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    return MRBF_OK;
}

// descent.jl:583-664: the criticality of directed search for a container -- objective Jacobians at x_n through the evaluation kernels,
// gathered by the roles table, one direction QP, one read-back
extern "C" int32_t mrbf_ds_criticality(mrbf_ctx *ctx, const mrbf_ps_problem *prob, const double *x_n, const double *lb, const double *ub,
                                       const double *r, double *d_out, double *mult_out, mrbf_ds_info *info) {
    if (!ctx) return -1;
    if (!prob) return fail(ctx, -3, "problem is NULL");
    if (!x_n) return fail(ctx, -4, "x_n is NULL");
    if (!lb) return fail(ctx, -5, "lb is NULL");
    if (!ub) return fail(ctx, -6, "ub is NULL");
    if (!r) return fail(ctx, -7, "r is NULL");
    if (!d_out) return fail(ctx, -8, "d_out is NULL");
    if (!info) return fail(ctx, -10, "info is NULL");
    std::memset(info, 0, sizeof(*info));
    if (prob->n_models < 1 || !prob->models || !prob->roles) return fail(ctx, -2, "mrbf_ds_criticality: grouped models with a roles table are required");
    std::vector<descent::SlotShape> slots;
    descent::Layout lay;
    if (descent::Defect D = descent::read(descent_shape(prob, prob->models, 1, slots), {true, descent::Centres::UNCHECKED}, lay))
        return fail(ctx, -2, "mrbf_ds_criticality: %s", D.msg.c_str());
    const int d = lay.d, k = prob->n_objectives, n_lin = prob->n_lin_eq + prob->n_lin_ineq;
    if (mrbf_dispatch_ds(d, k, prob->n_models, lay.n_nl, n_lin, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_ds_criticality: d = %d / k = %d / %d constraint rows outside the device path (ask mrbf_dispatch_ds first)", d, k, lay.n_nl + n_lin);
    const descent::Offsets at = lay.offsets(1, descent::Slots::OBJECTIVE);
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- host inputs, packed: x_n, lb, ub, r
    dcall::PackedIn in;
    const size_t axn = in.fetch(ctx, x_n, d), alb = in.fetch(ctx, lb, d), aub = in.fetch(ctx, ub, d), ar = in.fetch(ctx, r, k);
    MRBF_TRY(in.rc);
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, ctx->stream));
    // device arena: inputs | Jacobians | G | outputs (d, z, omega, mult, 3 int words)
    const size_t out_dbl = (size_t)d + 2 * (size_t)k + 1, out_cnt = out_dbl + 2;
    double *base;
    MRBF_TRY(get_buf(ctx, S_DS_IN, in.total + at.jtot + (size_t)k * d + out_cnt, &base));
    double *dJ = base + in.total, *dG = dJ + at.jtot, *dout = dG + (size_t)k * d;
    MRBF_TRY(in.upload(ctx, base));
    const double *dxn = in.dev(axn), *dlb = in.dev(alb), *dub = in.dev(aub), *dr = in.dev(ar);
    for (int j = 0; j < prob->n_models; ++j)
        if (lay.chosen(j, descent::Slots::OBJECTIVE)) MRBF_TRY(eval_model(ctx, prob->models[j], 1, dxn, nullptr, dJ + at.jac[j], nullptr));
    // ---- G from the Jacobians by the roles table (the objective rows of sd_lp.hip's assembly)
    sd::AsmArgs aa;
    std::memset(&aa, 0, sizeof(aa));
    aa.n = d, aa.k = k, aa.rows = k;
    aa.J = dJ, aa.xn = dxn, aa.x = dxn;
    aa.G = dG;
    descent::fill_sources(lay, at, true, aa.src);  // the linear rows are refused above: k objective rows
    MRBF_TRY(sd::launch_assemble(ctx, aa, 1));
    int *oi = reinterpret_cast<int *>(dout + out_dbl);
    MRBF_TRY(ds::launch(ctx, 1, d, k, dG, dr, dxn, 0, dlb, dub, 0, dout, dout + d, dout + d + k, dout + d + k + 1, oi, oi + 1));
    // ---- one read-back
    std::vector<double> hout(out_cnt);
    MRBF_HIP(ctx, hipMemcpyAsync(hout.data(), dout, out_cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MRBF_HIP(ctx, hipEventRecord(e1, ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    MRBF_HIP(ctx, hipEventElapsedTime(&info->ms_total, e0, e1));
    dcall::read_status(hout.data() + out_dbl, &info->status, &info->iterations, &info->dropped);
    info->omega = hout[d + k];
    MRBF_TRY(output_put(ctx, d_out, hout.data(), d));
    if (mult_out) MRBF_TRY(output_put(ctx, mult_out, hout.data() + d + k + 1, k));
    if (info->status == MRBF_DS_GAVE_UP) return fail(ctx, -2, "mrbf_ds_criticality: the direction QP gave up (take the host method)");
    return MRBF_OK;
}
