// The steepest-descent step on the device: compute_descent_step(::SteepestDescentConfig) (Morbit.jl src/descent.jl:243-318)
// for a whole SurrogateContainer, with the step size sigma of descent.jl:251-310 (_local_bounds, intersect_box, _intersect_bounds of
// utilities.jl:126-294) and the Armijo loop of _backtrack (descent.jl:150-185) over every step size at once.
//
// One call is a short chain on the ctx stream and one read-back:
//   eval_model at x (values + Jacobians) of every model that carries a modelled constraint row  -- the "intersect" branch's rows
//   sd_stepsize_kernel  (1 x 256)        lb_eff / ub_eff, isapprox(x, x_n), Delta, the branch, sigma; steps[i] = steps[i-1] * shrink
//   sd_trial_kernel     ((L + 2) x d)    row 0 = x_n, row 1 + i = x_n + steps[i] * d
//   eval_model at the L + 2 rows (values) of every model that carries an objective row
//   sd_armijo_kernel    (1 x 256)        the index the reference loop stops at, x+, m(x+) in objective order, ||step||_inf
// The host mirror (morbit.jl_amd/descent.py: _sd_stepsize, _intersect_bounds, _backtrack) is the specification.  Every sum runs in an
// order fixed by the shape (lane-strided partials, a fixed shuffle / LDS tree); every min / max is exact; no atomics.  The trial points
// and Armijo right-hand sides are formed without FMA contraction, so they round exactly as the host loop's `x + s * d` and
// `s * c * omega` do.  DESIGN.md section 10.
#include "descent_call.hpp"
#include "sd.hpp"

namespace mrbf {
namespace sdstep {

constexpr double SQRT_EPS = 1.4901161193847656e-08;  // sqrt(eps(Float64)) = 2^-26: Julia's isapprox rtol
constexpr double EPS = 2.220446049250313e-16;        // eps(Float64): _intersect_bounds' zero_tol

enum Branch { B_DELTA = 0, B_ONE = 1, B_INTERSECT = 2 };

__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }

// fixed-tree reductions over the 256 threads of the block (red: 256 doubles of LDS); every thread gets the result
template <class Op>
__device__ double block_reduce(double v, double *red, Op op) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
struct OpAdd {
    __device__ double operator()(double a, double b) const { return a + b; }
};
struct OpMin {
    __device__ double operator()(double a, double b) const { return nan_min(a, b); }
};
struct OpMax {
    __device__ double operator()(double a, double b) const { return nan_max(a, b); }
};
// wave-level fixed xor tree: every lane gets the sum
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// candidates of _intersect_bound_vec (utilities.jl:126-152) for one coordinate: the step to bound b from x along dd ("lb" / "ub" sense);
// returns +Inf when there is none (direction 0) so that it never becomes the minimum of the non-negative ones; `has` is set when the
// coordinate contributes an entry
__device__ __forceinline__ double bound_candidate(double xv, double bv, double dd, bool ub_sense, bool &has) {
    has = false;
    if (dd == 0.0) return INFINITY;
    has = true;
    const double tmp = bv - xv;
    if (tmp == 0.0) return ub_sense ? (dd < 0.0 ? INFINITY : 0.0) : (dd > 0.0 ? INFINITY : 0.0);
    return tmp / dd;
}
// smallest non-negative candidate so far (NaN is not >= 0: it never counts)
__device__ __forceinline__ void take_pos(double s, double &best, double &any_pos) {
    if (s >= 0.0) {
        best = s < best ? s : best;
        any_pos = 1.0;
    }
}

__global__ __launch_bounds__(THREADS) void sd_stepsize_kernel(StepArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[THREADS];
    __shared__ double rax[MAXROWS], rad[MAXROWS];
    __shared__ double s_sigma;
    __shared__ int s_mode;  // 0: finite equality sigma to check, 1: take the inequality-only candidates, 2: sigma decided
    const int tid = threadIdx.x, d = a.d;
    // ---- this start's arrays (lb / ub, the linear rows and the rows table are shared)
    const int64_t p = blockIdx.x;
    const double delta = a.delta[p];
    a.xn += p * a.sx, a.x += p * a.sx, a.dir += p * a.sdir, a.Jc += p * a.sJ, a.Vc += p * a.sV;
    a.steps += p * (a.max_loops + 1), a.out += p * 2;
    // ---- lb_eff, ub_eff (utilities.jl:290-294), isapprox(x, x_n), ||d||_inf, Delta = intersect_box(x_n, d, lb_eff, ub_eff; :pos)
    double neq = 0.0, nonfin = 0.0, sdiff = 0.0, sx = 0.0, sxn = 0.0, nd = 0.0, dnz = 0.0, best = INFINITY, anyp = 0.0;
    for (int t = tid; t < d; t += THREADS) {
        const double xv = a.x[t], xn = a.xn[t], dv = a.dir[t];
        const double lbe = nan_max(a.lb[t], xv - delta), ube = nan_min(a.ub[t], xv + delta);
        neq += (xv == xn) ? 0.0 : 1.0;
        nonfin += (isfinite(xv) && isfinite(xn)) ? 0.0 : 1.0;
        const double df = xv - xn;
        sdiff += df * df, sx += xv * xv, sxn += xn * xn;
        nd = nan_max(nd, fabs(dv));
        dnz += dv != 0.0 ? 1.0 : 0.0;
        bool h;
        take_pos(bound_candidate(xn, lbe, dv, false, h), best, anyp);
        take_pos(bound_candidate(xn, ube, dv, true, h), best, anyp);
    }
    neq = block_reduce(neq, red, OpAdd());
    nonfin = block_reduce(nonfin, red, OpAdd());
    sdiff = block_reduce(sdiff, red, OpAdd());
    sx = block_reduce(sx, red, OpAdd());
    sxn = block_reduce(sxn, red, OpAdd());
    nd = block_reduce(nd, red, OpMax());
    dnz = block_reduce(dnz, red, OpAdd());
    best = block_reduce(best, red, OpMin());
    anyp = block_reduce(anyp, red, OpMax());
    bool close;
    if (neq == 0.0) close = true;
    else if (nonfin != 0.0) close = false;
    else close = sqrt(sdiff) <= SQRT_EPS * fmax(sqrt(sx), sqrt(sxn));
    const double Delta = close ? delta : (dnz == 0.0 ? INFINITY : (anyp != 0.0 ? best : 0.0));
    double sigma = 0.0;
    int branch;
    if (Delta <= 1.0) {
        branch = B_DELTA;
        const double r = Delta / nd;
        sigma = (r != r) ? r : (1.0 < r ? 1.0 : r);
    } else {
        // isapprox(norm_d, 1)
        const bool one = nd == 1.0 || (isfinite(nd) && fabs(nd - 1.0) <= SQRT_EPS * fmax(fabs(nd), 1.0));
        branch = one ? B_INTERSECT : B_ONE;
        sigma = 1.0;
    }
    if (branch == B_INTERSECT) {
        // ---- _intersect_bounds([x_n; n], [d; d], [lb_eff; lb_eff - x], [ub_eff; ub_eff - x], blockdiag rows; :pos), n = x_n - x
        const int R = a.n_eq + a.n_in, lane = tid & 63, wave = tid >> 6;
        for (int r = wave; r < R; r += THREADS / 64) {
            const RowRef rr = a.rows[r];
            const double *A = rr.modelled ? a.Jc + rr.a_off : a.Alin + rr.a_off;
            double px = 0.0, pd = 0.0;
            for (int t = lane; t < d; t += 64) {
                const double av = A[(int64_t)t * rr.stride];
                const double xv = rr.modelled ? a.xn[t] - a.x[t] : a.xn[t];
                px += av * xv, pd += av * a.dir[t];
            }
            px = wave_sum(px), pd = wave_sum(pd);
            if (lane == 0) rax[r] = px, rad[r] = pd;
        }
        __syncthreads();
        if (tid == 0) {
            int mode = 1;
            double sg = 0.0;
            if (dnz == 0.0) {
                mode = 2, sg = INFINITY;
            } else if (a.n_eq > 0) {
                bool have = false, impossible = false;
                for (int r = 0; r < a.n_eq && !impossible; ++r) {
                    const RowRef rr = a.rows[r];
                    const double b = rr.modelled ? -a.Vc[rr.b_off] : a.blin[rr.b_off];
                    const double ad = rad[r];
                    double si;
                    if (ad != 0.0) {
                        si = -(rax[r] - b) / ad;
                    } else {
                        if (fabs(rax[r] - b) > EPS) impossible = true;
                        continue;
                    }
                    if (!have) {
                        sg = si, have = true;
                    } else if (!(si == sg || fabs(si - sg) <= SQRT_EPS * fmax(fabs(si), fabs(sg)))) {
                        impossible = true;
                    }
                }
                if (impossible) mode = 2, sg = 0.0;
                else if (!have || isinf(sg)) mode = 1;  // no row fixes sigma: the inequality-only problem (utilities.jl:262-264)
                else mode = 0;
            }
            s_mode = mode, s_sigma = sg;
        }
        __syncthreads();
        const int mode = s_mode;
        if (mode == 1) {
            // smallest non-negative candidate of the box rows of both halves and of the inequality rows (0 when there is none)
            double b2 = INFINITY, p2 = 0.0, h2 = 0.0;
            for (int t = tid; t < d; t += THREADS) {
                const double xv = a.x[t], xn = a.xn[t], dv = a.dir[t], nv = xn - xv;
                const double lbe = nan_max(a.lb[t], xv - delta), ube = nan_min(a.ub[t], xv + delta);
                bool h;
                take_pos(bound_candidate(xn, lbe, dv, false, h), b2, p2), h2 += h;
                take_pos(bound_candidate(nv, lbe - xv, dv, false, h), b2, p2), h2 += h;
                take_pos(bound_candidate(xn, ube, dv, true, h), b2, p2), h2 += h;
                take_pos(bound_candidate(nv, ube - xv, dv, true, h), b2, p2), h2 += h;
            }
            for (int r = a.n_eq + tid; r < R; r += THREADS) {
                const RowRef rr = a.rows[r];
                const double b = rr.modelled ? -a.Vc[rr.b_off] : a.blin[rr.b_off];
                bool h;
                take_pos(bound_candidate(rax[r], b, rad[r], true, h), b2, p2), h2 += h;
            }
            b2 = block_reduce(b2, red, OpMin());
            p2 = block_reduce(p2, red, OpMax());
            h2 = block_reduce(h2, red, OpAdd());
            sigma = h2 == 0.0 ? INFINITY : (p2 != 0.0 ? b2 : 0.0);
        } else if (mode == 0) {
            // x + sigma d against the box and the inequality rows (utilities.jl:266-281), then the sign test of :pos
            const double sg = s_sigma;
            double bad = 0.0;
            for (int t = tid; t < d; t += THREADS) {
                const double xv = a.x[t], xn = a.xn[t], dv = a.dir[t], nv = xn - xv;
                const double lbe = nan_max(a.lb[t], xv - delta), ube = nan_min(a.ub[t], xv + delta);
                const double sd = sg * dv;
                const double t1 = xn + sd, t2 = nv + sd;
                bad += (t1 < lbe || t1 > ube || t2 < lbe - xv || t2 > ube - xv) ? 1.0 : 0.0;
            }
            for (int r = a.n_eq + wave; r < R; r += THREADS / 64) {
                const RowRef rr = a.rows[r];
                const double *A = rr.modelled ? a.Jc + rr.a_off : a.Alin + rr.a_off;
                double p = 0.0;
                for (int t = lane; t < d; t += 64) {
                    const double xv = rr.modelled ? a.xn[t] - a.x[t] : a.xn[t];
                    const double sd = sg * a.dir[t];
                    p += A[(int64_t)t * rr.stride] * (xv + sd);
                }
                p = wave_sum(p);
                const double b = rr.modelled ? -a.Vc[rr.b_off] : a.blin[rr.b_off];
                if (lane == 0 && p - b > 0.0) bad += 1.0;
            }
            bad = block_reduce(bad, red, OpAdd());
            sigma = (bad != 0.0 || sg < 0.0) ? 0.0 : sg;
        } else {
            sigma = s_sigma;
        }
    }
    if (tid == 0) {
        // step sizes exactly as the sequential loop forms them: step_size *= alpha (descent.jl:175)
        double s = sigma;
        a.steps[0] = s;
        for (int i = 1; i <= a.max_loops; ++i) {
            s = s * a.shrink;
            a.steps[i] = s;
        }
        a.out[0] = sigma;
        a.out[1] = (double)branch;
    }
}

// per start: row 0 = x_n, row 1 + i = x_n + steps[i] * d (descent.jl:162, :177), i = 0 .. max_loops
__global__ __launch_bounds__(THREADS) void sd_trial_kernel(const double *__restrict__ xn, int64_t sx, const double *__restrict__ dir, int64_t sdir,
                                                           const double *__restrict__ steps, int d, int max_loops, int64_t total,
                                                           double *__restrict__ X) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= total) return;
    const int64_t per = (int64_t)(max_loops + 2) * d;
    const int64_t p = e / per, r = e - p * per;
    const int64_t row = r / d;
    const int t = (int)(r - row * d);
    xn += p * sx, dir += p * sdir, steps += p * (max_loops + 1);
    if (row == 0) {
        X[e] = xn[t];
    } else {
        const double sd = steps[row - 1] * dir[t];
        X[e] = xn[t] + sd;
    }
}

__global__ __launch_bounds__(THREADS) void sd_armijo_kernel(ArmijoArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[THREADS];
    __shared__ double mx[MAXK];
    const int tid = threadIdx.x, k = a.k;
    const int64_t p = blockIdx.x;
    const double omega = a.omega[p];
    a.V += p * a.sV, a.X += p * (int64_t)(a.max_loops + 2) * a.d, a.dir += p * a.sdir;
    a.steps += p * (a.max_loops + 1), a.stepout += p * 2;
    a.xplus += p * a.d, a.mxplus += p * k, a.tail += p * ARMIJO_TAIL;
    if (tid < k) mx[tid] = a.V[a.obj[tid].off];
    __syncthreads();
    const double sigma = a.stepout[0];
    const bool zero = !(sigma > a.min_stepsize_raw);  // descent.jl:312-317 (NaN included)
    double first = (double)a.max_loops;
    if (!zero) {
        double mxmax = mx[0];
        for (int l = 1; l < k; ++l) mxmax = nan_max(mxmax, mx[l]);
        for (int i = tid; i < a.max_loops; i += THREADS) {
            const double st = a.steps[i];
            const double sc = st * a.const_rhs;
            const double rhs = sc * omega;
            bool ok;
            if (a.strict) {
                ok = true;
                for (int l = 0; l < k; ++l) {
                    const double mp = a.V[a.obj[l].off + (int64_t)(i + 1) * a.obj[l].stride];
                    ok = ok && ((mx[l] - mp) >= rhs);
                }
            } else {
                double mpmax = a.V[a.obj[0].off + (int64_t)(i + 1) * a.obj[0].stride];
                for (int l = 1; l < k; ++l) mpmax = nan_max(mpmax, a.V[a.obj[l].off + (int64_t)(i + 1) * a.obj[l].stride]);
                ok = (mxmax - mpmax) >= rhs;
            }
            if (ok || st <= a.min_step) {
                first = (double)i;
                break;  // the smallest index of this thread's stride
            }
        }
    }
    first = block_reduce(first, red, OpMin());
    const int i = (int)first;
    const int64_t row = zero ? 0 : (int64_t)i + 1;
    const double st = zero ? 0.0 : a.steps[i];
    double nrm = 0.0;
    for (int t = tid; t < a.d; t += THREADS) {
        a.xplus[t] = a.X[row * a.d + t];
        nrm = nan_max(nrm, fabs(st * a.dir[t]));
    }
    nrm = block_reduce(nrm, red, OpMax());
    if (tid < k) a.mxplus[tid] = a.V[a.obj[tid].off + row * a.obj[tid].stride];
    if (tid == 0) {
        a.tail[0] = zero ? 0.0 : omega;
        a.tail[1] = zero ? 0.0 : nrm;
        a.tail[2] = zero ? 0.0 : (double)i;
        a.tail[3] = sigma;
        a.tail[4] = a.stepout[1];
    }
}

int launch_stepsize(mrbf_ctx *ctx, const StepArgs &a, int64_t n_starts) {
    hipLaunchKernelGGL(sd_stepsize_kernel, dim3((unsigned)n_starts), dim3(THREADS), 0, ctx->stream, a);
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}
int launch_trial(mrbf_ctx *ctx, const double *xn, int64_t sx, const double *dir, int64_t sdir, const double *steps, int d, int max_loops,
                 int64_t n_starts, double *X) {
    const int64_t tot = n_starts * (int64_t)(max_loops + 2) * d;
    hipLaunchKernelGGL(sd_trial_kernel, dim3((unsigned)((tot + THREADS - 1) / THREADS)), dim3(THREADS), 0, ctx->stream, xn, sx, dir, sdir, steps, d,
                       max_loops, tot, X);
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}
int launch_armijo(mrbf_ctx *ctx, const ArmijoArgs &a, int64_t n_starts) {
    hipLaunchKernelGGL(sd_armijo_kernel, dim3((unsigned)n_starts), dim3(THREADS), 0, ctx->stream, a);
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace sdstep
}  // namespace mrbf

using namespace mrbf;

extern "C" int32_t mrbf_sd_step(mrbf_ctx *ctx, const mrbf_ps_problem *prob, const double *x, const double *x_n, double delta,
                                const double *lb, const double *ub, double omega, const double *dir, const mrbf_sd_step_options *opts,
                                double *x_plus, double *mx_plus, mrbf_sd_step_info *info) {
    using namespace sdstep;
    if (!ctx) return -1;
    if (!prob) return fail(ctx, -2, "problem is NULL");
    if (!x) return fail(ctx, -3, "x is NULL");
    if (!x_n) return fail(ctx, -4, "x_n is NULL");
    if (!lb) return fail(ctx, -5, "lb is NULL");
    if (!ub) return fail(ctx, -6, "ub is NULL");
    if (!dir) return fail(ctx, -7, "d is NULL");
    if (!opts) return fail(ctx, -8, "opts is NULL");
    if (!x_plus) return fail(ctx, -9, "x_plus is NULL");
    if (!mx_plus) return fail(ctx, -10, "mx_plus is NULL");
    if (!info) return fail(ctx, -11, "info is NULL");
    std::memset(info, 0, sizeof(*info));
    if (!(opts->shrink > 0.0 && opts->shrink < 1.0)) return fail(ctx, -8, "mrbf_sd_step: shrink must lie in (0, 1)");
    if (prob->n_models < 1 || !prob->models || !prob->roles) return fail(ctx, -2, "mrbf_sd_step: grouped models with a roles table are required");
    // ---- objective sources and modelled constraint rows from the roles table
    std::vector<descent::SlotShape> slots;
    descent::Layout lay;
    if (descent::Defect D = descent::read(descent_shape(prob, prob->models, 1, slots), {true, descent::Centres::UNCHECKED}, lay))
        return fail(ctx, -2, "mrbf_sd_step: %s", D.msg.c_str());
    const int d = lay.d, k = prob->n_objectives, n_lin = prob->n_lin_eq + prob->n_lin_ineq;
    if (mrbf_dispatch_sd_step(d, k, prob->n_models, lay.n_nl, n_lin, 0, opts->max_loops) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_sd_step: d = %d / k = %d / %d rows / max_loops = %d outside the device path (ask mrbf_dispatch_sd_step first)",
                    d, k, lay.n_nl + n_lin, opts->max_loops);
    const int L = opts->max_loops;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- host inputs, packed: x_n, x, lb, ub, d, linear rows (eq, then ineq), their b, delta, omega
    dcall::PackedIn in;
    const size_t axn = in.fetch(ctx, x_n, d), ax = in.fetch(ctx, x, d), alb = in.fetch(ctx, lb, d), aub = in.fetch(ctx, ub, d), adir = in.fetch(ctx, dir, d);
    const auto [aA, ab] = in.fetch_linear_rows(ctx, prob, d);
    const size_t asc = in.room(2);
    MRBF_TRY(in.rc);
    in.h[asc] = delta, in.h[asc + 1] = omega;
    // the stacked rows over the modelled rows' evaluations at x; one block of (L + 2) x k_j objective values per model with an objective row
    const descent::Offsets con = lay.offsets(1, descent::Slots::CONSTRAINED), objv = lay.offsets(L + 2, descent::Slots::OBJECTIVE);
    const std::vector<RowRef> rows = stacked_rows(lay, con);
    const int n_eq = lay.meq, n_in = lay.min;
    const int64_t jtot = con.jtot, vtot = con.vtot, otot = objv.vtot;
    // ---- device arena: inputs | rows table | Jc | Vc | steps | trial rows | objective values | outputs
    const size_t rows_dbl = (rows.size() * sizeof(RowRef) + sizeof(double) - 1) / sizeof(double);
    const size_t out_cnt = (size_t)d + k + ARMIJO_TAIL;
    const size_t total = in.total + rows_dbl + jtot + vtot + (L + 1) + 2 + (size_t)(L + 2) * d + otot + out_cnt;
    double *base;
    MRBF_TRY(get_buf(ctx, S_SD_STEP, total, &base));
    double *dRows = base + in.total, *dJc = dRows + rows_dbl, *dVc = dJc + jtot, *dSteps = dVc + vtot, *dSig = dSteps + (L + 1);
    double *dX = dSig + 2, *dV = dX + (size_t)(L + 2) * d, *dOut = dV + otot;
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, ctx->stream));
    MRBF_TRY(in.upload(ctx, base));
    if (!rows.empty())
        MRBF_HIP(ctx, hipMemcpyAsync(dRows, rows.data(), rows.size() * sizeof(RowRef), hipMemcpyHostToDevice, ctx->stream));
    const double *dxn = in.dev(axn), *dx = in.dev(ax), *dlb = in.dev(alb), *dub = in.dev(aub), *ddir = in.dev(adir);
    const double *dA = in.dev(aA), *db = in.dev(ab), *ddelta = in.dev(asc), *domega = ddelta + 1;
    // ---- the modelled constraint rows at x (values + Jacobians; the "intersect" branch reads them)
    for (int j = 0; j < prob->n_models; ++j)
        if (lay.has_con[j]) MRBF_TRY(eval_model(ctx, prob->models[j], 1, dx, dVc + con.val[j], dJc + con.jac[j], nullptr));
    // ---- sigma and the step sizes
    StepArgs sa;
    sa.d = d, sa.n_eq = n_eq, sa.n_in = n_in, sa.max_loops = L;
    sa.shrink = opts->shrink;
    sa.sx = sa.sdir = sa.sJ = sa.sV = 0;  // one start
    sa.delta = ddelta;
    sa.xn = dxn, sa.x = dx, sa.lb = dlb, sa.ub = dub, sa.dir = ddir;
    sa.Alin = dA, sa.blin = db, sa.Jc = dJc, sa.Vc = dVc;
    sa.rows = reinterpret_cast<const RowRef *>(dRows);
    sa.steps = dSteps, sa.out = dSig;
    MRBF_TRY(launch_stepsize(ctx, sa, 1));
    // ---- the L + 2 trial rows and the objective models' values there
    MRBF_TRY(launch_trial(ctx, dxn, 0, ddir, 0, dSteps, d, L, 1, dX));
    for (int j = 0; j < prob->n_models; ++j)
        if (lay.has_obj[j]) MRBF_TRY(eval_model(ctx, prob->models[j], L + 2, dX, dV + objv.val[j], nullptr, nullptr));
    // ---- the Armijo scan
    ArmijoArgs aa;
    aa.d = d, aa.k = k, aa.max_loops = L, aa.strict = opts->strict != 0;
    aa.const_rhs = opts->const_rhs;
    aa.sV = aa.sdir = 0;
    aa.omega = domega;
    aa.min_stepsize_raw = opts->min_stepsize;
    aa.min_step = opts->min_stepsize >= 0.0 ? opts->min_stepsize : EPS;  // descent.jl:152
    aa.V = dV, aa.X = dX, aa.dir = ddir, aa.steps = dSteps, aa.stepout = dSig;
    aa.xplus = dOut, aa.mxplus = dOut + d, aa.tail = dOut + d + k;
    fill_objectives(lay, objv, aa.obj);
    MRBF_TRY(launch_armijo(ctx, aa, 1));
    // ---- one read-back: x+, mx+, omega, ||step||, loops, sigma, branch
    std::vector<double> hout(out_cnt);
    MRBF_HIP(ctx, hipMemcpyAsync(hout.data(), dOut, out_cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    const bool dev_x = is_device_ptr(x_plus), dev_m = is_device_ptr(mx_plus);
    if (dev_x) MRBF_HIP(ctx, hipMemcpyAsync(x_plus, dOut, (size_t)d * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (dev_m) MRBF_HIP(ctx, hipMemcpyAsync(mx_plus, dOut + d, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    MRBF_HIP(ctx, hipEventRecord(e1, ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    MRBF_HIP(ctx, hipEventElapsedTime(&info->ms_total, e0, e1));
    const double *o = hout.data();
    if (!dev_x) std::memcpy(x_plus, o, (size_t)d * sizeof(double));
    if (!dev_m) std::memcpy(mx_plus, o + d, (size_t)k * sizeof(double));
    info->sigma = o[d + k + 3];
    info->branch = (int32_t)o[d + k + 4];
    info->omega = o[d + k];
    info->step_norm = o[d + k + 1];
    info->loops = (int32_t)o[d + k + 2];
    return MRBF_OK;
}
