// Many-start directed search: the criticality of directed search (Morbit.jl src/descent.jl:583-664) followed by its step
// (descent.jl:645-660: the steepest-descent step on the normalised direction) for n_starts independent starts of one problem in one
// call -- the reference's Threads.@threads loop over Halton starts (examples/large_scale_benchmarks.jl:102-109), where every start
// carries its own surrogate container of one shared shape.  For start p the outputs are, bit for bit, those of mrbf_ds_criticality, the
// bindings' normalisation rule and mrbf_sd_step chained on start p's container: the kernels are the single calls' own, with the start
// on a grid dimension (ds.hpp, sd.hpp), and the one kernel between them divides as the host does.
//
// One call is one chain on the ctx stream and one read-back, with no host synchronisation in between:
//   one packed upload           [x_n; x] pairs, delta, lb, ub, r, the evaluation descriptors
//   eval_fused_batch            Jacobians only, at x_n, of the objective slots: the evaluation of mrbf_ds_criticality (one site, no
//                               values), one launch group per (kernel and parameters, k, dpad, split or unsplit centre range), so the
//                               centre-range split and the order of every sum are the single call's
//   sd_assemble_kernel          (k x n_starts)      G of every start in jac_out layout (objective rows only)
//   ds_qp_kernel                (n_starts)          the direction QPs: x at stride 2 d in the pairs, one box, r per start
//   ds_scale_kernel             (n_starts x 256)    ||d||_inf, d / ||d||_inf and omega, or zeros and 0: what the step is given
//   sd_stepsize_kernel          (n_starts x 256)    sigma, the branch, the step sizes
//   sd_trial_kernel             (n_starts x (L + 2) x d)
//   eval_fused_batch            values of the objective slots at the L + 2 trial rows of every start
//   sd_armijo_kernel            (n_starts x 256)    x+, m(x+) and the record words into one output block
//   one download of that block  (device to device for outputs given as device pointers)
// A member the fused evaluation does not take (MRBF_OPT_EVAL_IMPL = 1) is evaluated by eval_model on the same stream.  At a
// homogeneous batch the launch count does not depend on n_starts.  DESIGN.md section 22.
#include <limits>

#include "batch_chain.hpp"
#include "ds.hpp"
#include "ds_batch_host.hpp"
#include "sd.hpp"

using namespace mrbf;

static_assert(sizeof(mrbf_ds_batch_record) == 64, "mrbf_ds_batch_record is 64 bytes");
static_assert(dsbatch::TAIL == sdstep::ARMIJO_TAIL, "the record is packed from the Armijo kernel's tail");

namespace {
enum Site { SITE_XN = 0, SITE_TRIAL = 1 };

// max that keeps a NaN once it has one, as numpy.max does: exact, so the order of the tree does not show in the bits
__device__ inline double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// One workgroup per start, between the QP's outputs and the step's inputs: the bindings' rule of get_criticality_ds.  With status OK and
// ||d||_inf > 0 the step gets (omega, d / ||d||_inf) -- a plain IEEE division, as NumPy's d / nrm --, otherwise (0, zeros); dnorm is
// ||d||_inf of an OK start and 0 of any other.  The QP's own omega stays where the QP left it.
__global__ __launch_bounds__(dsbatch::SCALE_THREADS) void ds_scale_kernel(int d, const double *__restrict__ draw, const int *__restrict__ status,
                                                                         const double *__restrict__ omega, double *__restrict__ dir,
                                                                         double *__restrict__ omega_step, double *__restrict__ dnorm) {
    constexpr int T = dsbatch::SCALE_THREADS;
    __shared__ double part[T];
    const int t = threadIdx.x;
    const int64_t p = blockIdx.x;
    const double *src = draw + p * d;
    double *dst = dir + p * d;
    const bool ok = status[p] == MRBF_DS_OK;
    double m = 0.0;
    if (ok)
        for (int j = t; j < d; j += T) m = nan_max(m, fabs(src[j]));
    part[t] = m;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s) part[t] = nan_max(part[t], part[t + s]);
        __syncthreads();
    }
    const double nrm = part[0];
    const bool go = ok && nrm > 0.0;
    for (int j = t; j < d; j += T) dst[j] = go ? src[j] / nrm : 0.0;
    if (t == 0) {
        omega_step[p] = go ? omega[p] : 0.0;
        dnorm[p] = nrm;
    }
}

int launch_scale(mrbf_ctx *ctx, int64_t n_starts, int d, const double *draw, const int *status, const double *omega, double *dir,
                 double *omega_step, double *dnorm) {
    hipLaunchKernelGGL(ds_scale_kernel, dim3((unsigned)n_starts), dim3(dsbatch::SCALE_THREADS), 0, ctx->stream, d, draw, status, omega, dir,
                       omega_step, dnorm);
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int32_t mrbf_ds_iterate_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                                         const double *x, const double *x_n, const double *delta, const double *lb, const double *ub,
                                         const double *r, const mrbf_sd_step_options *opts, double *d_out, double *x_plus, double *mx_plus,
                                         double *mult_out, mrbf_ds_batch_record *records, float *ms_total) {
    dsbatch::Call c;
    c.has_ctx = ctx != nullptr, c.n_starts = n_starts;
    c.shape = shape != nullptr, c.models = models != nullptr, c.x = x != nullptr, c.x_n = x_n != nullptr, c.delta = delta != nullptr;
    c.lb = lb != nullptr, c.ub = ub != nullptr, c.r = r != nullptr, c.opts = opts != nullptr;
    c.d_out = d_out != nullptr, c.x_plus = x_plus != nullptr, c.mx_plus = mx_plus != nullptr, c.records = records != nullptr;
    if (opts) c.shrink = opts->shrink;
    if (shape) c.n_models = shape->n_models, c.roles = shape->roles != nullptr;
    if (const int rc = dsbatch::validate(c))
        return rc == -1 ? -1
                        : fail(ctx, rc, rc == -2 ? "mrbf_ds_iterate_batch: %lld starts (ask mrbf_dispatch_ds_batch first)"
                                                 : "mrbf_ds_iterate_batch: invalid argument (n_starts = %lld; a NULL array, shrink outside (0, 1), or a shape without grouped models and a roles table)",
                               (long long)n_starts);
    const int k = shape->n_objectives, nm = shape->n_models;
    const int64_t N = n_starts;
    // ---- the objective rows from the roles table (as mrbf_ds_criticality and mrbf_sd_step read it); the starts' slots agree
    std::vector<descent::SlotShape> slots;
    descent::Shape sh = descent_shape(shape, models, N, slots);
    sh.batch = true;
    descent::Layout lay;
    if (descent::Defect D = descent::read(sh, {true, descent::Centres::EVERY_SLOT}, lay))
        return fail(ctx, D.cls == descent::Defect::MODELS ? -4 : -3, "mrbf_ds_iterate_batch: %s", D.msg.c_str());
    const int d = lay.d, L = opts->max_loops, n_lin = shape->n_lin_eq + shape->n_lin_ineq;
    if (mrbf_dispatch_ds_batch(N, d, k, nm, lay.n_nl, n_lin, 0, L) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_ds_iterate_batch: %lld starts / d = %d / k = %d / %d constraint rows / max_loops = %d outside the device path (ask mrbf_dispatch_ds_batch first)",
                    (long long)N, d, k, lay.n_nl + n_lin, L);
    // the evaluations: Jacobians at x_n of the objective slots, values at the L + 2 trial rows of the objective slots
    const descent::Offsets atJ = lay.offsets(1, descent::Slots::OBJECTIVE), atO = lay.offsets(L + 2, descent::Slots::OBJECTIVE);
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- the evaluations of the two single calls, grouped by what one eval_fused_batch launch requires (batch_chain.hpp)
    chain::Plan ev;
    for (int site = 0; site < 2; ++site)
        for (int64_t p = 0; p < N; ++p)
            for (int j = 0; j < nm; ++j)
                if (lay.chosen(j, descent::Slots::OBJECTIVE)) ev.add(ctx, site, p, j, models[p * nm + j], site == SITE_XN ? 1 : L + 2, site == SITE_XN);
    ev.close();
    chain::Arena scratch;
    ev.carve(scratch);
    // ---- the arena (ds_batch_host.hpp): upload | work | evaluation scratch | output block
    dsbatch::Sizes sz;
    sz.n_starts = N, sz.d = d, sz.k = k, sz.max_loops = L;
    sz.jtot = (size_t)atJ.jtot, sz.otot = (size_t)atO.vtot, sz.desc_dbl = ev.desc_doubles(), sz.scratch = scratch.total;
    const dsbatch::Layout A = dsbatch::layout(sz);
    const size_t SN = (size_t)N;
    double *base;
    MRBF_TRY(get_buf(ctx, S_DS_BATCH, A.total, &base));
    double *dPairs = base + A.pairs, *dX = base + A.X;
    for (chain::Member &mb : ev.mem) {
        const size_t p = (size_t)mb.p;
        if (mb.group >= 0) mb.Xq += A.scratch, mb.xsq += A.scratch, mb.vpart += A.scratch, mb.gpart += A.scratch;
        if (mb.site == SITE_XN) {  // Jacobians only: no values buffer, as the single call passes none
            mb.ext = true;
            mb.X_at = dPairs + p * 2 * d, mb.vals_at = nullptr, mb.jac_at = base + A.J + p * sz.jtot + atJ.jac[mb.j];
        } else {
            mb.X = A.X + p * (size_t)(L + 2) * d, mb.vals = A.VO + p * sz.otot + atO.val[mb.j];
        }
    }
    // ---- the upload, staged in the pinned block where it fits
    chain::Staging up(ctx, A.up_cnt);
    double *hup = up.p;
    std::memset(hup, 0, A.up_cnt * sizeof(double));
    {
        std::vector<double> tmp(SN * d);
        MRBF_TRY(input_fetch(ctx, x_n, SN * d, tmp.data()));
        for (size_t p = 0; p < SN; ++p) std::memcpy(hup + A.pairs + p * 2 * d, tmp.data() + p * d, (size_t)d * sizeof(double));
        MRBF_TRY(input_fetch(ctx, x, SN * d, tmp.data()));
        for (size_t p = 0; p < SN; ++p) std::memcpy(hup + A.pairs + p * 2 * d + d, tmp.data() + p * d, (size_t)d * sizeof(double));
    }
    MRBF_TRY(input_fetch(ctx, delta, SN, hup + A.delta));
    MRBF_TRY(input_fetch(ctx, lb, d, hup + A.lb));
    MRBF_TRY(input_fetch(ctx, ub, d, hup + A.ub));
    MRBF_TRY(input_fetch(ctx, r, SN * k, hup + A.r));
    EvalDesc *hdesc = reinterpret_cast<EvalDesc *>(hup + A.desc);
    const EvalDesc *ddesc = reinterpret_cast<const EvalDesc *>(base + A.desc);
    ev.fill(base, hdesc);
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, st));
    MRBF_HIP(ctx, hipMemcpyAsync(base, hup, A.up_cnt * sizeof(double), hipMemcpyHostToDevice, st));
    MRBF_TRY(ev.launch(ctx, SITE_XN, base, hdesc, ddesc));
    // ---- G of every start from the Jacobians by the roles table (the objective rows of sd_lp.hip's assembly)
    sd::AsmArgs aa;
    std::memset(&aa, 0, sizeof(aa));
    aa.n = d, aa.k = k, aa.rows = k;
    aa.sJ = (int64_t)sz.jtot, aa.sx = 2 * (int64_t)d;
    aa.J = base + A.J, aa.xn = dPairs, aa.x = dPairs;
    aa.G = base + A.G;
    descent::fill_sources(lay, atJ, true, aa.src);  // the table refuses constraint rows: k objective rows
    MRBF_TRY(sd::launch_assemble(ctx, aa, N));
    // ---- the direction QPs, then what the step is given of them
    double *dRaw = base + A.draw, *dDir = base + A.dir, *dOmega = base + A.omega, *dOmegaStep = base + A.omega_step;
    int *dInts = reinterpret_cast<int *>(base + A.ints);
    MRBF_TRY(ds::launch(ctx, N, d, k, base + A.G, base + A.r, dPairs, 2 * (int64_t)d, base + A.lb, base + A.ub, 0, dRaw, base + A.z, dOmega,
                        base + A.mult, dInts, dInts + N));
    MRBF_TRY(launch_scale(ctx, N, d, dRaw, dInts, dOmega, dDir, dOmegaStep, base + A.dnorm));
    // ---- sigma and the step sizes, the trial rows, the objective models' values there, the Armijo scan
    sdstep::StepArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.d = d, sa.n_eq = 0, sa.n_in = 0, sa.max_loops = L;
    sa.shrink = opts->shrink;
    sa.sx = 2 * (int64_t)d, sa.sdir = d;
    sa.delta = base + A.delta;
    sa.xn = dPairs, sa.x = dPairs + d, sa.lb = base + A.lb, sa.ub = base + A.ub, sa.dir = dDir;
    sa.steps = base + A.steps, sa.out = base + A.sig;
    MRBF_TRY(sdstep::launch_stepsize(ctx, sa, N));
    MRBF_TRY(sdstep::launch_trial(ctx, dPairs, 2 * (int64_t)d, dDir, d, base + A.steps, d, L, N, dX));
    MRBF_TRY(ev.launch(ctx, SITE_TRIAL, base, hdesc, ddesc));
    sdstep::ArmijoArgs am;
    am.d = d, am.k = k, am.max_loops = L, am.strict = opts->strict != 0;
    am.const_rhs = opts->const_rhs;
    am.min_stepsize_raw = opts->min_stepsize;
    am.min_step = opts->min_stepsize >= 0.0 ? opts->min_stepsize : std::numeric_limits<double>::epsilon();  // descent.jl:152
    am.sV = (int64_t)sz.otot, am.sdir = d;
    am.omega = dOmegaStep;
    am.V = base + A.VO, am.X = dX, am.dir = dDir, am.steps = base + A.steps, am.stepout = base + A.sig;
    am.xplus = base + A.xp, am.mxplus = base + A.mxp, am.tail = base + A.tail;
    sdstep::fill_objectives(lay, atO, am.obj);
    MRBF_TRY(sdstep::launch_armijo(ctx, am, N));
    // ---- one read-back
    chain::Staging down(ctx, A.out_cnt);
    double *hout = down.p;
    MRBF_HIP(ctx, hipMemcpyAsync(hout, base + A.out0, A.out_cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    const struct Out {
        double *user;
        size_t at, cnt;  // place in the arena, doubles per start
        bool dev;
    } outs[4] = {{d_out, A.dir, (size_t)d, is_device_ptr(d_out)},
                 {x_plus, A.xp, (size_t)d, is_device_ptr(x_plus)},
                 {mx_plus, A.mxp, (size_t)k, is_device_ptr(mx_plus)},
                 {mult_out, A.mult, (size_t)k, mult_out != nullptr && is_device_ptr(mult_out)}};
    for (const Out &o : outs)
        if (o.user && o.dev) MRBF_HIP(ctx, hipMemcpyAsync(o.user, base + o.at, SN * o.cnt * sizeof(double), hipMemcpyDeviceToDevice, st));
    MRBF_HIP(ctx, hipEventRecord(e1, st));
    MRBF_HIP(ctx, hipStreamSynchronize(st));
    pin.flush();
    if (ms_total) MRBF_HIP(ctx, hipEventElapsedTime(ms_total, e0, e1));
    for (const Out &o : outs)
        if (o.user && !o.dev) std::memcpy(o.user, hout + (o.at - A.out0), SN * o.cnt * sizeof(double));
    const int32_t *hInts = reinterpret_cast<const int32_t *>(hout + (A.ints - A.out0));
    std::vector<double> nanrow;
    for (size_t p = 0; p < SN; ++p) {
        dsbatch::pack(records[p], p, SN, hInts, hout + (A.tail - A.out0), hout + (A.omega - A.out0), hout + (A.dnorm - A.out0));
        if (records[p].ds_status != MRBF_DS_GAVE_UP) continue;
        // the single call refuses this start (take the host method): its outputs say so
        if (nanrow.empty()) nanrow.assign((size_t)std::max(d, k), std::numeric_limits<double>::quiet_NaN());
        for (const Out &o : outs) {
            if (!o.user) continue;
            if (o.dev) MRBF_HIP(ctx, hipMemcpy(o.user + p * o.cnt, nanrow.data(), o.cnt * sizeof(double), hipMemcpyHostToDevice));
            else std::memcpy(o.user + p * o.cnt, nanrow.data(), o.cnt * sizeof(double));
        }
    }
    return MRBF_OK;
}
