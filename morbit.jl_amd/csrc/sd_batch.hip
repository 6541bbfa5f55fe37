// Many-start steepest descent: get_criticality(::SteepestDescentConfig, ...) (Morbit.jl src/descent.jl:187-241) followed by
// compute_descent_step (descent.jl:243-318) for n_starts independent starts of one problem in one call -- the reference's
// Threads.@threads loop over Halton starts (examples/large_scale_benchmarks.jl:102-109), where every start carries its own surrogate
// container of one shared shape.  For start p the outputs are, bit for bit, those of mrbf_sd_criticality and mrbf_sd_step chained on
// start p's container: the kernels are the single calls' own, with the start on a grid dimension (sd.hpp).
//
// One call is one chain on the ctx stream and one read-back, with no host synchronisation in between:
//   one packed upload           [x_n; x] pairs, delta, lb, ub, the linear rows, the rows table, the evaluation descriptors
//   eval_fused_batch            values + Jacobians at [x_n; x] of every used model and at x of the models with constraint rows, one
//                               launch group per (site, kernel and parameters, k, dpad, split or unsplit centre range): the evaluations
//                               and query counts of the single calls, so the centre-range split and the order of every sum are theirs
//   sd_assemble_kernel          (rows x n_starts)   G, A_eq / b_eq, A_ineq / b_ineq of every start in consecutive per-LP blocks
//   sd_lp_kernel                (n_starts)          the direction LPs
//   sd_stepsize_kernel          (n_starts x 256)    sigma, the branch, the step sizes; omega and d are read where the LP left them
//   sd_trial_kernel             (n_starts x (L + 2) x d)
//   eval_fused_batch            values of the objective models at the L + 2 trial rows of every start
//   sd_armijo_kernel            (n_starts x 256)    x+, m(x+) and the record words into one output block
//   one download of that block  (device to device for outputs given as device pointers)
// The starts share d, the model count, every model slot's output count, the roles table and the linear rows; the number of centres
// and the kernel parameters may differ from start to start (such members fall into different launch groups).  A member the fused
// evaluation does not take (MRBF_OPT_EVAL_IMPL = 1) is evaluated by eval_model on the same stream.  At a homogeneous batch the launch
// count does not depend on n_starts.  DESIGN.md section 11.
#include <limits>

#include "batch_chain.hpp"
#include "sd.hpp"

using namespace mrbf;

namespace {
enum Site { SITE_PAIR = 0, SITE_X = 1, SITE_TRIAL = 2 };
}  // namespace

extern "C" int32_t mrbf_sd_iterate_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                                         const double *x, const double *x_n, const double *delta, const double *lb, const double *ub,
                                         int32_t normalize, const mrbf_sd_step_options *opts, double *d_out, double *x_plus, double *mx_plus,
                                         mrbf_sd_batch_record *records, float *ms_total) {
    using sdstep::RowRef;
    if (!ctx) return -1;
    if (ms_total) *ms_total = 0.f;
    if (!shape) return fail(ctx, -3, "shape is NULL");
    if (!models) return fail(ctx, -4, "models is NULL");
    if (!x) return fail(ctx, -5, "x is NULL");
    if (!x_n) return fail(ctx, -6, "x_n is NULL");
    if (!delta) return fail(ctx, -7, "delta is NULL");
    if (!lb) return fail(ctx, -8, "lb is NULL");
    if (!ub) return fail(ctx, -9, "ub is NULL");
    if (!opts) return fail(ctx, -11, "opts is NULL");
    if (!d_out) return fail(ctx, -12, "d_out is NULL");
    if (!x_plus) return fail(ctx, -13, "x_plus is NULL");
    if (!mx_plus) return fail(ctx, -14, "mx_plus is NULL");
    if (!records) return fail(ctx, -15, "records is NULL");
    if (!(opts->shrink > 0.0 && opts->shrink < 1.0)) return fail(ctx, -11, "mrbf_sd_iterate_batch: shrink must lie in (0, 1)");
    if (shape->n_models < 1 || !shape->roles) return fail(ctx, -3, "mrbf_sd_iterate_batch: grouped models with a roles table are required");
    const int k = shape->n_objectives, nm = shape->n_models;
    if (n_starts < 1) return fail(ctx, -2, "mrbf_sd_iterate_batch: %lld starts (ask mrbf_dispatch_sd_batch first)", (long long)n_starts);
    const int64_t N = n_starts;
    // ---- rows of the LP and of the step from the roles table (as mrbf_sd_criticality and mrbf_sd_step read it); the starts' slots agree
    std::vector<descent::SlotShape> slots;
    descent::Shape sh = descent_shape(shape, models, N, slots);
    sh.batch = true;
    descent::Layout lay;
    if (descent::Defect D = descent::read(sh, {true, descent::Centres::EVERY_SLOT}, lay))
        return fail(ctx, D.cls == descent::Defect::MODELS ? -4 : -3, "mrbf_sd_iterate_batch: %s", D.msg.c_str());
    const int d = lay.d, L = opts->max_loops, n_lin = shape->n_lin_eq + shape->n_lin_ineq;
    if (mrbf_dispatch_sd_batch(N, d, k, nm, lay.n_nl, n_lin, 0, L) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_sd_iterate_batch: %lld starts / d = %d / k = %d / %d rows / max_loops = %d outside the device path (ask mrbf_dispatch_sd_batch first)",
                    (long long)N, d, k, lay.n_nl + n_lin, L);
    // the evaluations: [x_n; x] of every used slot (A), x of the slots with constraint rows (B), the L + 2 trial rows of the objective slots
    const descent::Offsets atA = lay.offsets(2, descent::Slots::USED), atB = lay.offsets(1, descent::Slots::CONSTRAINED);
    const descent::Offsets atO = lay.offsets(L + 2, descent::Slots::OBJECTIVE);
    const int64_t jtotA = atA.jtot, vtotA = atA.vtot, jtotB = atB.jtot, vtotB = atB.vtot, otot = atO.vtot;
    const int meq = lay.meq, min = lay.min, m = k + meq + min;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- the evaluations of the two single calls, grouped by what one eval_fused_batch launch requires (batch_chain.hpp)
    chain::Plan ev;
    const descent::Slots site_slots[3] = {descent::Slots::USED, descent::Slots::CONSTRAINED, descent::Slots::OBJECTIVE};
    auto site_m = [&](int site) -> int64_t { return site == SITE_PAIR ? 2 : (site == SITE_X ? 1 : L + 2); };
    for (int site = 0; site < 3; ++site)
        for (int64_t p = 0; p < N; ++p)
            for (int j = 0; j < nm; ++j) {
                if (!lay.chosen(j, site_slots[site])) continue;
                ev.add(ctx, site, p, j, models[p * nm + j], site_m(site), site != SITE_TRIAL);
            }
    ev.close();
    // ---- the arena (doubles; every piece a multiple of 16): upload | work | evaluation scratch | output block
    chain::Arena ar;
    const size_t nlin = (size_t)n_lin, SN = (size_t)N;
    const std::vector<RowRef> rows = sdstep::stacked_rows(lay, atB);
    const size_t rows_dbl = (rows.size() * sizeof(RowRef) + sizeof(double) - 1) / sizeof(double);
    const size_t desc_dbl = ev.desc_doubles();
    const size_t oPairs = ar.take(SN * 2 * d), oDelta = ar.take(SN), oLb = ar.take(d), oUb = ar.take(d), oA = ar.take(nlin * d), oB = ar.take(nlin);
    const size_t oRows = ar.take(rows_dbl), oDesc = ar.take(desc_dbl);
    const size_t up_cnt = ar.total;
    const size_t oJA = ar.take(SN * jtotA), oVA = ar.take(SN * vtotA), oJB = ar.take(SN * jtotB), oVB = ar.take(SN * vtotB);
    const size_t oG = ar.take(SN * k * d), oAeq = ar.take(SN * meq * d), oBeq = ar.take(SN * meq), oAin = ar.take(SN * min * d), oBin = ar.take(SN * min);
    const size_t oSteps = ar.take(SN * (L + 1)), oSig = ar.take(SN * 2), oX = ar.take(SN * (L + 2) * d), oVO = ar.take(SN * otot);
    ev.carve(ar);
    for (chain::Member &mb : ev.mem) {
        const size_t p = (size_t)mb.p;
        const int j = mb.j;
        if (mb.site == SITE_PAIR) mb.X = oPairs + p * 2 * d, mb.vals = oVA + p * vtotA + atA.val[j], mb.jacs = oJA + p * jtotA + atA.jac[j];
        else if (mb.site == SITE_X) mb.X = oPairs + p * 2 * d + d, mb.vals = oVB + p * vtotB + atB.val[j], mb.jacs = oJB + p * jtotB + atB.jac[j];
        else mb.X = oX + p * (size_t)(L + 2) * d, mb.vals = oVO + p * otot + atO.val[j];
    }
    // the output block: x+ | m(x+) | [omega_step, step_norm, loops, sigma, branch] | d | omega | status, (iterations, flips) words
    const size_t out0 = ar.total;
    const size_t oXp = ar.take(SN * d), oMxp = ar.take(SN * k), oTail = ar.take(SN * sdstep::ARMIJO_TAIL), oDir = ar.take(SN * d), oOmega = ar.take(SN);
    const size_t oInts = ar.take((3 * SN + 1) / 2);
    const size_t out_cnt = ar.total - out0;
    double *base;
    MRBF_TRY(get_buf(ctx, S_SD_BATCH, ar.total, &base));
    // ---- the upload, staged in the pinned block where it fits
    chain::Staging up(ctx, up_cnt);
    double *hup = up.p;
    std::memset(hup, 0, up_cnt * sizeof(double));
    {
        std::vector<double> tmp(SN * d);
        MRBF_TRY(input_fetch(ctx, x_n, SN * d, tmp.data()));
        for (size_t p = 0; p < SN; ++p) std::memcpy(hup + oPairs + p * 2 * d, tmp.data() + p * d, (size_t)d * sizeof(double));
        MRBF_TRY(input_fetch(ctx, x, SN * d, tmp.data()));
        for (size_t p = 0; p < SN; ++p) std::memcpy(hup + oPairs + p * 2 * d + d, tmp.data() + p * d, (size_t)d * sizeof(double));
    }
    MRBF_TRY(input_fetch(ctx, delta, SN, hup + oDelta));
    MRBF_TRY(input_fetch(ctx, lb, d, hup + oLb));
    MRBF_TRY(input_fetch(ctx, ub, d, hup + oUb));
    MRBF_TRY(fetch_linear_rows(ctx, shape, d, hup + oA, hup + oB));
    if (!rows.empty()) std::memcpy(hup + oRows, rows.data(), rows.size() * sizeof(RowRef));
    double *dPairs = base + oPairs, *dX = base + oX;
    EvalDesc *hdesc = reinterpret_cast<EvalDesc *>(hup + oDesc);
    const EvalDesc *ddesc = reinterpret_cast<const EvalDesc *>(base + oDesc);
    ev.fill(base, hdesc);
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, st));
    MRBF_HIP(ctx, hipMemcpyAsync(base, hup, up_cnt * sizeof(double), hipMemcpyHostToDevice, st));
    auto evaluate = [&](int site) -> int { return ev.launch(ctx, site, base, hdesc, ddesc); };
    MRBF_TRY(evaluate(SITE_PAIR));
    MRBF_TRY(evaluate(SITE_X));
    // ---- G, A_eq / b_eq (linear, then modelled), A_ineq / b_ineq (likewise) of every start
    sd::AsmArgs aa;
    aa.n = d, aa.k = k, aa.rows = m, aa.meq = meq, aa.min = min;
    aa.sJ = jtotA, aa.sV = vtotA, aa.sx = 2 * (int64_t)d;
    aa.J = base + oJA, aa.V = base + oVA, aa.xn = dPairs, aa.x = dPairs + d, aa.Alin = base + oA, aa.blin = base + oB;
    aa.G = base + oG, aa.Aeq = base + oAeq, aa.beq = base + oBeq, aa.Ain = base + oAin, aa.bin = base + oBin;
    descent::fill_sources(lay, atA, true, aa.src);
    MRBF_TRY(sd::launch_assemble(ctx, aa, N));
    double *dDir = base + oDir, *dOmega = base + oOmega;
    int *dInts = reinterpret_cast<int *>(base + oInts);
    MRBF_TRY(sd::launch(ctx, N, d, k, meq, min, normalize, base + oG, dPairs, 2 * (int64_t)d, base + oLb, base + oUb, 0,
                        meq ? base + oAeq : nullptr, meq ? base + oBeq : nullptr, min ? base + oAin : nullptr, min ? base + oBin : nullptr, dDir,
                        dOmega, nullptr, dInts, dInts + N));
    // ---- sigma and the step sizes, the trial rows, the objective models' values there, the Armijo scan
    sdstep::StepArgs sa;
    sa.d = d, sa.n_eq = meq, sa.n_in = min, sa.max_loops = L;
    sa.shrink = opts->shrink;
    sa.sx = 2 * (int64_t)d, sa.sdir = d, sa.sJ = jtotB, sa.sV = vtotB;
    sa.delta = base + oDelta;
    sa.xn = dPairs, sa.x = dPairs + d, sa.lb = base + oLb, sa.ub = base + oUb, sa.dir = dDir;
    sa.Alin = base + oA, sa.blin = base + oB, sa.Jc = base + oJB, sa.Vc = base + oVB;
    sa.rows = reinterpret_cast<const RowRef *>(base + oRows);
    sa.steps = base + oSteps, sa.out = base + oSig;
    MRBF_TRY(sdstep::launch_stepsize(ctx, sa, N));
    MRBF_TRY(sdstep::launch_trial(ctx, dPairs, 2 * (int64_t)d, dDir, d, base + oSteps, d, L, N, dX));
    MRBF_TRY(evaluate(SITE_TRIAL));
    sdstep::ArmijoArgs am;
    am.d = d, am.k = k, am.max_loops = L, am.strict = opts->strict != 0;
    am.const_rhs = opts->const_rhs;
    am.min_stepsize_raw = opts->min_stepsize;
    am.min_step = opts->min_stepsize >= 0.0 ? opts->min_stepsize : std::numeric_limits<double>::epsilon();  // descent.jl:152
    am.sV = otot, am.sdir = d;
    am.omega = dOmega;
    am.V = base + oVO, am.X = dX, am.dir = dDir, am.steps = base + oSteps, am.stepout = base + oSig;
    am.xplus = base + oXp, am.mxplus = base + oMxp, am.tail = base + oTail;
    sdstep::fill_objectives(lay, atO, am.obj);
    MRBF_TRY(sdstep::launch_armijo(ctx, am, N));
    // ---- one read-back
    chain::Staging down(ctx, out_cnt);
    double *hout = down.p;
    MRBF_HIP(ctx, hipMemcpyAsync(hout, base + out0, out_cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    const bool dev_d = is_device_ptr(d_out), dev_x = is_device_ptr(x_plus), dev_m = is_device_ptr(mx_plus);
    if (dev_d) MRBF_HIP(ctx, hipMemcpyAsync(d_out, dDir, SN * d * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (dev_x) MRBF_HIP(ctx, hipMemcpyAsync(x_plus, base + oXp, SN * d * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (dev_m) MRBF_HIP(ctx, hipMemcpyAsync(mx_plus, base + oMxp, SN * k * sizeof(double), hipMemcpyDeviceToDevice, st));
    MRBF_HIP(ctx, hipEventRecord(e1, st));
    MRBF_HIP(ctx, hipStreamSynchronize(st));
    pin.flush();
    if (ms_total) MRBF_HIP(ctx, hipEventElapsedTime(ms_total, e0, e1));
    const double *hXp = hout + (oXp - out0), *hMxp = hout + (oMxp - out0), *hTail = hout + (oTail - out0), *hDir = hout + (oDir - out0);
    const double *hOmega = hout + (oOmega - out0);
    const int *hInts = reinterpret_cast<const int *>(hout + (oInts - out0));
    if (!dev_d) std::memcpy(d_out, hDir, SN * d * sizeof(double));
    if (!dev_x) std::memcpy(x_plus, hXp, SN * d * sizeof(double));
    if (!dev_m) std::memcpy(mx_plus, hMxp, SN * k * sizeof(double));
    std::vector<double> nanrow;
    for (size_t p = 0; p < SN; ++p) {
        mrbf_sd_batch_record &R = records[p];
        const double *t = hTail + p * sdstep::ARMIJO_TAIL;
        std::memset(&R, 0, sizeof(R));
        R.sd_status = hInts[p];
        R.iterations = hInts[SN + 2 * p], R.bound_flips = hInts[SN + 2 * p + 1];
        R.omega = hOmega[p];
        R.omega_step = t[0], R.step_norm = t[1], R.loops = (int32_t)t[2], R.sigma = t[3], R.branch = (int32_t)t[4];
        if (R.sd_status != MRBF_SD_GAVE_UP) continue;
        // the single call refuses this start (take the reference method): its outputs say so
        if (nanrow.empty()) nanrow.assign((size_t)std::max(d, k), std::numeric_limits<double>::quiet_NaN());
        const struct {
            double *out;
            bool dev;
            size_t cnt;
        } outs[3] = {{d_out, dev_d, (size_t)d}, {x_plus, dev_x, (size_t)d}, {mx_plus, dev_m, (size_t)k}};
        for (const auto &o : outs) {
            if (o.dev) MRBF_HIP(ctx, hipMemcpy(o.out + p * o.cnt, nanrow.data(), o.cnt * sizeof(double), hipMemcpyHostToDevice));
            else std::memcpy(o.out + p * o.cnt, nanrow.data(), o.cnt * sizeof(double));
        }
    }
    return MRBF_OK;
}
