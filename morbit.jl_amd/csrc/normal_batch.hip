// Many-start normal step: compute_normal_step (Morbit.jl src/descent.jl:691-757) for n_starts independent starts of one problem in one
// call -- the reference's Threads.@threads loop over Halton starts (examples/large_scale_benchmarks.jl:102-109), where every start
// carries its own surrogate container of one shared shape.  For start p the outputs are, bit for bit, those of mrbf_normal_step on
// start p's container: the assembly and LP kernels are the single call's own, with the start on a grid dimension (normal.hpp), and
// the evaluations are the single call's, member by member (batch_chain.hpp).
//
// One call is one chain on the ctx stream and one read-back, with no host synchronisation in between:
//   one packed upload           x, delta, lb, ub, the linear rows, the evaluation descriptors
//   eval_fused_batch            values + Jacobians at x of every model slot that carries constraint rows, one launch group per (kernel
//                               and parameters, k, dpad, split or unsplit centre range): one query row per member, as the single call
//                               evaluates it, so the centre-range split and the order of every sum are that call's
//   normal_assemble_kernel      (rows x n_starts)   A_eq / b_eq, A_ineq / b_ineq of every start in consecutive per-LP blocks
//   normal_lp_kernel            (n_starts)          the LPs, all over the one box lb / ub (bound stride 0)
//   normal_finish_kernel        (n_starts x 256)    compute_normal_step's radius rule, NaN rows of the rejected starts, x + n, the records
//   one download of the output block  n | x + n | duals | records  (device to device for outputs given as device pointers)
// The starts share d, the model count, every model slot's output count, the roles table and the linear rows; the number of centres
// and the kernel parameters may differ from start to start (such members fall into different launch groups).  A member the fused
// evaluation does not take (MRBF_OPT_EVAL_IMPL = 1) is evaluated by eval_model on the same stream.  At a homogeneous batch the launch
// count does not depend on n_starts.  DESIGN.md section 13.
#include "batch_chain.hpp"
#include "normal.hpp"

using namespace mrbf;

namespace {

static_assert(sizeof(mrbf_normal_batch_record) == 32, "mrbf_normal_batch_record is 32 bytes");

struct FinishArgs {
    int d, variable_radius;
    double kappa_delta, delta_max;
    const double *x, *delta, *alpha;  // per start d / 1 / 1
    const int *status, *iters;        // status[p]; iterations and bound flips at iters[2 p], iters[2 p + 1]
    double *n, *xn;                   // per start d: the LP's step (rewritten as NaN for a rejected start), x + n
    mrbf_normal_batch_record *rec;
};

// one workgroup per start: the radius of descent.jl:738-757 exactly as mrbf_normal_step forms it on the host (the same division and
// comparison in fp64), NaN / -Inf for a start that is infeasible, gave up or needs a radius above delta_max, then x + n
__global__ __launch_bounds__(ns::THREADS) void normal_finish_kernel(FinishArgs a) {
    const int64_t p = blockIdx.x;
    const int t = threadIdx.x, d = a.d;
    const int status = a.status[p];
    const double alpha = a.alpha[p];
    bool ok = status == MRBF_NS_OK;
    double delta;
    if (ok && a.variable_radius) {
        delta = alpha / a.kappa_delta;
        ok = delta <= a.delta_max;
    } else {
        delta = a.delta[p];
    }
    if (!ok) delta = -__builtin_huge_val();
    const double *x = a.x + p * d;
    double *n = a.n + p * d, *xn = a.xn + p * d;
    for (int j = t; j < d; j += ns::THREADS) {
        if (ok) {
            xn[j] = x[j] + n[j];
        } else {
            n[j] = NAN;
            xn[j] = NAN;
        }
    }
    if (t == 0) {
        mrbf_normal_batch_record r;
        r.status = status, r.iterations = a.iters[2 * p], r.bound_flips = a.iters[2 * p + 1], r.reserved = 0;
        r.alpha = alpha, r.delta = delta;
        a.rec[p] = r;
    }
}

}  // namespace

extern "C" int32_t mrbf_normal_step_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                                          int32_t d, const double *x, const double *lb, const double *ub, const double *delta,
                                          double kappa_delta, double delta_max, int32_t variable_radius, double *n_out, double *x_n_out,
                                          double *dual_out, mrbf_normal_batch_record *records, float *ms_total) {
    if (!ctx) return -1;
    if (ms_total) *ms_total = 0.f;
    if (!shape) return fail(ctx, -3, "shape is NULL");
    if (!x) return fail(ctx, -6, "x is NULL");
    if (!lb) return fail(ctx, -7, "lb is NULL");
    if (!ub) return fail(ctx, -8, "ub is NULL");
    if (!delta) return fail(ctx, -9, "delta is NULL");
    if (!n_out) return fail(ctx, -13, "n_out is NULL");
    if (!records) return fail(ctx, -16, "records is NULL");
    const int nm = shape->n_models;
    if (nm < 0 || (nm > 0 && (!models || !shape->roles))) return fail(ctx, -4, "mrbf_normal_step_batch: models need handles and a roles table");
    if (variable_radius && !(kappa_delta > 0.0)) return fail(ctx, -10, "mrbf_normal_step_batch: kappa_delta = %g", kappa_delta);
    if (n_starts < 1) return fail(ctx, -2, "mrbf_normal_step_batch: %lld starts (ask mrbf_dispatch_normal_batch first)", (long long)n_starts);
    const int64_t N = n_starts;
    // ---- the modelled constraint rows from the roles table (as mrbf_normal_step reads it); the starts' slots agree
    std::vector<descent::SlotShape> slots;
    descent::Shape sh = descent_shape(shape, models, N, slots);
    sh.d = d, sh.batch = true;
    descent::Layout lay;
    if (descent::Defect D = descent::read(sh, {false, descent::Centres::CONSTRAINED_SLOTS}, lay))
        return fail(ctx, D.cls == descent::Defect::MODELS ? -4 : -3, "mrbf_normal_step_batch: %s", D.msg.c_str());
    const int n_lin = shape->n_lin_eq + shape->n_lin_ineq;
    if (mrbf_dispatch_normal_batch(N, d, nm, lay.n_nl, n_lin, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_normal_step_batch: %lld starts / d = %d / %d rows outside the device path (ask mrbf_dispatch_normal_batch first)",
                    (long long)N, d, lay.n_nl + n_lin);
    const descent::Offsets at = lay.offsets(1, descent::Slots::CONSTRAINED);
    const int64_t jtot = at.jtot, vtot = at.vtot;
    const int meq = lay.meq, min = lay.min, m = meq + min;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- the evaluations of the single calls (one query row at x per model slot with constraint rows), grouped (batch_chain.hpp)
    chain::Plan ev;
    for (int64_t p = 0; p < N; ++p)
        for (int j = 0; j < nm; ++j)
            if (lay.has_con[j]) ev.add(ctx, 0, p, j, models[p * nm + j], 1, true);
    ev.close();
    // ---- the arena (doubles; every piece a multiple of 16): upload | work | evaluation scratch | output block
    chain::Arena ar;
    const size_t nlin = (size_t)n_lin, SN = (size_t)N;
    const size_t oX = ar.take(SN * d), oDelta = ar.take(SN), oLb = ar.take(d), oUb = ar.take(d), oA = ar.take(nlin * d), oB = ar.take(nlin);
    const size_t oDesc = ar.take(ev.desc_doubles());
    const size_t up_cnt = ar.total;
    const size_t oJ = ar.take(SN * jtot), oV = ar.take(SN * vtot);
    const size_t oAeq = ar.take(SN * meq * d), oBeq = ar.take(SN * meq), oAin = ar.take(SN * min * d), oBin = ar.take(SN * min);
    const size_t oAlpha = ar.take(SN), oInts = ar.take((3 * SN + 1) / 2);
    ev.carve(ar);
    for (chain::Member &mb : ev.mem) {
        const size_t p = (size_t)mb.p;
        mb.X = oX + p * d, mb.vals = oV + p * vtot + at.val[mb.j], mb.jacs = oJ + p * jtot + at.jac[mb.j];
    }
    // the output block: n | x + n | duals | records
    const size_t out0 = ar.total;
    const size_t oN = ar.take(SN * d), oXn = ar.take(SN * d), oDual = ar.take(SN * m);
    const size_t oRec = ar.take(SN * sizeof(mrbf_normal_batch_record) / sizeof(double));
    const size_t out_cnt = ar.total - out0;
    double *base;
    MRBF_TRY(get_buf(ctx, S_NS_BATCH, ar.total, &base));
    // ---- the upload, staged in the pinned block where it fits
    chain::Staging up(ctx, up_cnt);
    double *hup = up.p;
    std::memset(hup, 0, up_cnt * sizeof(double));
    MRBF_TRY(input_fetch(ctx, x, SN * d, hup + oX));
    MRBF_TRY(input_fetch(ctx, delta, SN, hup + oDelta));
    MRBF_TRY(input_fetch(ctx, lb, d, hup + oLb));
    MRBF_TRY(input_fetch(ctx, ub, d, hup + oUb));
    MRBF_TRY(fetch_linear_rows(ctx, shape, d, hup + oA, hup + oB));
    EvalDesc *hdesc = reinterpret_cast<EvalDesc *>(hup + oDesc);
    const EvalDesc *ddesc = reinterpret_cast<const EvalDesc *>(base + oDesc);
    ev.fill(base, hdesc);
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, st));
    MRBF_HIP(ctx, hipMemcpyAsync(base, hup, up_cnt * sizeof(double), hipMemcpyHostToDevice, st));
    MRBF_TRY(ev.launch(ctx, 0, base, hdesc, ddesc));
    // ---- A_eq / b_eq (linear, then modelled), A_ineq / b_ineq (likewise) of every start
    ns::AsmArgs aa;
    aa.n = d, aa.rows = m, aa.meq = meq, aa.min = min;
    aa.sJ = jtot, aa.sV = vtot, aa.sx = d;
    aa.J = base + oJ, aa.V = base + oV, aa.x = base + oX, aa.Alin = base + oA, aa.blin = base + oB;
    aa.Aeq = base + oAeq, aa.beq = base + oBeq, aa.Ain = base + oAin, aa.bin = base + oBin;
    descent::fill_sources(lay, at, false, aa.src);
    MRBF_TRY(ns::launch_assemble(ctx, aa, N));
    int *dInts = reinterpret_cast<int *>(base + oInts);
    MRBF_TRY(ns::launch(ctx, N, d, meq, min, base + oX, base + oLb, base + oUb, 0, meq ? base + oAeq : nullptr, meq ? base + oBeq : nullptr,
                        min ? base + oAin : nullptr, min ? base + oBin : nullptr, base + oN, base + oAlpha, dual_out ? base + oDual : nullptr,
                        dInts, dInts + N));
    // ---- the radius rule, the rejected starts' NaN rows, x + n and the records
    FinishArgs fa;
    fa.d = d, fa.variable_radius = variable_radius != 0;
    fa.kappa_delta = kappa_delta, fa.delta_max = delta_max;
    fa.x = base + oX, fa.delta = base + oDelta, fa.alpha = base + oAlpha;
    fa.status = dInts, fa.iters = dInts + N;
    fa.n = base + oN, fa.xn = base + oXn;
    fa.rec = reinterpret_cast<mrbf_normal_batch_record *>(base + oRec);
    hipLaunchKernelGGL(normal_finish_kernel, dim3((unsigned)N), dim3(ns::THREADS), 0, st, fa);
    MRBF_HIP(ctx, hipGetLastError());
    // ---- one read-back
    chain::Staging down(ctx, out_cnt);
    double *hout = down.p;
    MRBF_HIP(ctx, hipMemcpyAsync(hout, base + out0, out_cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    const bool dev_n = is_device_ptr(n_out), dev_x = x_n_out && is_device_ptr(x_n_out), dev_y = dual_out && is_device_ptr(dual_out);
    if (dev_n) MRBF_HIP(ctx, hipMemcpyAsync(n_out, base + oN, SN * d * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (dev_x) MRBF_HIP(ctx, hipMemcpyAsync(x_n_out, base + oXn, SN * d * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (dev_y) MRBF_HIP(ctx, hipMemcpyAsync(dual_out, base + oDual, SN * m * sizeof(double), hipMemcpyDeviceToDevice, st));
    MRBF_HIP(ctx, hipEventRecord(e1, st));
    MRBF_HIP(ctx, hipStreamSynchronize(st));
    pin.flush();
    if (ms_total) MRBF_HIP(ctx, hipEventElapsedTime(ms_total, e0, e1));
    if (!dev_n) std::memcpy(n_out, hout + (oN - out0), SN * d * sizeof(double));
    if (x_n_out && !dev_x) std::memcpy(x_n_out, hout + (oXn - out0), SN * d * sizeof(double));
    if (dual_out && !dev_y) std::memcpy(dual_out, hout + (oDual - out0), SN * m * sizeof(double));
    std::memcpy(records, hout + (oRec - out0), SN * sizeof(mrbf_normal_batch_record));
    return MRBF_OK;
}
