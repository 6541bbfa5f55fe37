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
using chain::batch_fetch;

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
    if (shape->n_lin_eq < 0 || shape->n_lin_ineq < 0) return fail(ctx, -3, "mrbf_normal_step_batch: negative constraint count");
    if ((shape->n_lin_eq && (!shape->A_eq || !shape->b_eq)) || (shape->n_lin_ineq && (!shape->A_ineq || !shape->b_ineq)))
        return fail(ctx, -3, "mrbf_normal_step_batch: linear constraint matrices are NULL");
    if (variable_radius && !(kappa_delta > 0.0)) return fail(ctx, -10, "mrbf_normal_step_batch: kappa_delta = %g", kappa_delta);
    if (n_starts < 1) return fail(ctx, -2, "mrbf_normal_step_batch: %lld starts (ask mrbf_dispatch_normal_batch first)", (long long)n_starts);
    const int64_t N = n_starts;
    // ---- the shape: start 0's models give every slot's output count; every other start must agree
    std::vector<int> kj(nm);
    for (int j = 0; j < nm; ++j) {
        if (!models[j]) return fail(ctx, -4, "mrbf_normal_step_batch: model %d of start 0 is NULL", j);
        kj[j] = models[j]->k;
    }
    // ---- the modelled constraint rows from the roles table (as mrbf_normal_step reads it)
    std::vector<ns::RowSrc> meq_rows, min_rows;
    std::vector<int64_t> joff(nm, 0), voff(nm, 0);
    std::vector<char> used(nm, 0);
    int64_t jtot = 0, vtot = 0;
    for (int j = 0, e = 0; j < nm; ++j)
        for (int c = 0; c < kj[j]; ++c, ++e) {
            const int role = shape->roles[e];
            if (role == MRBF_ROLE_EQ || role == MRBF_ROLE_INEQ) {
                if (!used[j]) {
                    used[j] = 1, joff[j] = jtot, voff[j] = vtot;
                    jtot += (int64_t)kj[j] * d, vtot += kj[j];
                }
                ns::RowSrc s{2, 0, role == MRBF_ROLE_EQ, kj[j], joff[j] + c, voff[j] + c};
                (role == MRBF_ROLE_EQ ? meq_rows : min_rows).push_back(s);
            } else if (role < 0 && role != MRBF_ROLE_NONE) {
                return fail(ctx, -3, "mrbf_normal_step_batch: roles[%d] = %d is not a role", e, role);
            }
        }
    const int n_nl = (int)(meq_rows.size() + min_rows.size()), n_lin = shape->n_lin_eq + shape->n_lin_ineq;
    if (mrbf_dispatch_normal_batch(N, d, nm, n_nl, n_lin, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_normal_step_batch: %lld starts / d = %d / %d rows outside the device path (ask mrbf_dispatch_normal_batch first)",
                    (long long)N, d, n_nl + n_lin);
    for (int64_t p = 0; p < N; ++p)
        for (int j = 0; j < nm; ++j) {
            const mrbf_model *M = models[p * nm + j];
            if (!M) return fail(ctx, -4, "mrbf_normal_step_batch: model %d of start %lld is NULL", j, (long long)p);
            if (M->d != d || M->k != kj[j])
                return fail(ctx, -4, "mrbf_normal_step_batch: model %d of start %lld is %d variables x %d outputs, expected %d x %d", j, (long long)p,
                            M->d, M->k, d, kj[j]);
            if (used[j] && M->n == 0) return fail(ctx, -4, "mrbf_normal_step_batch: model %d of start %lld has no centres", j, (long long)p);
        }
    const int meq = shape->n_lin_eq + (int)meq_rows.size(), min = shape->n_lin_ineq + (int)min_rows.size(), m = meq + min;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- the evaluations of the single calls (one query row at x per model slot with constraint rows), grouped (batch_chain.hpp)
    chain::Plan ev;
    for (int64_t p = 0; p < N; ++p)
        for (int j = 0; j < nm; ++j)
            if (used[j]) ev.add(ctx, 0, p, j, models[p * nm + j], 1, true);
    ev.close();
    // ---- the arena (doubles; every piece a multiple of 16): upload | work | evaluation scratch | output block
    size_t total = 0;
    auto take = [&](size_t cnt) {
        const size_t at = total;
        total += (cnt + 15) & ~(size_t)15;
        return at;
    };
    const size_t nlin = (size_t)n_lin, SN = (size_t)N;
    const size_t oX = take(SN * d), oDelta = take(SN), oLb = take(d), oUb = take(d), oA = take(nlin * d), oB = take(nlin);
    const size_t oDesc = take(ev.desc_doubles());
    const size_t up_cnt = total;
    const size_t oJ = take(SN * jtot), oV = take(SN * vtot);
    const size_t oAeq = take(SN * meq * d), oBeq = take(SN * meq), oAin = take(SN * min * d), oBin = take(SN * min);
    const size_t oAlpha = take(SN), oInts = take((3 * SN + 1) / 2);
    ev.carve(take);
    for (chain::Member &mb : ev.mem) {
        const size_t p = (size_t)mb.p;
        mb.X = oX + p * d, mb.vals = oV + p * vtot + voff[mb.j], mb.jacs = oJ + p * jtot + joff[mb.j];
    }
    // the output block: n | x + n | duals | records
    const size_t out0 = total;
    const size_t oN = take(SN * d), oXn = take(SN * d), oDual = take(SN * m);
    const size_t oRec = take(SN * sizeof(mrbf_normal_batch_record) / sizeof(double));
    const size_t out_cnt = total - out0;
    double *base;
    MRBF_TRY(get_buf(ctx, S_NS_BATCH, total, &base));
    // ---- the upload, staged in the pinned block where it fits
    std::vector<double> hup_v;
    double *hup = reinterpret_cast<double *>(up_cnt * sizeof(double) <= ((size_t)4 << 20) ? pin_take(ctx, up_cnt * sizeof(double)) : nullptr);
    if (!hup) {
        hup_v.resize(up_cnt);
        hup = hup_v.data();
    }
    std::memset(hup, 0, up_cnt * sizeof(double));
    MRBF_TRY(batch_fetch(ctx, x, SN * d, hup + oX));
    MRBF_TRY(batch_fetch(ctx, delta, SN, hup + oDelta));
    MRBF_TRY(batch_fetch(ctx, lb, d, hup + oLb));
    MRBF_TRY(batch_fetch(ctx, ub, d, hup + oUb));
    MRBF_TRY(batch_fetch(ctx, shape->A_eq, (size_t)shape->n_lin_eq * d, hup + oA));
    MRBF_TRY(batch_fetch(ctx, shape->A_ineq, (size_t)shape->n_lin_ineq * d, hup + oA + (size_t)shape->n_lin_eq * d));
    MRBF_TRY(batch_fetch(ctx, shape->b_eq, shape->n_lin_eq, hup + oB));
    MRBF_TRY(batch_fetch(ctx, shape->b_ineq, shape->n_lin_ineq, hup + oB + shape->n_lin_eq));
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
    {
        int r = 0;
        for (int i = 0; i < shape->n_lin_eq; ++i) aa.src[r++] = ns::RowSrc{1, i, 1, 1, 0, i};
        for (size_t i = 0; i < meq_rows.size(); ++i) aa.src[r] = meq_rows[i], aa.src[r++].dst = shape->n_lin_eq + (int)i;
        for (int i = 0; i < shape->n_lin_ineq; ++i) aa.src[r++] = ns::RowSrc{1, i, 0, 1, 0, shape->n_lin_eq + i};
        for (size_t i = 0; i < min_rows.size(); ++i) aa.src[r] = min_rows[i], aa.src[r++].dst = shape->n_lin_ineq + (int)i;
    }
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
    std::vector<double> hout_v;
    double *hout = reinterpret_cast<double *>(out_cnt * sizeof(double) <= ((size_t)4 << 20) ? pin_take(ctx, out_cnt * sizeof(double)) : nullptr);
    if (!hout) {
        hout_v.resize(out_cnt);
        hout = hout_v.data();
    }
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
