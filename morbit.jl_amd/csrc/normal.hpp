// What the normal-step entry points share: the LP's launcher and the row assembly of normal_lp.hip.  Both kernels take the start on a
// grid dimension and per-start strides, so that the single call (mrbf_normal_step) is the batch of one of mrbf_normal_step_batch
// (normal_batch.hip) through the same code.
#pragma once
#include "common.hpp"

namespace mrbf {
namespace ns {

constexpr int THREADS = 256;
constexpr int MAXM = 64;
constexpr int MAXD = 4096;

// ---- the right-hand sides of the normal step: one workgroup per LP row and start (RowSrc and its filler: descent_problem.hpp); only
// linear (kind 1) and modelled constraint rows (kind 2), Jacobian and value both at x
using descent::RowSrc;
struct AsmArgs {
    int n, rows, meq, min;
    int64_t sJ, sV, sx;  // per-start strides of J, of V, of x; A_eq, b_eq, A_ineq, b_ineq lie in the consecutive per-LP blocks of launch()
    const double *J, *V, *x, *Alin, *blin;  // Alin / blin: the one MOP's linear rows, shared by the starts
    double *Aeq, *beq, *Ain, *bin;
    RowSrc src[MAXM];
};
int launch_assemble(mrbf_ctx *ctx, const AsmArgs &a, int64_t n_starts);

// all device pointers; LPs in chunks so that the per-LP workspace stays below 256 MB.  LP p reads its bounds at lb / ub + p bound_stride
// (0: one box for every LP); everything else lies in consecutive per-LP blocks.
int launch(mrbf_ctx *ctx, int64_t n_lp, int n, int meq, int min, const double *x, const double *lb, const double *ub, int64_t bound_stride,
           const double *Aeq, const double *beq, const double *Ain, const double *bin, double *n_out, double *alpha_out, double *dual_out,
           int *status_out, int *iters_out);

}  // namespace ns
}  // namespace mrbf
