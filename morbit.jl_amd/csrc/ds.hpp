// What the directed-search entry points share (ds_qp.hip): the host logic of ds_host.hpp and the direction QP's launcher.  The kernel
// takes the QP on a grid dimension and per-QP strides, as sd.hpp's launchers do, so that mrbf_ds_criticality is the batch of one of
// mrbf_ds_direction through the same code.
#pragma once
#include "common.hpp"
#include "ds_host.hpp"
#include "sd.hpp"  // the objective rows of sd_lp.hip's assembly gather G from the evaluation kernels' Jacobians

namespace mrbf {
namespace ds {

// all device pointers; QPs in chunks so that the per-QP workspaces stay below dcall::WS_LIMIT_BYTES.  QP p reads x at x + p x_stride and its
// bounds at lb / ub + p bound_stride (0: one box for every QP); G (k x n column-major), r and the outputs lie in consecutive per-QP blocks.
int launch(mrbf_ctx *ctx, int64_t n_qp, int n, int k, const double *G, const double *r, const double *x, int64_t x_stride, const double *lb,
           const double *ub, int64_t bound_stride, double *d_out, double *z_out, double *omega_out, double *mult_out, int *status_out,
           int *iters_out);

}  // namespace ds
}  // namespace mrbf
