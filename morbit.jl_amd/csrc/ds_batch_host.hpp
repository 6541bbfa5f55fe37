// Host logic of the many-start directed-search call (ds_batch.hip: mrbf_ds_iterate_batch), free of HIP so that
// tools/ds_batch_host_check.cpp drives it on the CPU under the sanitizers: the validation behind the call's return codes, the layout
// of the chain's one device arena, and the packing of a start's record from the words the kernels leave in the output block.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/mrbf.h"

namespace mrbf {
namespace dsbatch {

constexpr int SCALE_THREADS = 256;    // ds_scale_kernel: one workgroup per start
constexpr int64_t MAX_STARTS = 65535;  // the start is a grid dimension of the evaluation and assembly kernels
constexpr int TAIL = 5;                // words per start the Armijo kernel leaves: [omega_step, step_norm, loops, sigma, branch] (sd.hpp)

// what mrbf_ds_iterate_batch knows before anything is read or launched (a flag per pointer: given)
struct Call {
    bool has_ctx = false;
    int64_t n_starts = 0;
    bool shape = false, models = false, x = false, x_n = false, delta = false, lb = false, ub = false, r = false, opts = false;
    bool d_out = false, x_plus = false, mx_plus = false, records = false;  // mult_out and ms_total may be NULL
    double shrink = 0.5;                                                   // opts->shrink where opts is given
    int n_models = 1;                                                      // shape->n_models where shape is given
    bool roles = true;                                                     // shape->roles != NULL where shape is given
};

// 0, or the call's return code (include/mrbf.h): -1 no context; -3 NULL shape, or a shape without models or without a roles table; -4
// NULL models; -5 .. -10 NULL x, x_n, delta, lb, ub, r; -11 NULL opts or shrink outside (0, 1); -12 .. -15 NULL d_out, x_plus, mx_plus,
// records; then -2 for a start count outside 1 .. MAX_STARTS (the first row of mrbf_dispatch_ds_batch; the rest of the table is asked
// once the models' shapes are read)
inline int validate(const Call &c) {
    if (!c.has_ctx) return -1;
    if (!c.shape) return -3;
    if (!c.models) return -4;
    if (!c.x) return -5;
    if (!c.x_n) return -6;
    if (!c.delta) return -7;
    if (!c.lb) return -8;
    if (!c.ub) return -9;
    if (!c.r) return -10;
    if (!c.opts) return -11;
    if (!c.d_out) return -12;
    if (!c.x_plus) return -13;
    if (!c.mx_plus) return -14;
    if (!c.records) return -15;
    if (!(c.shrink > 0.0 && c.shrink < 1.0)) return -11;
    if (c.n_models < 1 || !c.roles) return -3;
    if (c.n_starts < 1 || c.n_starts > MAX_STARTS) return -2;
    return 0;
}

// ---- the arena, counted in doubles.  Every offset is a multiple of 16; [0, up_cnt) is the one upload, [out0, out0 + out_cnt) the one
// read-back, and the evaluation scratch (chain::Plan::carve, `scratch` doubles) lies between the work pieces and the output block.
struct Sizes {
    int64_t n_starts = 0;
    int d = 0, k = 0, max_loops = 0;
    size_t jtot = 0;      // per start: the Jacobians of the objective slots at x_n (sum of k_j d)
    size_t otot = 0;      // per start: the values of the objective slots at the max_loops + 2 trial rows (sum of (max_loops + 2) k_j)
    size_t desc_dbl = 0;  // the evaluation descriptors
    size_t scratch = 0;   // the evaluation scratch
};
struct Layout {
    // upload
    size_t pairs, delta, lb, ub, r, desc, up_cnt;
    // work
    size_t J, G, draw, z, omega_step, steps, sig, X, VO, scratch;
    // output block
    size_t out0, xp, mxp, tail, dir, mult, omega, dnorm, ints, out_cnt;
    size_t total;
};
inline size_t pad16(size_t cnt) { return (cnt + 15) & ~(size_t)15; }
inline size_t ints_doubles(size_t n_starts) { return (3 * n_starts + 1) / 2; }  // status, then (iterations, dropped) per start
inline Layout layout(const Sizes &s) {
    Layout L{};
    size_t at = 0;
    auto take = [&](size_t cnt) {
        const size_t o = at;
        at += pad16(cnt);
        return o;
    };
    const size_t N = (size_t)s.n_starts, d = (size_t)s.d, k = (size_t)s.k, loops = (size_t)s.max_loops;
    L.pairs = take(N * 2 * d), L.delta = take(N), L.lb = take(d), L.ub = take(d), L.r = take(N * k), L.desc = take(s.desc_dbl);
    L.up_cnt = at;
    L.J = take(N * s.jtot), L.G = take(N * k * d), L.draw = take(N * d), L.z = take(N * k), L.omega_step = take(N);
    L.steps = take(N * (loops + 1)), L.sig = take(N * 2), L.X = take(N * (loops + 2) * d), L.VO = take(N * s.otot);
    L.scratch = take(s.scratch);
    L.out0 = at;
    L.xp = take(N * d), L.mxp = take(N * k), L.tail = take(N * TAIL), L.dir = take(N * d), L.mult = take(N * k), L.omega = take(N);
    L.dnorm = take(N), L.ints = take(ints_doubles(N));
    L.out_cnt = at - L.out0;
    L.total = at;
    return L;
}

// ---- start p's record from the read-back: `ints` = the status words of all starts, then (iterations, dropped) per start
inline void pack(mrbf_ds_batch_record &R, size_t p, size_t n_starts, const int32_t *ints, const double *tail, const double *omega,
                 const double *dnorm) {
    const double *t = tail + p * TAIL;
    std::memset(&R, 0, sizeof(R));
    R.ds_status = ints[p];
    R.iterations = ints[n_starts + 2 * p], R.dropped = ints[n_starts + 2 * p + 1];
    R.omega = omega[p];
    R.omega_step = t[0], R.step_norm = t[1], R.loops = (int32_t)t[2], R.sigma = t[3], R.branch = (int32_t)t[4];
    R.dnorm = dnorm[p];
}

}  // namespace dsbatch
}  // namespace mrbf
