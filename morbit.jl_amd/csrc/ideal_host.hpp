// Host logic of the local-ideal-point calls (ps_solver.hip: mrbf_ideal_point_problem, mrbf_ideal_point_batch), free of HIP so that
// tools/ideal_host_check.cpp drives it on the CPU under the sanitizers: the validation behind the calls' return codes, the layout of
// the host block the outputs are gathered in before they are put where the caller wants them, and the packing of a start's record.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/mrbf.h"

namespace mrbf {
namespace ideal {

constexpr int64_t MAX_STARTS = 65535;  // the start is a grid dimension of the population kernels (mrbf_dispatch_ps_batch)
constexpr int MAX_OBJECTIVES = 8;      // a bit per objective in mrbf_ideal_info::found / refined (ps::MAXOBJ)

// what a call knows before anything is read or launched (a flag per pointer: given)
struct Call {
    bool has_ctx = false;
    bool batch = false;     // mrbf_ideal_point_batch: `models` and `n_starts` are arguments of their own
    int64_t n_starts = 1;
    bool problem = false, models = false, x_n = false, lb = false, ub = false, opts = false, ideal_out = false, info = false;
    // x_ideal_out, mx_out, seeds and ms_total may be NULL
    int n_models = 1;       // problem->n_models where the problem is given
    bool roles = true;      // problem->roles != NULL where the problem is given
};

// 0, or the call's return code (include/mrbf.h): -1 no context; -3 NULL problem / shape, or one without models or without a roles
// table; -4 NULL models (the batch; the single call's handles are the problem's, hence -3); -5 NULL x_n; -6 NULL lb_eff; -7 NULL
// ub_eff; -8 NULL opts; -9 NULL ideal_out; -10 NULL info / infos; then -2 for a start count outside 1 .. MAX_STARTS (the first row of
// mrbf_dispatch_ideal_batch; the rest of the table is asked once the models' shapes are read)
inline int validate(const Call &c) {
    if (!c.has_ctx) return -1;
    if (!c.problem) return -3;
    if (!c.models) return c.batch ? -4 : -3;
    if (!c.x_n) return -5;
    if (!c.lb) return -6;
    if (!c.ub) return -7;
    if (!c.opts) return -8;
    if (!c.ideal_out) return -9;
    if (!c.info) return -10;
    if (c.n_models < 1 || !c.roles) return -3;
    if (c.batch && (c.n_starts < 1 || c.n_starts > MAX_STARTS)) return -2;
    return 0;
}

// ---- the output block, counted in doubles: [ideal: n_starts x k][mx: n_starts x k][x_ideal: n_starts x k x d].  The block is filled
// whether or not the optional outputs were given; nothing of it reaches the caller before the whole call has succeeded.
struct Layout {
    size_t ideal, mx, x_ideal, total;
    size_t k, d;
    size_t ideal_at(size_t p, size_t l) const { return ideal + p * k + l; }
    size_t mx_at(size_t p, size_t l) const { return mx + p * k + l; }
    size_t x_ideal_at(size_t p, size_t l) const { return x_ideal + (p * k + l) * d; }  // d doubles from here
};
inline Layout layout(int64_t n_starts, int d, int k) {
    Layout L{};
    const size_t N = (size_t)n_starts;
    L.k = (size_t)k, L.d = (size_t)d;
    L.ideal = 0, L.mx = N * L.k, L.x_ideal = 2 * N * L.k;
    L.total = L.x_ideal + N * L.k * L.d;
    return L;
}

// ---- a start's record: found[l] / refined[l] != 0 -> bit l of the masks
inline void pack(mrbf_ideal_info &I, int k, int evals_ideal, int generations, const char *found, const char *refined) {
    std::memset(&I, 0, sizeof(I));
    I.evals_ideal = evals_ideal, I.generations = generations;
    for (int l = 0; l < k && l < MAX_OBJECTIVES; ++l) {
        if (found[l]) I.found |= (int32_t)1 << l;
        if (refined[l]) I.refined |= (int32_t)1 << l;
    }
}

}  // namespace ideal
}  // namespace mrbf
