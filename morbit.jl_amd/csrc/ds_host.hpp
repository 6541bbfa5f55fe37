// Host logic of the directed-search direction QP (ds_qp.hip: mrbf_ds_direction, mrbf_ds_criticality), free of HIP so that
// tools/ds_host_check.cpp drives it on the CPU under the sanitizers: the constants of the active-set method, the validation behind
// mrbf_ds_direction's return codes, the per-QP workspace in the context arena (what dcall::chunk of descent_call_host.hpp cuts a batch
// into launches by), the iteration cap, and the LDS carve -- one function that the launcher and the kernel both call.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MRBF_DS_HD __host__ __device__
#else
#define MRBF_DS_HD
#endif

namespace mrbf {
namespace ds {

constexpr int THREADS = 256;  // one workgroup per QP
constexpr int MAXD = 4096;    // variables
constexpr int MAXK = 16;      // rows of G: the k x k objects live in LDS and are factorised by one thread

// ---- the constants of the method; morbit.jl_amd/descent.py carries the same values for the host method
constexpr double RANK_TOL = 1e-12;    // a row of M = G_N G_N' whose residual diagonal falls to RANK_TOL M_ii depends on the rows pivoted before it
constexpr double VANISH_TOL = 1e-13;  // a step with |dz_i| <= VANISH_TOL (sum_j |G_ij| + |r_i|) in every row has vanished
constexpr double DUAL_TOL = 1e-11;    // a multiplier violates its sign beyond DUAL_TOL times the magnitudes it was formed from
constexpr double FEAS_TOL = 1e-13;    // sd_lp.hip's FEAS_TOL: the returned d has g_i . d <= FEAS_TOL sum_j |G_ij|

// what mrbf_ds_direction knows before anything is launched (a flag per pointer: given)
struct Call {
    bool has_ctx = false;
    int64_t n_qp = 0;
    int d = 0, k = 0;
    bool G = false, r = false, x = false, lb = false, ub = false;
    bool d_out = false, z_out = false, omega_out = false, status_out = false;  // mult_out and iters_out may be NULL
};

// 0, or the call's return code (include/mrbf.h): -1 no context; -3 n_qp < 1; -4 d outside 1 .. MAXD; -5 k outside 1 .. MAXK; -6 .. -10
// NULL G, r, x, lb, ub; -11 .. -14 NULL d_out, z_out, omega_out, status_out.  -2 is never returned: it is the descent entry points' "take
// the host method".
inline int validate(const Call &c) {
    if (!c.has_ctx) return -1;
    if (c.n_qp < 1) return -3;
    if (c.d < 1 || c.d > MAXD) return -4;
    if (c.k < 1 || c.k > MAXK) return -5;
    if (!c.G) return -6;
    if (!c.r) return -7;
    if (!c.x) return -8;
    if (!c.lb) return -9;
    if (!c.ub) return -10;
    if (!c.d_out) return -11;
    if (!c.z_out) return -12;
    if (!c.omega_out) return -13;
    if (!c.status_out) return -14;
    return 0;
}

// the iteration cap of one QP: steps, drops and multiplier checks all count
MRBF_DS_HD inline int iteration_cap(int d, int k) { return 8 * (d + k) + 16; }

// ---- the d-length state of one QP in the context arena: 4 d doubles (d, p, l, u) and d ints (bound flags)
constexpr int WS_DOUBLES_PER_VAR = 4;
inline size_t ws_doubles(int d) { return (size_t)WS_DOUBLES_PER_VAR * (size_t)d; }
inline size_t ws_ints(int d) { return (size_t)d; }
inline size_t ws_bytes(int d) { return ws_doubles(d) * sizeof(double) + ws_ints(d) * sizeof(int32_t); }

// ---- LDS carve (offsets in bytes, each a multiple of 16): three k x k matrices (M, its factor L, the normal equations A), NVEC vectors
// of MAXK doubles, the reduction scratch (THREADS doubles and THREADS ints), MAXK-int tables and the scalar words
constexpr int NVEC = 20;
constexpr int NIVEC = 3;   // pivot order, pivoted flags, row set S
constexpr int NISC = 16, NDSC = 8;
struct Carve {
    size_t M, L, A, vec, part, ipart, ivec, isc, dsc, total;
};
MRBF_DS_HD inline Carve carve(int k) {
    Carve c{};
    const size_t kk = ((size_t)k * (size_t)k * sizeof(double) + 15) & ~(size_t)15;
    c.M = 0;
    c.L = c.M + kk;
    c.A = c.L + kk;
    c.vec = c.A + kk;
    c.part = c.vec + (size_t)NVEC * MAXK * sizeof(double);
    c.ipart = c.part + (size_t)THREADS * sizeof(double);
    c.ivec = c.ipart + (size_t)THREADS * sizeof(int32_t);
    c.isc = c.ivec + (size_t)NIVEC * MAXK * sizeof(int32_t);
    c.dsc = c.isc + (size_t)NISC * sizeof(int32_t);
    c.total = c.dsc + (size_t)NDSC * sizeof(double);
    return c;
}

}  // namespace ds
}  // namespace mrbf
