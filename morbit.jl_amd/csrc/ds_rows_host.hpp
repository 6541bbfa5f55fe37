// Host logic of the directed-search direction QP with constraint rows (ds_qp_rows.hip: mrbf_ds_direction_rows,
// mrbf_ds_criticality_rows), free of HIP so that tools/ds_rows_host_check.cpp drives it on the CPU under the
// sanitizers: the start tolerance, the row-kind table, the validation behind mrbf_ds_direction_rows' return codes, the per-QP workspace
// (ds_host.hpp's: the d-length state does not grow with the rows) and the LDS carve -- one function that the launcher and the kernel
// both call.  The method's other constants, the iteration cap and the limits are ds_host.hpp's.
#pragma once
#include "ds_host.hpp"

namespace mrbf {
namespace ds {
namespace rows {

// A constraint row that the start d = 0 misses -- |b_eq,i|, or -b_in,i where b_in,i < 0 -- by at most START_TOL sum_j |W_ij| has its
// right-hand side clamped to zero; a larger miss ends the QP with MRBF_DS_NO_START.  What the normal step leaves behind is
// normal_lp.hip's FEAS_TOL = 1e-13 on its own row scale max(1, |b_i| + sum_j |A_ij|): on this scale 1e-13 (1 + |b_i| / sum_j |A_ij|), so
// 1e-10 admits right-hand sides up to a thousand row sums; SLSQP on the host route accepts rows within 1e-9, so a clamped start moves
// the problem by less than the host route's own acceptance.  morbit.jl_amd/descent.py carries the same value (DS_START_TOL).
constexpr double START_TOL = 1e-10;

// ---- the row-kind table: W = [G; A_eq; A_in], objective rows first
enum Kind { OBJECTIVE = 0, EQUALITY = 1, INEQUALITY = 2 };
MRBF_DS_HD inline int kind_of(int i, int k, int m_eq) { return i < k ? OBJECTIVE : (i < k + m_eq ? EQUALITY : INEQUALITY); }
// may a row of this kind be dropped from S for its multiplier's sign / does it block on either side of its right-hand side?
MRBF_DS_HD inline bool droppable(int kind) { return kind != EQUALITY; }
MRBF_DS_HD inline bool two_sided(int kind) { return kind == EQUALITY; }

// what mrbf_ds_direction_rows knows before anything is launched (a flag per pointer: given)
struct Call {
    bool has_ctx = false;
    int64_t n_qp = 0;
    int d = 0, k = 0, m_eq = 0, m_in = 0;
    bool G = false, r = false, x = false, lb = false, ub = false;
    bool A_eq = false, b_eq = false, A_in = false, b_in = false;               // may be NULL where their count is 0
    bool d_out = false, c_out = false, omega_out = false, status_out = false;  // mult_out and iters_out may be NULL
};

// 0, or the call's return code (include/mrbf.h): -1 no context; -3 n_qp < 1; -4 d outside 1 .. MAXD; -5 k outside 1 .. MAXK; -6 m_eq < 0;
// -7 m_in < 0; -8 k + m_eq + m_in > MAXK; -9 .. -13 NULL G, r, x, lb, ub; -14 / -15 NULL A_eq / b_eq with m_eq > 0; -16 / -17 NULL A_in /
// b_in with m_in > 0; -18 .. -21 NULL d_out, c_out, omega_out, status_out.  -2 is never returned: it is the descent entry points' "take
// the host method".
inline int validate(const Call &c) {
    if (!c.has_ctx) return -1;
    if (c.n_qp < 1) return -3;
    if (c.d < 1 || c.d > MAXD) return -4;
    if (c.k < 1 || c.k > MAXK) return -5;
    if (c.m_eq < 0) return -6;
    if (c.m_in < 0) return -7;
    if ((int64_t)c.k + c.m_eq + c.m_in > MAXK) return -8;
    if (!c.G) return -9;
    if (!c.r) return -10;
    if (!c.x) return -11;
    if (!c.lb) return -12;
    if (!c.ub) return -13;
    if (c.m_eq && !c.A_eq) return -14;
    if (c.m_eq && !c.b_eq) return -15;
    if (c.m_in && !c.A_in) return -16;
    if (c.m_in && !c.b_in) return -17;
    if (!c.d_out) return -18;
    if (!c.c_out) return -19;
    if (!c.omega_out) return -20;
    if (!c.status_out) return -21;
    return 0;
}

// the doubles of one QP's inputs in the call's arena: G, r, x, lb, ub, A_eq, b_eq, A_in, b_in
inline size_t input_doubles(int d, int k, int m_eq, int m_in) {
    return (size_t)k * d + (size_t)k + 3 * (size_t)d + (size_t)(m_eq + m_in) * ((size_t)d + 1);
}

// ---- LDS carve (offsets in bytes, each a multiple of 16): ds_host.hpp's carve with a fourth K x K matrix -- M over all K rows next to
// its restriction MU to the universe U that the K x K work runs on --, NVEC vectors of MAXK doubles (the compact ones of the K x K work
// and the full-length ones of the rows) and NIVEC tables of MAXK ints (pivot order, pivoted flags, S on U, S, U)
constexpr int NVEC = 24;
constexpr int NIVEC = 5;
struct Carve {
    size_t M, MU, L, A, vec, part, ipart, ivec, isc, dsc, total;
};
MRBF_DS_HD inline Carve carve(int K) {
    Carve c{};
    const size_t kk = ((size_t)K * (size_t)K * sizeof(double) + 15) & ~(size_t)15;
    c.M = 0;
    c.MU = c.M + kk;
    c.L = c.MU + kk;
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

}  // namespace rows
}  // namespace ds
}  // namespace mrbf
