// Device functions of the directed-search direction QPs (ds_qp.hip, ds_qp_rows.hip): the k x k work of one QP -- the Cholesky with
// pivots from the row set S first, the step coefficients, the multipliers --, which runs on thread 0 alone in LDS, and the workgroup's
// argmin.  Both kernels run them in the same text (DESIGN.md sections 21 and 23).
#pragma once
#include <hip/hip_runtime.h>

#include "ds_host.hpp"

namespace mrbf {
namespace ds {

enum { I_BAD = 0, I_MODE, I_KIND, I_IDX, I_NHIT, I_ROWHIT };
enum { MODE_STEP = 0, MODE_MULT };
enum { D_ALPHA = 0, D_BEST };
// the vectors of MAXK doubles in the carve
enum { V_Z = 0, V_RHO, V_DZ, V_AV, V_C, V_T, V_BV, V_MU, V_DG, V_TOL, V_W, V_ROWSUM, V_RSCALE, V_R, V_Y, V_YSC, V_AR, V_NVEC };
static_assert(V_NVEC <= NVEC, "carve too small");

// the k x k objects of one QP (LDS); the functions below run on thread 0 alone
struct Small {
    int k;
    double *M, *L, *A, *v;
    int *piv, *done, *inS;
    __device__ double *vec(int which) const { return v + which * MAXK; }
};

// the smallest (v, idx) pair of the workgroup, lowest index on ties, in rv[0] / ri[0]
__device__ inline void block_argmin(double v, int idx, double *rv, int *ri) {
    const int t = threadIdx.x;
    rv[t] = v, ri[t] = idx;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double a = rv[t], b = rv[t + s];
            const int ia = ri[t], ib = ri[t + s];
            if (b < a || (b == a && ib < ia)) rv[t] = b, ri[t] = ib;
        }
        __syncthreads();
    }
}

// Cholesky of M with pivots from S first (largest residual diagonal, lowest index on ties), then from the other rows; a row whose residual
// diagonal is within RANK_TOL M_ii is left out, and leaves S if it was there; so is every row once max_rank pivots are taken (the rows
// kernel passes the count of free variables, which bounds the rank whatever rounding leaves on a diagonal; ds_qp.hip passes MAXK: no
// limit).  L is zero on entry.  Returns the rank; n_s: the pivots in S.
__device__ inline int factor(const Small &s, int &n_s, int max_rank) {
    const int k = s.k;
    double *dg = s.vec(V_DG), *tol = s.vec(V_TOL);
    for (int i = 0; i < k; ++i) dg[i] = s.M[i * k + i], tol[i] = RANK_TOL * dg[i], s.done[i] = 0;
    int rank = 0;
    n_s = 0;
    for (int phase = 1; phase >= 0; --phase) {
        for (;;) {
            int best = -1;
            double bv = 0.0;
            for (int i = 0; i < k; ++i)
                if (!s.done[i] && (s.inS[i] != 0) == (phase != 0) && dg[i] > tol[i] && dg[i] > bv) best = i, bv = dg[i];
            if (best < 0 || rank == max_rank) break;
            const int c = rank;
            const double lp = sqrt(dg[best]);
            s.L[best * k + c] = lp;
            s.done[best] = 1;
            s.piv[rank++] = best;
            for (int i = 0; i < k; ++i) {
                if (s.done[i]) continue;
                double acc = s.M[i * k + best];
                for (int q = 0; q < c; ++q) acc -= s.L[i * k + q] * s.L[best * k + q];
                const double v = acc / lp;
                s.L[i * k + c] = v;
                dg[i] -= v * v;
            }
        }
        if (phase) {
            n_s = rank;
            for (int i = 0; i < k; ++i) s.inS[i] = s.done[i];  // a row of S that was left out leaves S: the working set stays independent
        }
    }
    return rank;
}

// a (V_AV) with the minimum-norm step p_N = G_N' a; false where the small normal equations break down
__device__ inline bool step_coeffs(const Small &s, int &n_s_out, int max_rank = MAXK) {
    const int k = s.k;
    double *z = s.vec(V_Z), *rho = s.vec(V_RHO), *c = s.vec(V_C), *tv = s.vec(V_T), *bv = s.vec(V_BV), *av = s.vec(V_AV);
    int n_s;
    const int rank = factor(s, n_s, max_rank);
    n_s_out = n_s;
    for (int a = 0; a < n_s; ++a) {
        const int p = s.piv[a];
        double acc = -z[p];
        for (int q = 0; q < a; ++q) acc -= s.L[p * k + q] * c[q];
        c[a] = acc / s.L[p * k + a];
    }
    const int r2 = rank - n_s;
    int nT = 0;
    for (int i = 0; i < k; ++i) nT += s.inS[i] ? 0 : 1;
    if (r2) {
        for (int i = 0; i < k; ++i) {
            if (s.inS[i]) continue;
            double acc = rho[i];
            for (int q = 0; q < n_s; ++q) acc -= s.L[i * k + q] * c[q];
            tv[i] = acc;
        }
        if (nT == r2) {  // every other row pivoted: a triangular solve in pivot order
            for (int b = 0; b < r2; ++b) {
                const int p = s.piv[n_s + b];
                double acc = tv[p];
                for (int q = 0; q < b; ++q) acc -= s.L[p * k + n_s + q] * c[n_s + q];
                c[n_s + b] = acc / s.L[p * k + n_s + b];
            }
        } else {  // least squares over all other rows: normal equations of the r2 columns, Cholesky
            double *A = s.A;
            for (int a = 0; a < r2; ++a) {
                for (int b = 0; b <= a; ++b) {
                    double acc = 0.0;
                    for (int i = 0; i < k; ++i)
                        if (!s.inS[i]) acc += s.L[i * k + n_s + a] * s.L[i * k + n_s + b];
                    A[a * k + b] = acc;
                }
                double acc = 0.0;
                for (int i = 0; i < k; ++i)
                    if (!s.inS[i]) acc += s.L[i * k + n_s + a] * tv[i];
                bv[a] = acc;
            }
            for (int a = 0; a < r2; ++a)
                for (int b = 0; b <= a; ++b) {
                    double acc = A[a * k + b];
                    for (int q = 0; q < b; ++q) acc -= A[a * k + q] * A[b * k + q];
                    if (a == b) {
                        if (!(acc > 0.0)) return false;
                        A[a * k + a] = sqrt(acc);
                    } else {
                        A[a * k + b] = acc / A[b * k + b];
                    }
                }
            for (int a = 0; a < r2; ++a) {
                double acc = bv[a];
                for (int q = 0; q < a; ++q) acc -= A[a * k + q] * bv[q];
                bv[a] = acc / A[a * k + a];
            }
            for (int a = r2 - 1; a >= 0; --a) {
                double acc = bv[a];
                for (int q = a + 1; q < r2; ++q) acc -= A[q * k + a] * bv[q];
                bv[a] = acc / A[a * k + a];
            }
            for (int a = 0; a < r2; ++a) c[n_s + a] = bv[a];
        }
    }
    for (int i = 0; i < k; ++i) av[i] = 0.0;
    for (int a = rank - 1; a >= 0; --a) {
        double acc = c[a];
        for (int q = a + 1; q < rank; ++q) acc -= s.L[s.piv[q] * k + a] * av[s.piv[q]];
        av[s.piv[a]] = acc / s.L[s.piv[a] * k + a];
    }
    return true;
}

// mu (V_MU): M_PP mu_P = (M rho)_P on the pivoted rows P of S (the first n_s pivots), zero elsewhere
__device__ inline void multipliers(const Small &s, int n_s) {
    const int k = s.k;
    double *rho = s.vec(V_RHO), *mu = s.vec(V_MU), *w = s.vec(V_W);
    for (int i = 0; i < k; ++i) mu[i] = 0.0;
    for (int a = 0; a < n_s; ++a) {
        const int p = s.piv[a];
        double acc = 0.0;
        for (int i = 0; i < k; ++i) acc += s.M[p * k + i] * rho[i];
        for (int q = 0; q < a; ++q) acc -= s.L[p * k + q] * w[q];
        w[a] = acc / s.L[p * k + a];
    }
    for (int a = n_s - 1; a >= 0; --a) {
        double acc = w[a];
        for (int q = a + 1; q < n_s; ++q) acc -= s.L[s.piv[q] * k + a] * mu[s.piv[q]];
        mu[s.piv[a]] = acc / s.L[s.piv[a] * k + a];
    }
}

}  // namespace ds
}  // namespace mrbf
