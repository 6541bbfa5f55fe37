// The normal step on the device: the LP of compute_normal_step (src/descent.jl:691-757) and the whole call around it.
//
// One workgroup solves one LP, in the step n = x_new - x:
//   minimise alpha over (n, alpha)  s.t.  -alpha <= n_j <= alpha,  l'_j <= n_j <= u'_j (l' = lb - x, u' = ub - x),
//   A_eq n = b_eq,  A_ineq n <= b_ineq,  alpha >= alpha0 = max(0, max_j l'_j, max_j -u'_j)  (implied, so alpha* is unchanged).
// by an active-set dual simplex over the constraints.  The working set W holds d + 1 constraints: every n_j is either free or
// pinned by one of its four constraints (box below / above: n_j = l'_j / u'_j; band below / above: n_j = -alpha / +alpha), the
// C rows in W hold with equality, and at most one more member fixes alpha (alpha >= alpha0, or a second constraint of one pinned
// column).  Pinned columns are substituted out, which leaves a dense system M in (free n_j, alpha) whose rows are the C rows in W
// and the alpha-fixing member: M is at most (m + 1) x (m + 1) and its inverse lives in LDS; the band pins only add +-C_j to
// alpha's column of M.  The start (every n_j pinned where |n_j| is smallest at alpha0, on the side the violated rows prefer;
// alpha = alpha0) is dual feasible.  The costs of the columns are perturbed (+-1e-12 w_j / sqrt(d) on n_j, the sign of the start
// pin), so every pin starts with a positive multiplier of its own and the pivots do not stall on the d zero multipliers of the
// unperturbed start; the primal point depends on W alone, so it is a vertex of the true LP, and its alpha exceeds alpha* by at
// most the perturbation's weight.  Each iteration prices the most violated constraint (its violation over the length of its
// normal), expresses its normal in W (a transposed solve with M^-1 and one pass over the columns) and removes a member whose
// multiplier reaches zero first: Harris' two-pass ratio test (multipliers within 1e-12 of zero count as zero; among those the
// largest rate, ties to the lower constraint index).  M^-1 is rebuilt by Gauss-Jordan with partial pivoting every iteration, so
// nothing accumulates; the primal point and the multipliers are recomputed from it.  A result is accepted only when, besides
// primal feasibility, every multiplier of an inequality member of W is >= -DUAL_TOL (else GAVE_UP).  Every sum runs in a fixed order that
// depends on the shape alone, and no atomics touch values: an LP's result does not depend on its position in the batch.
#include "descent_call.hpp"
#include "lp_dev.hpp"
#include "normal.hpp"

namespace mrbf {
namespace ns {

static_assert(THREADS == lp::THREADS, "row_pass and invert run on a workgroup of lp::THREADS");

constexpr double FEAS_TOL = 1e-13;    // relative to the constraint's magnitude
constexpr double PIVOT_TOL = 1e-9;    // ratio-test candidates: rate > PIVOT_TOL * the largest |rate|
constexpr double PIVOT_FLOOR = 1e-13; // ... and > PIVOT_FLOOR (a lone rate at rounding level is no pivot)
constexpr double HARRIS_TOL = 1e-12;  // ratio test: multipliers this close to zero count as zero (Harris' two passes)
constexpr double DUAL_TOL = 1e-9;     // accepted optimum: multipliers of inequality members >= -DUAL_TOL max(1, max |multiplier|)
constexpr double PERTURB = 1e-12;     // cost perturbation of the columns: PERTURB * w_j / sqrt(d), w_j in [1, 2)

enum { BOXL = 0, BOXU = 1, BANDL = 2, BANDU = 3 };  // pin types; pin[j] < 0: free in slot -1 - pin[j]
enum { FIX_NONE = 0, FIX_APIN = 1, FIX_DOUBLE = 2 };
__host__ __device__ inline int sgn(int t) { return (t & 1) ? 1 : -1; }
__host__ __device__ inline int tau(int t) { return t >> 1; }

struct Args {
    int n, meq, min, m;
    int64_t bs;  // LP p reads lb / ub at + p * bs (0: one box for every LP)
    const double *x, *lb, *ub, *Aeq, *beq, *Ain, *bin;
    double *n_out, *alpha_out, *dual_out;
    int *status_out, *iters_out;
    double *ws;  // per LP 6 n doubles: n, l', u', rates, multipliers of the pins, perturbed costs
    int *wsi;    // per LP n ints: the pin of each column
};

struct Lp {
    const double *Aeq, *Ain;
    int n, meq;
    __device__ double c(int i, int j) const { return i < meq ? Aeq[(size_t)i * n + j] : Ain[(size_t)(i - meq) * n + j]; }
};

// per-LP scalars in LDS
struct Sc {
    int nr, nf, fix, fixj, fixt, act, enter, enter_dir, status, iters, flips;
};

enum { A_PIVOT = 0, A_DONE, A_GIVEUP };

// LDS carve; offsets in bytes, multiples of 16
struct Carve {
    size_t minv, aug, vec, part, pidx, lists, sc, total;
};
// sized by the LP's rows: M is at most ms x ms with ms = m + 1, so LPs with few rows share a CU
__host__ __device__ inline Carve carve(int ms) {
    Carve c;
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    c.minv = 0;
    c.aug = up(c.minv + (size_t)ms * ms * sizeof(double));
    c.vec = up(c.aug + (size_t)ms * 2 * ms * sizeof(double));
    c.part = up(c.vec + (size_t)14 * ms * sizeof(double));
    c.pidx = up(c.part + (size_t)2 * THREADS * sizeof(double));
    c.lists = up(c.pidx + (size_t)THREADS * sizeof(int));
    c.sc = up(c.lists + (size_t)3 * ms * sizeof(int));
    c.total = up(c.sc + sizeof(Sc));
    return c;
}

// (key, index) reduction over the workgroup: better(a, b) decides; ties of every kind are settled by the caller's comparison
template <class B>
__device__ void argbest(double *key, double *key2, int *idx, B better) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s && better(key[t + s], key2[t + s], idx[t + s], key[t], key2[t], idx[t]))
            key[t] = key[t + s], key2[t] = key2[t + s], idx[t] = idx[t + s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void normal_lp_kernel(Args a, int64_t lp0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t lp = lp0 + blockIdx.x;
    const int t = threadIdx.x, n = a.n, m = a.m, meq = a.meq;
    const int ms = m + 1;
    const Carve cv = carve(ms);
    double *Minv = (double *)(smem + cv.minv), *aug = (double *)(smem + cv.aug), *vec = (double *)(smem + cv.vec);
    double *aal = vec, *ccon = vec + ms, *rhs = vec + 2 * ms, *z = vec + 3 * ms, *rv = vec + 4 * ms, *mur = vec + 5 * ms;
    double *lamr = vec + 6 * ms, *bt = vec + 7 * ms, *cn = vec + 8 * ms, *cabs = vec + 9 * ms, *rowbuf = vec + 10 * ms;
    double *part = (double *)(smem + cv.part), *part2 = part + THREADS;
    int *pidx = (int *)(smem + cv.pidx), *lists = (int *)(smem + cv.lists);
    int *F = lists, *R = lists + ms, *inR = lists + 2 * ms;
    Sc &S = *(Sc *)(smem + cv.sc);
    double *cmaxv = vec + 12 * ms, *cnrm = vec + 13 * ms;  // rowbuf takes 2 ms

    const Lp L{a.Aeq ? a.Aeq + lp * meq * n : nullptr, a.Ain ? a.Ain + lp * a.min * n : nullptr, n, meq};
    const double *x = a.x + lp * n, *lb = a.lb + lp * a.bs, *ub = a.ub + lp * a.bs;
    double *nv = a.ws + (size_t)blockIdx.x * 6 * n, *lo = nv + n, *hi = nv + 2 * n, *mu = nv + 3 * n, *lam = nv + 4 * n, *pc = nv + 5 * n;
    int *pin = a.wsi + (size_t)blockIdx.x * n;
    const double INF = __builtin_huge_val();
    auto bval = [&](int ty, int j) { return ty == BOXL ? -lo[j] : (ty == BOXU ? hi[j] : 0.0); };  // right-hand side of a pin

    // ---- bounds of the step, alpha0, right-hand sides
    double amax = 0.0;
    int bad = 0;
    for (int j = t; j < n; j += THREADS) {
        const double l = lb[j] - x[j], u = ub[j] - x[j];
        lo[j] = l, hi[j] = u;
        if (!(l <= u)) bad = 1;
        amax = fmax(amax, fmax(l, -u));
    }
    part[t] = amax;
    bad = __syncthreads_or(bad);
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) part[t] = fmax(part[t], part[t + s]);
        __syncthreads();
    }
    const double a0 = part[0];
    if (!(a0 < INF)) bad = 1;
    if (t < m) bt[t] = t < meq ? a.beq[lp * meq + t] : a.bin[lp * a.min + t - meq], inR[t] = 0;
    if (t == 0) {
        S.nr = 0, S.nf = 0, S.fix = FIX_APIN, S.fixj = -1, S.fixt = -1, S.iters = 0, S.flips = 0;
        S.status = bad ? MRBF_NS_INFEASIBLE : MRBF_NS_OK;
    }
    __syncthreads();
    // ---- start: each n_j pinned where |n_j| is smallest at alpha0, then turned to the side the violated rows prefer
    if (S.status == MRBF_NS_OK) {
        for (int j = t; j < n; j += THREADS) {
            const double Lv = fmax(lo[j], -a0), Uv = fmin(hi[j], a0);
            const int pl = lo[j] >= -a0 ? BOXL : BANDL, pu = hi[j] <= a0 ? BOXU : BANDU;
            pin[j] = fabs(Lv) <= fabs(Uv) ? pl : pu;
            nv[j] = fabs(Lv) <= fabs(Uv) ? Lv : Uv;
        }
        __syncthreads();
        if (m > 0) {
            lp::row_pass(n, m, [&](int i, int j) { return L.c(i, j) * nv[j]; }, part, cn);
            lp::row_pass(n, m, [&](int i, int j) { return fabs(L.c(i, j)); }, part, cabs);
            lp::row_pass(n, m, [&](int i, int j) { const double v = L.c(i, j); return v * v; }, part, cnrm);
            if (t < m) cnrm[t] = cnrm[t] > 0.0 ? sqrt(cnrm[t]) : 1.0;
            if (t < m) {
                const double r = cn[t] - bt[t], tol = FEAS_TOL * fmax(1.0, fabs(bt[t]) + cabs[t] * fmax(1.0, a0));
                rowbuf[t] = cabs[t] > 0.0 ? (r > tol ? 1.0 / cabs[t] : (t < meq && r < -tol ? -1.0 / cabs[t] : 0.0)) : 0.0;
            }
            __syncthreads();
            for (int j = t; j < n; j += THREADS) {
                double g = 0.0;
                for (int i = 0; i < m; ++i) g += rowbuf[i] * L.c(i, j);
                if (g > 0.0) pin[j] = lo[j] >= -a0 ? BOXL : BANDL;
                else if (g < 0.0) pin[j] = hi[j] <= a0 ? BOXU : BANDU;
            }
            __syncthreads();
        }
        // the perturbed costs: every pin starts with a small positive multiplier of its own, so the pivots are not degenerate
        const double eps = PERTURB / sqrt((double)n);
        for (int j = t; j < n; j += THREADS) {
            const double w = 1.0 + (double)((unsigned)j * 2654435761u) * 0x1p-32;
            pc[j] = sgn(pin[j]) > 0 ? -eps * w : eps * w;
        }
        __syncthreads();
    }
    const int cap = 8 * (m + n);
    while (S.status == MRBF_NS_OK) {
        const int nr = S.nr, nf = S.nf, sz = nf + 1, fix = S.fix;
        // ---- M: rows R (then the alpha-fixing member), columns the free n_j (then alpha)
        if (m > 0) {
            lp::row_pass(n, m, [&](int i, int j) { const int p = pin[j]; return p >= BANDL ? sgn(p) * L.c(i, j) : 0.0; }, part, aal);
            lp::row_pass(n, m, [&](int i, int j) { const int p = pin[j]; return (p == BOXL || p == BOXU) ? L.c(i, j) * sgn(p) * bval(p, j) : 0.0; },
                     part, ccon);
        }
        double kap = -1.0, rf = -a0;
        if (fix == FIX_DOUBLE) {
            const int t1 = pin[S.fixj], t2 = S.fixt;
            kap = (double)(sgn(t1) * sgn(t2) * tau(t1) - tau(t2));
            rf = bval(t2, S.fixj) - sgn(t1) * sgn(t2) * bval(t1, S.fixj);
        }
        const int W = 2 * sz;
        for (int e = t; e < sz * W; e += THREADS) {
            const int p = e / W, c = e % W;
            double v;
            if (c >= sz) v = (c - sz == p) ? 1.0 : 0.0;
            else if (p < nr) v = c < nf ? L.c(R[p], F[c]) : aal[R[p]];
            else v = c < nf ? 0.0 : kap;
            aug[e] = v;
        }
        if (t < nr) rhs[t] = bt[R[t]] - ccon[R[t]];
        if (t == 0 && fix != FIX_NONE) rhs[nr] = rf;
        __syncthreads();
        if (!lp::invert(sz, aug, Minv, rowbuf, part, cmaxv, pidx)) {
            if (t == 0) S.status = MRBF_NS_GAVE_UP;
            __syncthreads();
            break;
        }
        // ---- primal point z = M^-1 rhs; multipliers of the rows lamr = -(M^-T c~) for the perturbed costs c~ = (pc, 1)
        lp::row_pass(n, 1, [&](int, int j) { const int p = pin[j]; return p >= BANDL ? sgn(p) * pc[j] : 0.0; }, part, rv + nf);
        if (t < nf) rv[t] = pc[F[t]];
        if (t == nf) rv[t] += 1.0;
        __syncthreads();
        if (t < sz) {
            double acc = 0.0, al = 0.0;
            for (int p = 0; p < sz; ++p) acc += Minv[t * sz + p] * rhs[p];
            for (int v = 0; v < sz; ++v) al += Minv[v * sz + t] * rv[v];
            z[t] = acc;
            lamr[t] = -al;
        }
        __syncthreads();
        const double alpha = z[nf];
        // ---- the columns: n_j, multipliers of the pins, violations of the column constraints
        double best = 0.0;
        int bid = 0x7fffffff;
        for (int j = t; j < n; j += THREADS) {
            const int p = pin[j];
            double v;
            if (p < 0) {
                v = z[-1 - p];
                lam[j] = 0.0;
            } else {
                v = sgn(p) * (bval(p, j) + tau(p) * alpha);
                double cm = 0.0;
                for (int q = 0; q < nr; ++q) cm += lamr[q] * L.c(R[q], j);
                if (fix == FIX_DOUBLE && S.fixj == j) cm += sgn(S.fixt) * lamr[nr];
                lam[j] = -sgn(p) * (pc[j] + cm);  // the pin's multiplier: its part of -(A_W^-T c~)
            }
            nv[j] = v;
            const double tol = fmax(1.0, fmax(fabs(alpha), fabs(v)));
            for (int ty = 0; ty < 4; ++ty) {
                if (ty == p || (fix == FIX_DOUBLE && S.fixj == j && S.fixt == ty)) continue;
                const double b = bval(ty, j);
                if (!(fabs(b) < INF)) continue;
                const double viol = sgn(ty) * v - tau(ty) * alpha - b, sc = fmax(tol, fabs(b));
                const double key = tau(ty) ? viol * 0.70710678118654752 : viol;  // the violation over the normal's length
                if (viol > FEAS_TOL * sc && key > best) best = key, bid = m + 1 + 4 * j + ty;
            }
        }
        part[t] = best, part2[t] = 0.0, pidx[t] = bid;
        argbest(part, part2, pidx, [](double k, double, int i, double k0, double, int i0) { return k > k0 || (k == k0 && i < i0); });
        const double cbest = part[0];
        const int cid = pidx[0];
        __syncthreads();
        // ---- the rows outside W, alpha >= alpha0
        if (m > 0) {
            lp::row_pass(n, m, [&](int i, int j) { return L.c(i, j) * nv[j]; }, part, cn);
            lp::row_pass(n, m, [&](int i, int j) { return fabs(L.c(i, j) * nv[j]); }, part, cabs);
        }
        if (t == 0) {
            double bv = cbest;
            int id = cid, dir = 1;
            for (int i = 0; i < m; ++i) {
                if (inR[i]) continue;
                const double r = cn[i] - bt[i], sc = fmax(1.0, fabs(bt[i]) + cabs[i]), key = fabs(r) / cnrm[i];
                if (r > FEAS_TOL * sc && (key > bv || (key == bv && i < id))) bv = key, id = i, dir = 1;
                else if (i < meq && -r > FEAS_TOL * sc && (key > bv || (key == bv && i < id))) bv = key, id = i, dir = -1;
            }
            if (fix != FIX_APIN) {
                const double r = a0 - alpha, sc = fmax(1.0, a0), key = r;
                if (r > FEAS_TOL * sc && (key > bv || (key == bv && m < id))) bv = key, id = m, dir = 1;
            }
            S.act = id == 0x7fffffff ? A_DONE : (S.iters >= cap ? A_GIVEUP : A_PIVOT);
            S.enter = id, S.enter_dir = dir;
        }
        __syncthreads();
        if (S.act == A_DONE) break;
        if (S.act == A_GIVEUP) {
            if (t == 0) S.status = MRBF_NS_GAVE_UP;
            __syncthreads();
            break;
        }
        // ---- the entering normal (g, g_alpha) in W: rv = its image in M's columns, mur = M^-T rv, then the rates of the pins
        const int e = S.enter, edir = S.enter_dir;
        const int ej = e > m ? (e - m - 1) >> 2 : -1, et = e > m ? (e - m - 1) & 3 : -1;
        if (t < sz) {
            double v;
            if (t < nf) v = e < m ? edir * L.c(e, F[t]) : (F[t] == ej ? (double)sgn(et) : 0.0);
            else if (e < m) v = edir * aal[e];
            else if (e == m) v = -1.0;
            else v = -tau(et) + (pin[ej] >= BANDL ? (double)(sgn(pin[ej]) * sgn(et)) : 0.0);
            rv[t] = v;
        }
        __syncthreads();
        if (t < sz) {
            double acc = 0.0;
            for (int v = 0; v < sz; ++v) acc += Minv[v * sz + t] * rv[v];
            mur[t] = acc;
        }
        __syncthreads();
        double rmax = 0.0;
        for (int j = t; j < n; j += THREADS) {
            const int p = pin[j];
            if (p < 0) continue;
            double cm = 0.0;
            for (int q = 0; q < nr; ++q) cm += mur[q] * L.c(R[q], j);
            const double g = e < m ? edir * L.c(e, j) : (j == ej ? (double)sgn(et) : 0.0);
            double r = g - cm;
            if (fix == FIX_DOUBLE && S.fixj == j) r -= sgn(S.fixt) * mur[nr];
            mu[j] = sgn(p) * r;
            rmax = fmax(rmax, fabs(mu[j]));
        }
        if (t < nr && R[t] >= meq) rmax = fmax(rmax, fabs(mur[t]));
        if (t == 0 && fix != FIX_NONE) rmax = fmax(rmax, fabs(mur[nr]));
        part[t] = rmax;
        __syncthreads();
        for (int s = THREADS / 2; s > 0; s >>= 1) {
            if (t < s) part[t] = fmax(part[t], part[t + s]);
            __syncthreads();
        }
        const double ptol = fmax(PIVOT_TOL * part[0], PIVOT_FLOOR);
        __syncthreads();
        // ---- ratio test (Harris): the bound tmax on the step from multipliers relaxed by HARRIS_TOL, then among the members whose
        // multiplier reaches zero within tmax the one with the largest rate (ties: the lower index)
        auto each = [&](auto &&f) {
            for (int j = t; j < n; j += THREADS)
                if (pin[j] >= 0) f(mu[j], lam[j], m + 1 + j);
            if (t < nr && R[t] >= meq) f(mur[t], lamr[t], R[t]);
            if (t == 0 && fix != FIX_NONE) f(mur[nr], lamr[nr], m);
        };
        double tm = INF;
        each([&](double rate, double lm, int) {
            if (rate > ptol) tm = fmin(tm, (fmax(lm, 0.0) + HARRIS_TOL) / rate);
        });
        part[t] = tm;
        __syncthreads();
        for (int s = THREADS / 2; s > 0; s >>= 1) {
            if (t < s) part[t] = fmin(part[t], part[t + s]);
            __syncthreads();
        }
        const double tmax = part[0];
        __syncthreads();
        double bt_r = 0.0, bt_s = 0.0;
        int bt_i = 0x7fffffff;
        each([&](double rate, double lm, int id) {
            if (!(rate > ptol) || fmax(lm, 0.0) / rate > tmax) return;
            if (rate > bt_r || (rate == bt_r && id < bt_i)) bt_r = rate, bt_s = fmax(lm, 0.0) / rate, bt_i = id;
        });
        part[t] = bt_r, part2[t] = bt_s, pidx[t] = bt_i;
        argbest(part, part2, pidx, [](double k, double, int i, double k0, double, int i0) { return k > k0 || (k == k0 && i < i0); });
        const int lid = pidx[0];
        __syncthreads();
        // ---- the swap (one thread; lists of at most 65 entries)
        if (t == 0) {
            ++S.iters;
            int st = MRBF_NS_OK;
            if (lid == 0x7fffffff) {
                st = MRBF_NS_INFEASIBLE;  // the dual is unbounded along the entering constraint
            } else {
                // leave
                int lj = -1;
                if (lid < m) {
                    int q = 0;
                    while (R[q] != lid) ++q;
                    for (; q + 1 < S.nr; ++q) R[q] = R[q + 1];
                    --S.nr, inR[lid] = 0;
                } else if (lid == m) {
                    S.fix = FIX_NONE;
                } else {
                    lj = lid - m - 1;
                    if (S.fix == FIX_DOUBLE && S.fixj == lj) {
                        pin[lj] = S.fixt, S.fix = FIX_NONE;
                    } else {
                        F[S.nf] = lj, pin[lj] = -1 - S.nf, ++S.nf;
                    }
                }
                // enter
                if (e < m) {
                    R[S.nr] = e, ++S.nr, inR[e] = 1;
                } else if (e == m) {
                    if (S.fix != FIX_NONE) st = MRBF_NS_GAVE_UP;
                    else S.fix = FIX_APIN;
                } else if (pin[ej] < 0) {
                    int q = -1 - pin[ej];
                    for (; q + 1 < S.nf; ++q) F[q] = F[q + 1], pin[F[q]] = -1 - q;
                    --S.nf, pin[ej] = et;
                    if (lj == ej) ++S.flips;
                } else if (S.fix != FIX_NONE) {
                    st = MRBF_NS_GAVE_UP;
                } else {
                    S.fix = FIX_DOUBLE, S.fixj = ej, S.fixt = et;
                }
            }
            S.status = st;
        }
        __syncthreads();
    }
    // ---- optimality needs dual feasibility too: every multiplier of an inequality member of W (pins, inequality rows, the
    // alpha-fixing member) >= -DUAL_TOL max(1, max |multiplier|) for the perturbed costs; else the vertex is not certified: GAVE_UP
    if (S.status == MRBF_NS_OK) {
        double lmin = 0.0, lmax = 0.0;
        for (int j = t; j < n; j += THREADS)
            if (pin[j] >= 0) lmin = fmin(lmin, lam[j]), lmax = fmax(lmax, fabs(lam[j]));
        if (t < S.nr && R[t] >= meq) lmin = fmin(lmin, lamr[t]), lmax = fmax(lmax, fabs(lamr[t]));
        if (t == 0 && S.fix != FIX_NONE) lmin = fmin(lmin, lamr[S.nr]), lmax = fmax(lmax, fabs(lamr[S.nr]));
        part[t] = lmin, part2[t] = lmax;
        __syncthreads();
        for (int s = THREADS / 2; s > 0; s >>= 1) {
            if (t < s) part[t] = fmin(part[t], part[t + s]), part2[t] = fmax(part2[t], part2[t + s]);
            __syncthreads();
        }
        if (t == 0 && part[0] < -DUAL_TOL * fmax(1.0, part2[0])) S.status = MRBF_NS_GAVE_UP;
        __syncthreads();
    }
    // ---- outputs: n projected into the box (clamp(x + n, lb, ub) - x), alpha = ||n||_inf of the returned n, the row multipliers
    const int status = S.status;
    double *nout = a.n_out + lp * n;
    double amx = 0.0;
    for (int j = t; j < n; j += THREADS) {
        double v = NAN;
        if (status == MRBF_NS_OK) {
            v = fmin(fmax(x[j] + nv[j], lb[j]), ub[j]) - x[j];
            amx = fmax(amx, fabs(v));
        }
        nout[j] = v;
    }
    part[t] = amx;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) part[t] = fmax(part[t], part[t + s]);
        __syncthreads();
    }
    if (t == 0) a.alpha_out[lp] = status == MRBF_NS_OK ? part[0] : INF;
    // the row multipliers of the unperturbed costs (-(M^-T e_alpha)) where they are admissible (>= 0 on inequality rows), else
    // those of the perturbed costs: either is a certificate (normal_lp_dual_bound), the first an exact one
    if (t == 0 && status == MRBF_NS_OK) {
        const int sz = S.nf + 1;
        bool ok = true;
        for (int q = 0; q < S.nr; ++q) ok = ok && (R[q] < meq || -Minv[S.nf * sz + q] >= 0.0);
        if (ok)
            for (int q = 0; q < S.nr; ++q) lamr[q] = -Minv[S.nf * sz + q];
    }
    __syncthreads();
    if (a.dual_out && t < m) {
        double y = 0.0;
        if (status == MRBF_NS_OK)
            for (int q = 0; q < S.nr; ++q)
                if (R[q] == t) y = lamr[q];
        a.dual_out[lp * m + t] = t < meq ? y : fmax(y, 0.0);  // within DUAL_TOL of >= 0 by the check above; clamped to keep the promise
    }
    if (t == 0) {
        a.status_out[lp] = status;
        if (a.iters_out) a.iters_out[2 * lp] = S.iters, a.iters_out[2 * lp + 1] = S.flips;
    }
}

// ---- the right-hand sides of the normal step (normal.hpp): one workgroup per LP row and start
__global__ __launch_bounds__(THREADS) void normal_assemble_kernel(AsmArgs a) {
    __shared__ double part[THREADS];
    const RowSrc s = a.src[blockIdx.x];
    const int t = threadIdx.x, n = a.n;
    // the start's blocks (the argument itself stays untouched: a modified copy of it would live in scratch memory)
    const int64_t p = blockIdx.y;
    const double *J = a.J + p * a.sJ, *V = a.V + p * a.sV, *x = a.x + p * a.sx;
    double *A = s.eq ? a.Aeq + p * a.meq * n : a.Ain + p * a.min * n, *b = s.eq ? a.beq + p * a.meq : a.bin + p * a.min;
    double *row = A + (size_t)s.dst * n;
    const double *src = s.kind == 1 ? a.Alin + s.val * n : J + s.jac;
    const int64_t step = s.kind == 1 ? 1 : s.stride;
    double acc = 0.0;
    for (int j = t; j < n; j += THREADS) {
        const double v = src[j * step];
        row[j] = v;
        if (s.kind == 1) acc += v * x[j];
    }
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int i = 0; i < THREADS; ++i) sum += part[i];
        b[s.dst] = s.kind == 1 ? a.blin[s.val] - sum : -V[s.val];  // b - A x  /  -m(x)
    }
}

int launch_assemble(mrbf_ctx *ctx, const AsmArgs &a, int64_t n_starts) {
    hipLaunchKernelGGL(normal_assemble_kernel, dim3((unsigned)a.rows, (unsigned)n_starts), dim3(THREADS), 0, ctx->stream, a);
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}

int launch(mrbf_ctx *ctx, int64_t n_lp, int n, int meq, int min, const double *x, const double *lb, const double *ub, int64_t bound_stride,
           const double *Aeq, const double *beq, const double *Ain, const double *bin, double *n_out, double *alpha_out, double *dual_out,
           int *status_out, int *iters_out) {
    Args a;
    a.n = n, a.meq = meq, a.min = min, a.m = meq + min;
    a.bs = bound_stride;
    a.x = x, a.lb = lb, a.ub = ub, a.Aeq = Aeq, a.beq = beq, a.Ain = Ain, a.bin = bin;
    a.n_out = n_out, a.alpha_out = alpha_out, a.dual_out = dual_out, a.status_out = status_out, a.iters_out = iters_out;
    const int64_t chunk = dcall::chunk(n_lp, (size_t)n * (6 * sizeof(double) + sizeof(int)));
    MRBF_TRY(get_buf(ctx, S_NS_WS, (size_t)chunk * n * 6, &a.ws));
    MRBF_TRY(get_buf(ctx, S_NS_OUT, (size_t)chunk * n, &a.wsi));
    const size_t shm = carve(a.m + 1).total;
    MRBF_HIP(ctx, hipFuncSetAttribute((const void *)normal_lp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    for (int64_t l0 = 0; l0 < n_lp; l0 += chunk) {
        const unsigned grid = (unsigned)std::min<int64_t>(chunk, n_lp - l0);
        hipLaunchKernelGGL(normal_lp_kernel, dim3(grid), dim3(THREADS), shm, ctx->stream, a, l0);
        MRBF_HIP(ctx, hipGetLastError());
    }
    return 0;
}

}  // namespace ns
}  // namespace mrbf

using namespace mrbf;

extern "C" int32_t mrbf_normal_direction(mrbf_ctx *ctx, int64_t n_lp, int32_t d, int32_t m_eq, int32_t m_ineq, const double *x,
                                         const double *lb, const double *ub, const double *A_eq, const double *b_eq, const double *A_ineq,
                                         const double *b_ineq, double *n_out, double *alpha_out, double *dual_out, int32_t *status_out,
                                         int32_t *iters_out) {
    if (!ctx) return -1;
    if (n_lp < 0) return fail(ctx, -2, "n_lp < 0");
    if (d < 1 || d > ns::MAXD) return fail(ctx, -3, "d = %d out of range (1..%d)", d, ns::MAXD);
    if (m_eq < 0) return fail(ctx, -4, "m_eq < 0");
    if (m_ineq < 0) return fail(ctx, -5, "m_ineq < 0");
    if ((int64_t)m_eq + m_ineq < 1 || (int64_t)m_eq + m_ineq > ns::MAXM)
        return fail(ctx, -4, "m_eq + m_ineq = %d rows (1..%d)", m_eq + m_ineq, ns::MAXM);
    if (!x) return fail(ctx, -6, "x is NULL");
    if (!lb) return fail(ctx, -7, "lb is NULL");
    if (!ub) return fail(ctx, -8, "ub is NULL");
    if (m_eq && !A_eq) return fail(ctx, -9, "A_eq is NULL");
    if (m_eq && !b_eq) return fail(ctx, -10, "b_eq is NULL");
    if (m_ineq && !A_ineq) return fail(ctx, -11, "A_ineq is NULL");
    if (m_ineq && !b_ineq) return fail(ctx, -12, "b_ineq is NULL");
    if (!n_out) return fail(ctx, -13, "n_out is NULL");
    if (!alpha_out) return fail(ctx, -14, "alpha_out is NULL");
    if (!status_out) return fail(ctx, -16, "status_out is NULL");
    if (n_lp == 0) return MRBF_OK;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    const int m = m_eq + m_ineq;
    const size_t N = (size_t)n_lp;
    const size_t in_cnt = N * (3 * (size_t)d + (size_t)m * (d + 1));
    double *arena;
    MRBF_TRY(get_buf(ctx, S_NS_IN, in_cnt, &arena));
    const double *dx, *dlb, *dub, *dAeq, *dbeq, *dAin, *dbin;
    MRBF_TRY(input_view(ctx, x, N * d, arena, &dx));
    MRBF_TRY(input_view(ctx, lb, N * d, arena, &dlb));
    MRBF_TRY(input_view(ctx, ub, N * d, arena, &dub));
    MRBF_TRY(input_view(ctx, A_eq, N * m_eq * d, arena, &dAeq));
    MRBF_TRY(input_view(ctx, b_eq, N * m_eq, arena, &dbeq));
    MRBF_TRY(input_view(ctx, A_ineq, N * m_ineq * d, arena, &dAin));
    MRBF_TRY(input_view(ctx, b_ineq, N * m_ineq, arena, &dbin));
    dcall::Outputs out;  // n, alpha, dual, status, iterations
    MRBF_TRY(out.open(ctx, S_STAGE_D, {{n_out, N * d, false}, {alpha_out, N, false}, {dual_out, N * m, false}, {status_out, N, true}, {iters_out, 2 * N, true}}));
    MRBF_TRY(ns::launch(ctx, n_lp, d, m_eq, m_ineq, dx, dlb, dub, d, dAeq, dbeq, dAin, dbin, out.at<double>(0), out.at<double>(1), out.at<double>(2), out.at<int>(3), out.at<int>(4)));
    MRBF_TRY(out.copy_back(ctx));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    return MRBF_OK;
}

extern "C" int32_t mrbf_normal_step(mrbf_ctx *ctx, const mrbf_ps_problem *prob, int32_t d, const double *x, const double *lb, const double *ub,
                                    double delta, double kappa_delta, double delta_max, int32_t variable_radius, double *n_out,
                                    double *dual_out, mrbf_normal_info *info) {
    if (!ctx) return -1;
    if (!prob) return fail(ctx, -2, "problem is NULL");
    if (!x) return fail(ctx, -3, "x is NULL");
    if (!lb) return fail(ctx, -4, "lb is NULL");
    if (!ub) return fail(ctx, -5, "ub is NULL");
    if (!n_out) return fail(ctx, -6, "n_out is NULL");
    if (!info) return fail(ctx, -8, "info is NULL");
    std::memset(info, 0, sizeof(*info));
    if (prob->n_models < 0 || (prob->n_models > 0 && (!prob->models || !prob->roles)))
        return fail(ctx, -2, "mrbf_normal_step: models need a roles table");
    if (variable_radius && !(kappa_delta > 0.0)) return fail(ctx, -2, "mrbf_normal_step: kappa_delta = %g", kappa_delta);
    // ---- the modelled constraint rows from the roles table (the objective rows are not this call's); their evaluations at x
    std::vector<descent::SlotShape> slots;
    descent::Shape shape = descent_shape(prob, prob->models, 1, slots);
    shape.d = d;
    descent::Layout lay;
    if (descent::Defect D = descent::read(shape, {false, descent::Centres::UNCHECKED}, lay)) return fail(ctx, -2, "mrbf_normal_step: %s", D.msg.c_str());
    const int n_lin = prob->n_lin_eq + prob->n_lin_ineq;
    if (mrbf_dispatch_normal(d, prob->n_models, lay.n_nl, n_lin, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_normal_step: d = %d / %d rows outside the device path (ask mrbf_dispatch_normal first)", d, lay.n_nl + n_lin);
    const descent::Offsets at = lay.offsets(1, descent::Slots::CONSTRAINED);
    const int64_t jtot = at.jtot, vtot = at.vtot;
    const int meq = lay.meq, min = lay.min, m = meq + min;
    (void)hipSetDevice(ctx->device);
    PinGuard pin(ctx);
    // ---- host inputs, packed: x, lb, ub, linear rows (eq, then ineq), their b
    dcall::PackedIn in;
    const size_t ax = in.fetch(ctx, x, d), alb = in.fetch(ctx, lb, d), aub = in.fetch(ctx, ub, d);
    const auto [aA, ab] = in.fetch_linear_rows(ctx, prob, d);
    MRBF_TRY(in.rc);
    hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
    MRBF_HIP(ctx, hipEventRecord(e0, ctx->stream));
    // device arena: inputs | Jacobians | values | LP data (A_eq, b_eq, A_ineq, b_ineq) | outputs (n, alpha, dual, 3 int words)
    const size_t lp_cnt = (size_t)m * (d + 1), out_dbl = (size_t)d + 1 + m, out_cnt = out_dbl + 2;
    double *base;
    MRBF_TRY(get_buf(ctx, S_NS_IN, in.total + jtot + vtot + lp_cnt + out_cnt, &base));
    double *dJ = base + in.total, *dV = dJ + jtot, *dAeq = dV + vtot, *dbeq = dAeq + (size_t)meq * d;
    double *dAin = dbeq + meq, *dbin = dAin + (size_t)min * d, *dout = dbin + min;
    MRBF_TRY(in.upload(ctx, base));
    const double *dx = in.dev(ax), *dlb = in.dev(alb), *dub = in.dev(aub), *dA = in.dev(aA), *db = in.dev(ab);
    // ---- values and Jacobians at x: one site per model that carries constraint rows
    for (int j = 0; j < prob->n_models; ++j)
        if (lay.has_con[j]) MRBF_TRY(eval_model(ctx, prob->models[j], 1, dx, dV + at.val[j], dJ + at.jac[j], nullptr));
    // ---- A_eq / b_eq (linear, then modelled), A_ineq / b_ineq (likewise) on the device
    ns::AsmArgs aa;
    aa.n = d, aa.rows = m, aa.meq = meq, aa.min = min;
    aa.sJ = jtot, aa.sV = vtot, aa.sx = d;
    aa.J = dJ, aa.V = dV, aa.x = dx, aa.Alin = dA, aa.blin = db;
    aa.Aeq = dAeq, aa.beq = dbeq, aa.Ain = dAin, aa.bin = dbin;
    descent::fill_sources(lay, at, false, aa.src);
    MRBF_TRY(ns::launch_assemble(ctx, aa, 1));
    int *oi = reinterpret_cast<int *>(dout + out_dbl);
    MRBF_TRY(ns::launch(ctx, 1, d, meq, min, dx, dlb, dub, 0, meq ? dAeq : nullptr, meq ? dbeq : nullptr, min ? dAin : nullptr,
                        min ? dbin : nullptr, dout, dout + d, dout + d + 1, oi, oi + 1));
    // ---- one read-back
    std::vector<double> hout(out_cnt);
    MRBF_HIP(ctx, hipMemcpyAsync(hout.data(), dout, out_cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MRBF_HIP(ctx, hipEventRecord(e1, ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pin.flush();
    MRBF_HIP(ctx, hipEventElapsedTime(&info->ms_total, e0, e1));
    dcall::read_status(hout.data() + out_dbl, &info->status, &info->iterations, &info->bound_flips);
    info->alpha = hout[d];
    // ---- compute_normal_step's radius (descent.jl:691-757): the given one, or alpha / kappa_delta up to delta_max
    bool ok = info->status == MRBF_NS_OK;
    if (ok && variable_radius) {
        info->delta = info->alpha / kappa_delta;
        ok = info->delta <= delta_max;
    } else {
        info->delta = delta;
    }
    if (!ok) {
        info->delta = -__builtin_huge_val();
        for (int j = 0; j < d; ++j) hout[j] = NAN;
    }
    MRBF_TRY(output_put(ctx, n_out, hout.data(), d));
    if (dual_out) MRBF_TRY(output_put(ctx, dual_out, hout.data() + d + 1, m));
    if (info->status == MRBF_NS_GAVE_UP) return fail(ctx, -2, "mrbf_normal_step: the normal-step LP gave up (take the reference method)");
    return MRBF_OK;
}
