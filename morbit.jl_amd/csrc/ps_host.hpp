// Host part of the Pascoletti-Serafini step (ps_solver.hip), free of any device include so that tools/ps_host_check.cpp drives it on
// the CPU under the sanitizers: the limits the kernels' argument blocks are sized with, the host view of a problem, the sizes of a
// start's populations and state, the budgets, and the gradient refinement (prox_weights, Descent) that decides which iterate is
// accepted and when a descent ends.  Plain arithmetic on host vectors; the model handle stays an opaque pointer.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/mrbf.h"

namespace mrbf {

namespace ps {

constexpr int MAXLAM = 7168;   // population limit: the ranking keeps one run's records in one workgroup's LDS
constexpr int MAXRUNS = 9;     // k <= 8 ideal-point runs side by side, or the PS run
constexpr int MAXMODELS = 8;   // grouped models of one container
constexpr int MAXOBJ = 8;
constexpr int MAXCON = 32;     // modelled (nonlinear) constraint rows

// the MOP's linear constraints in scaled variables (row-major rows x d): host copies, owned once by the call and shared by its starts
struct LinRows {
    std::vector<double> A_eq, b_eq, A_ineq, b_ineq;
};

// host view of the problem (function table, constraints) shared by the driver and the polish
struct Problem {
    int nmodels = 0, nobj = 0, nftot = 0, d = 0;
    const mrbf_model *models[MAXMODELS] = {};
    int foff[MAXMODELS] = {};  // first column of model j in the concatenated function vector
    int obj_model[MAXOBJ] = {}, obj_col[MAXOBJ] = {};
    int ncon = 0, con_model[MAXCON] = {}, con_col[MAXCON] = {}, con_eq[MAXCON] = {};
    int nlin_eq = 0, nlin_ineq = 0;
    const LinRows *lin = nullptr;  // (polish, final feasibility); read only where nlin_eq + nlin_ineq > 0
    double eq_tol = 1e-8;
    double objective(const std::vector<double> &allF, int l) const { return allF[foff[obj_model[l]] + obj_col[l]]; }
    bool model_has_objective(int j) const {
        bool has = false;
        for (int l = 0; l < nobj; ++l) has = has || obj_model[l] == j;
        return has;
    }
    // sum of squared violations of the modelled and linear constraints at x (allF = all model outputs at x)
    double violation(const std::vector<double> &allF, const double *x) const {
        double phi = 0.0;
        for (int c = 0; c < ncon; ++c) {
            const double v = allF[foff[con_model[c]] + con_col[c]];
            if (con_eq[c] ? std::fabs(v) > eq_tol : v > 0.0) phi += v * v;
            if (!(v == v)) phi = INFINITY;
        }
        for (int c = 0; c < nlin_eq + nlin_ineq; ++c) {
            const bool eq = c < nlin_eq;
            const double *Ar = eq ? &lin->A_eq[(size_t)c * d] : &lin->A_ineq[(size_t)(c - nlin_eq) * d];
            double s = 0.0;
            for (int j = 0; j < d; ++j) s = std::fma(Ar[j], x[j], s);
            s -= eq ? lin->b_eq[c] : lin->b_ineq[c - nlin_eq];
            if (eq ? std::fabs(s) > eq_tol : s > 0.0) phi += s * s;
        }
        return phi;
    }
};

// ---- what a start takes, in individuals and in doubles of device memory: the k ideal-point runs (population lam_ip each, d variables)
// and the PS run (lam_ps, 1 + d variables) follow each other and share their place.  rows: the evaluation batch of the larger phase;
// per_ip / per_ps: one run's populations, step sizes (ping-pong), objective, violation and order; state: the runs of the larger
// phase; best_per: the runs' best records (k x (d + 2), or d + 3 for the PS run).  A phase that does not run takes no room:
// need_ideal = false (a direction was given), with_ps = false (the ideal-point calls).  The step's arena and the chunk sizing read
// this one function.
struct Sizes {
    int lam_ip, lam_ps, rows;
    size_t per_ip, per_ps, state, best_per;
};
inline Sizes sizes(int d, int k, bool need_ideal, bool with_ps) {
    Sizes z{};
    z.lam_ip = 20 * (d + 1);
    z.lam_ps = with_ps ? 20 * (d + 2) : 0;
    z.rows = std::max(need_ideal ? k * z.lam_ip : 0, z.lam_ps);
    z.per_ip = (size_t)4 * z.lam_ip * d + (size_t)3 * z.lam_ip;
    z.per_ps = (size_t)4 * z.lam_ps * (d + 1) + (size_t)3 * z.lam_ps;
    z.state = std::max(need_ideal ? k * z.per_ip : 0, z.per_ps);
    z.best_per = std::max((size_t)k * (d + 2), (size_t)d + 3);
    return z;
}

// ---- budgets.  The reference's defaults (descent.jl:527, :416); a negative option asks for them.
inline int default_budget(int d) { return 500 * (d + 1); }
inline int budget(int asked, int d) { return asked < 0 ? default_budget(d) : asked; }
// The evolution strategy is a global method: in d + 1 >= 25 variables it locates a basin, it does not descend into it (with the
// reference's defaults the step at d = 128 stayed at 7 % of what the subproblem allows).  A tenth of every global budget is
// therefore kept back for gradient steps from the strategy's best point -- the evaluations are counted against the same budget, so
// the call never evaluates more than the configuration allows.
inline int reserve(int budget) { return budget < 20 * 13 ? 0 : budget / 10; }

}  // namespace ps

// weights of the proximal minimax step: minimise  sigma / 2 |sum_l lam_l g_l|^2 - sum_l lam_l gap_l  over the simplex (M = G G',
// gap_l = F_l - max F <= 0), Frank-Wolfe with exact line search.  sigma -> infinity: the minimum-norm point of the hull of ALL
// gradients (the common descent direction); sigma -> 0: the gradient of the active objective alone.  In between an objective
// counts as far as a step of that length can make it active -- no fixed "nearly active" tolerance.
inline void prox_weights(int k, const std::vector<double> &M, const std::vector<double> &gap, double sigma, std::vector<double> &lam) {
    int b0 = 0;
    for (int a = 1; a < k; ++a)
        if (gap[a] > gap[b0]) b0 = a;
    lam.assign(k, 0.0);
    lam[b0] = 1.0;
    std::vector<double> Ml(k);
    for (int it = 0; it < 400; ++it) {
        double lMl = 0.0, lg = 0.0;
        for (int a = 0; a < k; ++a) {
            Ml[a] = 0.0;
            for (int b = 0; b < k; ++b) Ml[a] += M[(size_t)a * k + b] * lam[b];
            lMl += lam[a] * Ml[a];
            lg += lam[a] * gap[a];
        }
        int best = 0;
        double gbest = sigma * Ml[0] - gap[0];
        for (int a = 1; a < k; ++a) {
            const double ga = sigma * Ml[a] - gap[a];
            if (ga < gbest) {
                gbest = ga;
                best = a;
            }
        }
        const double slope = (sigma * lMl - lg) - gbest;  // -(directional derivative towards the vertex) >= 0
        if (slope <= 1e-14 * std::max(std::fabs(sigma * lMl) + std::fabs(lg), 1e-300)) break;
        const double curv = sigma * (lMl - 2.0 * Ml[best] + M[(size_t)best * k + best]);
        const double gamma = curv > 0.0 ? std::min(1.0, slope / curv) : 1.0;
        for (int a = 0; a < k; ++a) lam[a] *= (1.0 - gamma);
        lam[best] += gamma;
    }
}

// Gradient refinement of a point of the box: a proximal steepest-descent method for
//     min_x  max_{l in objs} (m_l(x) - off_l) / scale_l     subject to the problem's constraints and the box
// -- the Pascoletti-Serafini subproblem itself with objs = all objectives, off = m(x_n), scale = r (the value is tau, kept in
// [-1, 0]), one objective of the local ideal point with objs = {l}, off = 0, scale = 1.  (The reference hands a local NLopt
// algorithm for the polish, descent.jl:560-569; the paper benchmark uses :LD_MMA with 100 (d + 1) evaluations,
// examples/large_scale_benchmarks.jl:217-219.)  Per iteration one evaluation with Jacobians, then NSTEP trial points
// x - sigma_u sum_l lam_l(sigma_u) g_l for NSTEP proximity parameters a factor two apart (each with its own weights, see
// prox_weights), projected onto the box, evaluated as ONE batch; components that the step would push through an active bound are
// taken out and the weights recomputed.  The best feasible improving trial point is taken; the range of sigma follows the accepted
// steps.  It stops when the budget is used up or no step down to 1e-9 of the box improves (stationarity), NOT at the first line
// search without improvement.  Every accepted iterate is feasible.  Each iteration costs 1 + NSTEP evaluations.
// One proximal minimax descent as a state machine: `trials` writes the NSTEP trial points of the next iteration (false: the descent has
// ended), `consume` takes their values and Jacobians.  Several independent descents (the k ideal-point refinements) advance in
// lockstep through ONE evaluation per iteration (ps_descend_groups) -- a round trip per iteration for all of them instead of one each.
struct Descent {
    static constexpr int NSTEP = 12;
    const ps::Problem *P = nullptr;
    const std::vector<double> *lb = nullptr, *ub = nullptr;
    std::vector<int> objs;
    std::vector<double> off, scale;
    bool clamp = false;
    int max_evals = 0;
    double xtol_rel = 0.0;
    double val = 0.0;
    std::vector<double> x;
    // state
    int evals = 0, nsmall = 0;
    double width = 0.0, frac = 0.25;  // the largest trial step moves the fastest component by `frac` of the box
    bool have = false, done = false;  // have: allF / J hold the values and the objectives' Jacobian rows at x
    std::vector<double> allF, J, XT;

    void start() {
        const int d = P->d;
        width = 0.0;
        for (int t = 0; t < d; ++t) width = std::max(width, (*ub)[t] - (*lb)[t]);
        XT.assign((size_t)NSTEP * d, 0.0);
        done = !(width > 0.0);
    }
    bool wants_start_eval() const { return !done && !have && evals + 1 + NSTEP <= max_evals; }
    void take_start(const double *F_row, const double *J_rows) {  // values (nftot) and Jacobian rows (nobj x d) at x
        allF.assign(F_row, F_row + P->nftot);
        J.assign(J_rows, J_rows + (size_t)P->nobj * P->d);
        ++evals;
        have = true;
    }
    // the trial points of the next iteration into XT; false: ended (budget, no gradient, range exhausted)
    bool trials() {
        if (done) return false;
        if (!have || evals + NSTEP > max_evals) {
            done = true;
            return false;
        }
        const int d = P->d, k = (int)objs.size();
        std::vector<double> F(k), gap(k), dir(d), M((size_t)k * k), lam, G((size_t)k * d);
        std::vector<char> fixed(d);
        double tmax = -INFINITY, gmax = 0.0;
        for (int l = 0; l < k; ++l) {
            F[l] = (P->objective(allF, objs[l]) - off[l]) / scale[l];
            tmax = std::max(tmax, F[l]);
        }
        for (int l = 0; l < k; ++l) {
            gap[l] = F[l] - tmax;
            for (int t = 0; t < d; ++t) {
                G[(size_t)l * d + t] = J[(size_t)objs[l] * d + t] / scale[l];
                gmax = std::max(gmax, std::fabs(G[(size_t)l * d + t]));
            }
        }
        if (!(gmax > 0.0) || !(gmax < INFINITY)) {
            done = true;
            return false;
        }
        const double sigma0 = frac * width / gmax;
        for (int u = 0; u < NSTEP; ++u) {
            const double sigma = sigma0 * std::ldexp(1.0, -u);
            std::fill(fixed.begin(), fixed.end(), 0);
            for (int pass = 0; pass < 2; ++pass) {
                for (int a = 0; a < k; ++a)
                    for (int b = 0; b <= a; ++b) {
                        double sdot = 0.0;
                        for (int t = 0; t < d; ++t)
                            if (!fixed[t]) sdot += G[(size_t)a * d + t] * G[(size_t)b * d + t];
                        M[(size_t)a * k + b] = M[(size_t)b * k + a] = sdot;
                    }
                prox_weights(k, M, gap, sigma, lam);
                bool changed = false;
                for (int t = 0; t < d; ++t) {
                    double v = 0.0;
                    if (!fixed[t])
                        for (int a = 0; a < k; ++a) v -= sigma * lam[a] * G[(size_t)a * d + t];
                    dir[t] = v;
                    if (!fixed[t] && ((x[t] <= (*lb)[t] && v < 0.0) || (x[t] >= (*ub)[t] && v > 0.0))) {
                        fixed[t] = 1;
                        dir[t] = 0.0;
                        changed = true;
                    }
                }
                if (!changed) break;
            }
            for (int t = 0; t < d; ++t) XT[(size_t)u * d + t] = std::min(std::max(x[t] + dir[t], (*lb)[t]), (*ub)[t]);
        }
        return true;
    }
    // values (NSTEP x nftot) and Jacobian rows (NSTEP x nobj x d) of the trial points
    void consume(const double *allFT, const double *JT) {
        const int d = P->d, k = (int)objs.size();
        std::vector<double> row(P->nftot);
        evals += NSTEP;
        int bestj = -1;
        double bestv = val - 1e-13 * std::max(1.0, std::fabs(val));
        for (int j = 0; j < NSTEP; ++j) {
            for (int c = 0; c < P->nftot; ++c) row[c] = allFT[(size_t)j * P->nftot + c];
            double tt = -INFINITY;
            bool nan = false;  // (std::max keeps its first argument beside a NaN: the NaN would be lost)
            for (int l = 0; l < k; ++l) {
                const double v = (P->objective(row, objs[l]) - off[l]) / scale[l];
                nan = nan || !(v == v);
                tt = std::max(tt, v);
            }
            if (nan || !(tt < INFINITY)) continue;
            bool feas = P->violation(row, &XT[(size_t)j * d]) == 0.0;
            if (clamp) {
                // tau = the t this x admits, a hair towards 0 so that rounding cannot make the PS constraints fail (descent.jl:443)
                tt = std::min(std::max(tt < 0.0 ? tt * (1.0 - 1e-14) : tt, -1.0), 0.0);
                for (int l = 0; l < k; ++l) feas = feas && (P->objective(row, objs[l]) - off[l] - tt * scale[l] <= 0.0);
            }
            if (feas && tt < bestv) {
                bestv = tt;
                bestj = j;
            }
        }
        if (bestj < 0) {
            frac *= std::ldexp(1.0, -NSTEP);  // nothing down to 2^-11 of the range improved: continue below it
            if (frac < 1e-9) done = true;
            return;
        }
        bool small = true;  // NLopt's xtol_rel test (descent.jl:379, :485), on two accepted steps in a row
        for (int t = 0; t < d; ++t) {
            const double xn2 = XT[(size_t)bestj * d + t];
            small = small && std::fabs(xn2 - x[t]) <= xtol_rel * std::max(std::fabs(xn2), 1e-300);
            x[t] = xn2;
        }
        allF.assign(allFT + (size_t)bestj * P->nftot, allFT + (size_t)(bestj + 1) * P->nftot);
        J.assign(JT + (size_t)bestj * P->nobj * d, JT + (size_t)(bestj + 1) * P->nobj * d);
        val = bestv;
        frac = std::min(1.0, frac * std::ldexp(4.0, -bestj));  // the accepted step sits two levels below the top of the next range
        if (clamp && val <= -1.0) done = true;
        nsmall = small ? nsmall + 1 : 0;
        if (nsmall >= 2) done = true;
    }
};

// the descent of objective l alone from a run's best record (x: d doubles, val = m_l(x)): off = 0, scale = 1, no clamp
inline Descent descent_of_objective(const ps::Problem *P, const std::vector<double> *lb, const std::vector<double> *ub, int l, const double *x,
                                    double val, int max_evals, double xtol_rel) {
    Descent D;
    D.P = P, D.lb = lb, D.ub = ub;
    D.objs = std::vector<int>{l};
    D.off = std::vector<double>{0.0};
    D.scale = std::vector<double>{1.0};
    D.clamp = false;
    D.max_evals = max_evals;
    D.xtol_rel = xtol_rel;
    D.val = val;
    D.x.assign(x, x + P->d);
    return D;
}
// the polish of the Pascoletti-Serafini run's best point: all objectives, off = m(x_n), scale = r, val = tau kept in [-1, 0]
inline Descent descent_of_ps(const ps::Problem *P, const std::vector<double> *lb, const std::vector<double> *ub, double tau,
                             const std::vector<double> &x_trial, const std::vector<double> &mx, const std::vector<double> &r, int max_evals,
                             double xtol_rel) {
    Descent D;
    D.P = P, D.lb = lb, D.ub = ub;
    D.objs.resize(P->nobj);
    for (int l = 0; l < P->nobj; ++l) D.objs[l] = l;
    D.off = mx;
    D.scale = r;
    D.clamp = true;
    D.max_evals = max_evals;
    D.xtol_rel = xtol_rel;
    D.val = tau;
    D.x = x_trial;
    return D;
}

}  // namespace mrbf
