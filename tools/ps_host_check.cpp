// Stand-alone host check of the Pascoletti-Serafini step's host part (morbit.jl_amd/csrc/ps_host.hpp): the refinement that decides
// which iterate is accepted and when a descent ends (prox_weights, Descent), the constraint violation of ps::Problem, the sizes of a
// start's state and the budgets.  Analytic functions are evaluated on the host; every case is judged by what the comments above
// prox_weights, Descent, Problem::violation and Sizes promise, not by a second copy of the code.  Build and run (no GPU, no library):
//     c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined tools/ps_host_check.cpp -o /tmp/ps_host_check && /tmp/ps_host_check
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../morbit.jl_amd/csrc/ps_host.hpp"

using namespace mrbf;

static long g_cases = 0;
static int g_failed = 0;
#define CHECK(...)                                                                                      \
    do {                                                                                                \
        if (!(__VA_ARGS__)) {                                                                           \
            if (++g_failed <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__);   \
        }                                                                                               \
    } while (0)

static const double NaN = std::numeric_limits<double>::quiet_NaN();

// ---- prox_weights
static bool on_simplex(const std::vector<double> &lam, int k) {
    double s = 0.0;
    bool ok = (int)lam.size() == k;
    for (double v : lam) ok = ok && v >= 0.0 && v <= 1.0 + 1e-15, s += v;
    return ok && std::fabs(s - 1.0) <= 1e-12;
}
static void check_prox_weights() {
    std::vector<double> lam;
    // "over the simplex": Gram matrices of pseudo-random gradients, gaps <= 0 with one zero, sigma over twelve decades
    unsigned long long s = 12345;
    auto rnd = [&]() { return (double)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 11) / 9007199254740992.0; };
    for (int k = 1; k <= 8; ++k)
        for (int rep = 0; rep < 6; ++rep)
            for (double sigma : {0.0, 1e-9, 1e-3, 1.0, 1e3}) {
                const int d = 1 + rep;
                std::vector<double> G((size_t)k * d), M((size_t)k * k), gap(k);
                for (double &g : G) g = 2.0 * rnd() - 1.0;
                for (int a = 0; a < k; ++a) {
                    gap[a] = -rnd();
                    for (int b = 0; b < k; ++b) {
                        M[(size_t)a * k + b] = 0.0;
                        for (int t = 0; t < d; ++t) M[(size_t)a * k + b] += G[(size_t)a * d + t] * G[(size_t)b * d + t];
                    }
                }
                gap[rep % k] = 0.0;
                prox_weights(k, M, gap, sigma, lam);
                ++g_cases;
                CHECK(on_simplex(lam, k));
                if (k == 1) CHECK(lam[0] == 1.0);
            }
    // two orthogonal unit gradients, equal gaps, sigma large: the minimum-norm point of the hull, (1/2, 1/2).  The method stops when
    // the slope sigma (e + 2 e^2) of lam = (1/2 + e, 1/2 - e) falls below 1e-14 sigma / 2: e <= 5e-15
    const std::vector<double> I2 = {1.0, 0.0, 0.0, 1.0};
    for (double sigma : {1e3, 1e9}) {
        prox_weights(2, I2, {0.0, 0.0}, sigma, lam);
        ++g_cases;
        CHECK(std::fabs(lam[0] - 0.5) <= 1e-14 && std::fabs(lam[1] - 0.5) <= 1e-14);
    }
    // "sigma -> 0: the gradient of the active objective alone": the vertex of the largest gap
    const std::vector<double> M3 = {2.0, 0.5, -0.3, 0.5, 1.0, 0.2, -0.3, 0.2, 3.0};
    for (double sigma : {0.0, 1e-300, 1e-12}) {
        prox_weights(3, M3, {-1.0, 0.0, -0.5}, sigma, lam);
        ++g_cases;
        CHECK(lam[0] == 0.0 && lam[1] == 1.0 && lam[2] == 0.0);
    }
    // an all-zero M (no gradient at all) terminates on the simplex
    for (double sigma : {0.0, 1.0, 1e12}) {
        prox_weights(3, std::vector<double>(9, 0.0), {-0.25, -0.5, 0.0}, sigma, lam);
        ++g_cases;
        CHECK(on_simplex(lam, 3));
    }
}

// ---- Descent on separable quadratics f_l(x) = sum_t w_t (x_t - c_l)^2 (one model with k outputs: nftot = k)
struct Quad {
    int d, k;
    std::vector<double> w, c;  // d weights; k centres (every coordinate of objective l has centre c[l])
    double f(int l, const double *x) const {
        double s = 0.0;
        for (int t = 0; t < d; ++t) s += w[t] * (x[t] - c[l]) * (x[t] - c[l]);
        return s;
    }
    void eval(const double *x, double *F, double *J) const {
        for (int l = 0; l < k; ++l) {
            F[l] = f(l, x);
            for (int t = 0; t < d; ++t) J[(size_t)l * d + t] = 2.0 * w[t] * (x[t] - c[l]);
        }
    }
};
static ps::Problem problem_of(int d, int k, const ps::LinRows *lin = nullptr, int nlin_ineq = 0) {
    ps::Problem P;
    P.nmodels = 1, P.nobj = k, P.nftot = k, P.d = d;
    for (int l = 0; l < k; ++l) P.obj_model[l] = 0, P.obj_col[l] = l;
    P.lin = lin, P.nlin_ineq = nlin_ineq;
    return P;
}
static double value_of(const Descent &D, const Quad &q, const double *x) {
    double v = -INFINITY;
    for (size_t i = 0; i < D.objs.size(); ++i) v = std::fmax(v, (q.f(D.objs[i], x) - D.off[i]) / D.scale[i]);
    return v;
}
// drives one descent the way ps_descend_groups does, checking the promises at every iteration; returns the iteration count
static int drive(Descent &D, const Quad &q) {
    constexpr int NSTEP = Descent::NSTEP;
    const int d = q.d, k = q.k;
    std::vector<double> F(k), J((size_t)k * d), FT((size_t)NSTEP * k), JT((size_t)NSTEP * k * d);
    D.start();
    if (D.wants_start_eval()) {
        q.eval(D.x.data(), F.data(), J.data());
        D.take_start(F.data(), J.data());
        CHECK(D.evals == 1);
    }
    int it = 0;
    while (D.trials()) {
        CHECK(!D.done);
        if (++it > 5000) break;  // "the machine ends"
        for (int u = 0; u < NSTEP; ++u) q.eval(&D.XT[(size_t)u * d], &FT[(size_t)u * k], &JT[(size_t)u * k * d]);
        const double before = D.val;
        const int evals_before = D.evals;
        D.consume(FT.data(), JT.data());
        ++g_cases;
        CHECK(D.evals == evals_before + NSTEP && D.evals == 1 + NSTEP * it && D.evals <= D.max_evals);
        CHECK(D.val <= before);
        for (int t = 0; t < d; ++t) CHECK(D.x[t] >= (*D.lb)[t] && D.x[t] <= (*D.ub)[t]);
        q.eval(D.x.data(), F.data(), J.data());
        CHECK(D.P->violation(F, D.x.data()) == 0.0);
        // val is the value at x (clamped descents: pulled a hair towards 0 and kept in [-1, 0])
        const double v = value_of(D, q, D.x.data());
        if (D.clamp)
            CHECK(D.val >= -1.0 && D.val <= 0.0 && D.val >= std::fmax(v, -1.0) && D.val <= std::fmax(v, -1.0) + 1e-12);
        else
            CHECK(D.val == v);
    }
    CHECK(it <= 5000 && D.done && !D.trials());
    return it;
}

static void check_descent_quadratics() {
    for (int k : {1, 2})
        for (int d : {1, 3, 17})
            for (bool at_bound : {false, true})
                for (int mode = 0; mode < 3; ++mode) {  // how it ends: 0 stationarity (frac < 1e-9), 1 the budget, 2 two small steps
                    Quad q{d, k, std::vector<double>(d), std::vector<double>(k)};
                    for (int t = 0; t < d; ++t) q.w[t] = 1.0 + 0.25 * (t % 5);
                    // centres inside the box [0, 1]^d, or below it: the minimiser then lies on the lower bound, where the start already is
                    for (int l = 0; l < k; ++l) q.c[l] = at_bound ? -0.2 - 0.3 * l : 0.35 + 0.3 * l;
                    const ps::Problem P = problem_of(d, k);
                    std::vector<double> lb(d, 0.0), ub(d, 1.0), x0(d);
                    for (int t = 0; t < d; ++t) x0[t] = at_bound && t % 2 == 0 ? 0.0 : 0.9 - 0.02 * t;
                    const int max_evals = mode == 1 ? 1 + 3 * Descent::NSTEP + 5 : 100000;
                    const double xtol = mode == 2 ? 0.5 : 1e-12;
                    Descent D;
                    if (k == 1) {
                        D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), q.f(0, x0.data()), max_evals, xtol);
                        CHECK(D.objs.size() == 1 && D.objs[0] == 0 && D.off[0] == 0.0 && D.scale[0] == 1.0 && !D.clamp);
                    } else {  // max of the two objectives: off = 0, scale = 1 by hand
                        D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), 0.0, max_evals, xtol);
                        D.objs = {0, 1}, D.off = {0.0, 0.0}, D.scale = {1.0, 1.0};
                        D.val = value_of(D, q, x0.data());
                    }
                    const double start_val = D.val;
                    const int it = drive(D, q);
                    if (!(at_bound && d == 1)) CHECK(D.val < start_val);  // (d = 1 at its bound starts at the minimiser: nothing is accepted)
                    else CHECK(D.val == start_val && D.x == x0);
                    if (mode == 0) CHECK(D.frac < 1e-9 || D.nsmall >= 2);
                    if (mode == 1) CHECK(it == 3 && D.evals == 1 + 3 * Descent::NSTEP);
                    if (mode == 2) CHECK(D.nsmall >= 2 || D.frac < 1e-9);
                    if (mode == 0 && k == 1)  // the minimiser of one separable quadratic over the box: the centre, projected
                        for (int t = 0; t < d; ++t) CHECK(std::fabs(D.x[t] - std::fmin(std::fmax(q.c[0], 0.0), 1.0)) <= 1e-6);
                }
    // a linear row x_0 + x_1 <= 0.9 that the unconstrained minimiser (0.7, 0.7, ..) violates: every accepted iterate stays feasible
    for (int d : {3, 17}) {
        Quad q{d, 1, std::vector<double>(d, 1.0), {0.7}};
        ps::LinRows lin;
        lin.A_ineq.assign(d, 0.0), lin.A_ineq[0] = lin.A_ineq[1] = 1.0, lin.b_ineq = {0.9};
        const ps::Problem P = problem_of(d, 1, &lin, 1);
        std::vector<double> lb(d, 0.0), ub(d, 1.0), x0(d, 0.2);
        Descent D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), q.f(0, x0.data()), 100000, 1e-12);
        drive(D, q);
        CHECK(D.x[0] + D.x[1] <= 0.9 && D.x[0] + D.x[1] > 0.8 && D.val < q.f(0, x0.data()));
    }
}

static void check_descent_cases() {
    // "the value is tau, kept in [-1, 0]": the polish with a direction r so short that tau = -1 is reached; the descent ends there
    for (int d : {1, 3, 17}) {
        Quad q{d, 2, std::vector<double>(d, 1.0), {0.4, 0.6}};
        const ps::Problem P = problem_of(d, 2);
        std::vector<double> lb(d, 0.0), ub(d, 1.0), x0(d, 0.95);
        const std::vector<double> mx = {q.f(0, x0.data()), q.f(1, x0.data())}, r = {0.05 * mx[0], 0.05 * mx[1]};
        Descent D = descent_of_ps(&P, &lb, &ub, 0.0, x0, mx, r, 100000, 1e-12);
        CHECK(D.clamp && D.objs.size() == 2 && D.off == mx && D.scale == r && D.val == 0.0 && D.x == x0);
        drive(D, q);
        CHECK(D.val == -1.0 && D.done);
    }
    // a zero gradient ends at once: one evaluation, no trial points
    {
        Quad q{3, 1, {1.0, 2.0, 3.0}, {0.5}};
        const ps::Problem P = problem_of(3, 1);
        std::vector<double> lb(3, 0.0), ub(3, 1.0), x0(3, 0.5);
        Descent D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), 0.0, 1000, 1e-3);
        CHECK(drive(D, q) == 0 && D.evals == 1 && D.done && D.x == x0);
    }
    // a box of zero width is done after start(): nothing is evaluated
    {
        Quad q{3, 1, {1.0, 1.0, 1.0}, {0.5}};
        const ps::Problem P = problem_of(3, 1);
        std::vector<double> lb(3, 0.25), ub(3, 0.25), x0(3, 0.25);
        Descent D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), q.f(0, x0.data()), 1000, 1e-3);
        D.start();
        ++g_cases;
        CHECK(D.done && !D.wants_start_eval() && !D.trials() && D.evals == 0);
    }
    // a budget below one iteration (1 + NSTEP evaluations): no start evaluation is asked for, the descent ends without one
    {
        Quad q{3, 1, {1.0, 1.0, 1.0}, {0.5}};
        const ps::Problem P = problem_of(3, 1);
        std::vector<double> lb(3, 0.0), ub(3, 1.0), x0(3, 0.25);
        Descent D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), q.f(0, x0.data()), Descent::NSTEP, 1e-3);
        CHECK(drive(D, q) == 0 && D.evals == 0);
    }
    // a component at its bound whose step points outward is taken out of the direction: it stays where it is in every trial point,
    // and the others take the plain step -sigma_u g with sigma_0 = frac width / max |g|, a factor two apart
    {
        const int d = 3;
        Quad q{d, 1, {1.0, 1.0, 1.0}, {0.5}};
        const ps::Problem P = problem_of(d, 1);
        std::vector<double> lb = {0.75, 0.0, 0.0}, ub = {1.0, 1.0, 1.0}, x0 = {0.75, 0.625, 0.5625};  // g = (0.5, 0.25, 0.125): x_0 wants below its bound
        Descent D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), q.f(0, x0.data()), 1000, 1e-3);
        std::vector<double> F(1), J(d);
        D.start();
        q.eval(x0.data(), F.data(), J.data());
        D.take_start(F.data(), J.data());
        CHECK(D.trials());
        const double sigma0 = 0.25 * 1.0 / 0.5;
        for (int u = 0; u < Descent::NSTEP; ++u) {
            ++g_cases;
            CHECK(D.XT[(size_t)u * d] == 0.75);
            for (int t = 1; t < d; ++t) CHECK(D.XT[(size_t)u * d + t] == x0[t] - sigma0 * std::ldexp(1.0, -u) * J[t]);
        }
    }
    // a non-finite trial value (NaN, +inf) is skipped, not accepted: the first trial point reports one although it is the best point
    for (double bad : {NaN, (double)INFINITY}) {
        const int d = 2;
        Quad q{d, 1, {1.0, 1.0}, {0.5}};
        const ps::Problem P = problem_of(d, 1);
        std::vector<double> lb(d, 0.0), ub(d, 1.0), x0 = {0.9, 0.8};
        Descent D = descent_of_objective(&P, &lb, &ub, 0, x0.data(), q.f(0, x0.data()), 1000, 1e-3);
        std::vector<double> F(1), J(d), FT(Descent::NSTEP), JT((size_t)Descent::NSTEP * d);
        D.start();
        q.eval(x0.data(), F.data(), J.data());
        D.take_start(F.data(), J.data());
        CHECK(D.trials());
        for (int u = 0; u < Descent::NSTEP; ++u) q.eval(&D.XT[(size_t)u * d], &FT[u], &JT[(size_t)u * d]);
        int best = 1;
        for (int u = 2; u < Descent::NSTEP; ++u)
            if (FT[u] < FT[best]) best = u;
        FT[0] = bad;
        D.consume(FT.data(), JT.data());
        ++g_cases;
        CHECK(std::isfinite(D.val) && D.val == FT[best] && D.x[0] == D.XT[(size_t)best * d] && D.x[1] == D.XT[(size_t)best * d + 1]);
        // every trial value non-finite: nothing is accepted, the range shrinks by 2^-NSTEP
        Descent E = descent_of_objective(&P, &lb, &ub, 0, x0.data(), q.f(0, x0.data()), 1000, 1e-3);
        E.start();
        E.take_start(F.data(), J.data());
        CHECK(E.trials());
        std::vector<double> allbad(Descent::NSTEP, bad);
        E.consume(allbad.data(), JT.data());
        ++g_cases;
        CHECK(E.x == x0 && E.val == q.f(0, x0.data()) && E.frac == 0.25 * std::ldexp(1.0, -Descent::NSTEP) && !E.done);
    }
}

// ---- Problem::violation: "sum of squared violations of the modelled and linear constraints at x"
static void check_violation() {
    ps::LinRows lin;
    const int d = 3;
    lin.A_eq = {1.0, 1.0, 0.0}, lin.b_eq = {1.0};           // x_0 + x_1 = 1
    lin.A_ineq = {0.0, 0.0, 1.0, 1.0, 0.0, 0.0}, lin.b_ineq = {0.5, 0.25};  // x_2 <= 0.5, x_0 <= 0.25
    ps::Problem P;
    P.nmodels = 2, P.nobj = 1, P.nftot = 4, P.d = d;
    P.foff[0] = 0, P.foff[1] = 2;
    P.obj_model[0] = 1, P.obj_col[0] = 1;                    // allF[3]
    P.ncon = 2;
    P.con_model[0] = 0, P.con_col[0] = 1, P.con_eq[0] = 0;   // allF[1] <= 0
    P.con_model[1] = 1, P.con_col[1] = 0, P.con_eq[1] = 1;   // allF[2] = 0
    P.eq_tol = 1e-3;
    const double x_ok[3] = {0.25, 0.75, 0.5};
    ++g_cases;
    CHECK(P.objective({9.0, 9.0, 9.0, 7.0}, 0) == 7.0);
    CHECK(P.model_has_objective(1) && !P.model_has_objective(0));
    // modelled rows only (no linear rows counted yet: the shared vectors are not read)
    CHECK(P.violation({9.0, -3.0, 0.0, 0.0}, x_ok) == 0.0);              // slack of an inequality is not counted
    CHECK(P.violation({9.0, 2.0, 0.0, 0.0}, x_ok) == 4.0);
    CHECK(P.violation({9.0, -1.0, 5e-4, 0.0}, x_ok) == 0.0);             // inside the equality tolerance
    CHECK(P.violation({9.0, -1.0, -1e-3, 0.0}, x_ok) == 0.0);            // on it
    CHECK(P.violation({9.0, -1.0, 2e-3, 0.0}, x_ok) == 2e-3 * 2e-3);            // beyond it: the whole value squared
    CHECK(P.violation({9.0, 2.0, -0.5, 0.0}, x_ok) == 4.25);
    CHECK(P.violation({9.0, NaN, 0.0, 0.0}, x_ok) == INFINITY);          // a NaN in a modelled constraint
    CHECK(P.violation({9.0, -1.0, NaN, 0.0}, x_ok) == INFINITY);
    CHECK(P.violation({NaN, -1.0, 0.0, NaN}, x_ok) == 0.0);              // (objectives and unused outputs are not constraints)
    // linear rows, read from the vectors the call owns: two problems share them
    P.lin = &lin, P.nlin_eq = 1, P.nlin_ineq = 2;
    ps::Problem Q = P;
    const std::vector<double> F = {0.0, -1.0, 0.0, 0.0};
    const double x_eq[3] = {0.25, 0.5, 0.5}, x_in[3] = {0.25, 0.75, 1.0}, x_two[3] = {0.5, 0.5, 0.0};
    ++g_cases;
    CHECK(P.violation(F, x_ok) == 0.0 && Q.violation(F, x_ok) == 0.0);
    CHECK(P.violation(F, x_eq) == 0.0625);                               // x_0 + x_1 - 1 = -0.25
    CHECK(P.violation(F, x_in) == 0.25);                                 // x_2 - 0.5 = 0.5
    CHECK(P.violation(F, x_two) == 0.0625);                              // x_0 - 0.25 = 0.25; x_2 has slack
    lin.b_ineq[1] = 0.5;                                                 // the shared row moves: both problems see it
    CHECK(P.violation(F, x_two) == 0.0 && Q.violation(F, x_two) == 0.0);
    const double x_tol[3] = {0.25, 0.7505, 0.5};
    CHECK(P.violation(F, x_tol) == 0.0);                                 // the equality tolerance holds for linear rows too
}

// ---- Sizes, the budgets and the reserve rule, against the closed forms written out
static void check_sizes() {
    for (int d : {1, 3, 129, 356})
        for (int k : {1, 2, 8}) {
            const size_t D = (size_t)d, K = (size_t)k;
            const size_t lam_ip = 20 * (D + 1), lam_ps = 20 * (D + 2);
            const size_t per_ip = 4 * lam_ip * D + 3 * lam_ip, per_ps = 4 * lam_ps * (D + 1) + 3 * lam_ps;
            const size_t best_per = K * (D + 2) > D + 3 ? K * (D + 2) : D + 3;
            const ps::Sizes full = ps::sizes(d, k, true, true), given = ps::sizes(d, k, false, true), ideal = ps::sizes(d, k, true, false);
            ++g_cases;
            CHECK((size_t)full.lam_ip == lam_ip && (size_t)full.lam_ps == lam_ps && full.per_ip == per_ip && full.per_ps == per_ps);
            CHECK((size_t)full.rows == (K * lam_ip > lam_ps ? K * lam_ip : lam_ps) && full.state == (K * per_ip > per_ps ? K * per_ip : per_ps));
            // a direction was given: the PS run alone
            CHECK((size_t)given.rows == lam_ps && given.state == per_ps && (size_t)given.lam_ps == lam_ps && given.per_ps == per_ps);
            // the ideal-point calls: no room for the PS run
            CHECK(ideal.lam_ps == 0 && ideal.per_ps == 0 && (size_t)ideal.rows == K * lam_ip && ideal.state == K * per_ip);
            CHECK((size_t)ideal.lam_ip == lam_ip && ideal.per_ip == per_ip);
            CHECK(ideal.rows <= full.rows && ideal.state <= full.state && ideal.best_per <= full.best_per);
            CHECK(full.best_per == best_per && given.best_per == best_per && ideal.best_per == best_per);
            CHECK(full.lam_ps <= ps::MAXLAM && k + 1 <= ps::MAXRUNS);  // d <= 356: a population the ranking can hold
            CHECK(ps::default_budget(d) == 500 * (d + 1) && ps::budget(-1, d) == 500 * (d + 1) && ps::budget(0, d) == 0 && ps::budget(77, d) == 77);
        }
    ++g_cases;
    CHECK(ps::reserve(0) == 0 && ps::reserve(259) == 0 && ps::reserve(260) == 26 && ps::reserve(64500) == 6450);
    CHECK(ps::MAXLAM == 7168 && ps::MAXRUNS == 9 && ps::MAXMODELS == 8 && ps::MAXOBJ == 8 && ps::MAXCON == 32);
}

int main() {
    check_prox_weights();
    check_descent_quadratics();
    check_descent_cases();
    check_violation();
    check_sizes();
    std::printf("ps_host_check: %ld cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("ps_host_check: ok\n");
    return g_failed == 0 ? 0 : 1;
}
