"""The steepest-descent step on the device (run with -m gpu): mrbf_sd_step against the host mirror descent.compute_descent_step_sd
(which is the specification: _sd_stepsize for sigma, _backtrack for the Armijo loop) on every container shape, every sigma branch and
every way the loop ends; bit identity across calls and between host and device pointers; a chained normal step -> criticality ->
descent step loop on device buffers; and the fallback for shapes outside the decision table."""
import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg


def f_a(X):
    return np.sum((np.atleast_2d(X) - 1.0) ** 2, axis=1)


def f_b(X):
    return np.sum((np.atleast_2d(X) + 1.0) ** 2, axis=1)


def f_c(X):
    X = np.atleast_2d(X)
    return np.sum(X ** 2, axis=1) + X[:, 0]


def g_in(X):
    X = np.atleast_2d(X)
    return X[:, 0] + 0.3 * np.sum(X ** 2, axis=1) / X.shape[1] - 0.1


def h_eq(X):
    X = np.atleast_2d(X)
    return np.sum(X, axis=1) / X.shape[1] - 0.05


def _fit(fs, d, rng, kernel="multiquadric"):
    n = max(40, 2 * d + 20)
    C = rng.uniform(-2.0, 2.0, (n, d))
    return pkg.update_model(pkg.RbfConfig(kernel=kernel, polynomial_degree=1), C, np.stack([f(C) for f in fs], axis=1))


_MODELS = {}


def models(d):
    """the fitted models of one dimension (cached: fits are the slow part)"""
    if d not in _MODELS:
        rng = np.random.default_rng(1000 + d)
        _MODELS[d] = dict(
            ab=_fit([f_a, f_b], d, rng),
            a_cubic=_fit([f_a], d, rng, "cubic"),
            b_mq=_fit([f_b], d, rng, "multiquadric"),
            c_gauss=_fit([f_c], d, rng, "gaussian"),
            mixed=_fit([f_a, g_in, f_b, h_eq, f_c], d, rng),       # objectives, an inequality, an equality and an unused row
            con=_fit([g_in], d, rng, "cubic"),
        )
    return _MODELS[d]


def containers(d):
    M = models(d)
    return {
        "in_order": sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["ab"], [0, 1])]),
        "three_models": sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["a_cubic"], [0]), sg.RefSurrogate(M["b_mq"], [0]),
                                                          sg.RefSurrogate(M["c_gauss"], [0])]),
        "out_of_order": sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["ab"], [1, 0])]),
        "shared": sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["mixed"], [2, 0])], nl_eq_constraints=[sg.RefSurrogate(M["mixed"], [3])],
                                        nl_ineq_constraints=[sg.RefSurrogate(M["mixed"], [1])]),
        "two_models_con": sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["a_cubic"], [0]), sg.RefSurrogate(M["b_mq"], [0])],
                                                nl_ineq_constraints=[sg.RefSurrogate(M["con"], [0])]),
    }


def _constraints_at_x(sc, x):
    n = x.size
    out = []
    for kind in ("nl_eq_constraints", "nl_ineq_constraints"):
        if sc.lists[kind[:-1]]:
            out += [getattr(sg, "eval_container_%s_jacobian_at_scaled_site" % kind)(sc, None, x),
                    getattr(sg, "eval_container_%s_at_scaled_site" % kind)(sc, None, x)]
        else:
            out += [np.zeros((0, n)), np.zeros(0)]
    return tuple(out)


def host_step(cfg, sc, x, x_n, delta, lb, ub, omega, d, lin=None):
    """the host mirror with its intermediate values: (sigma, branch, loops, (omega, x+, mx+, ||step||)); the result is checked
    against compute_descent_step_sd itself"""
    sigma, branch = descent._sd_stepsize(x, x_n, delta, lb, ub, d, lin, lambda: _constraints_at_x(sc, x))
    loops = 0
    if sigma > cfg.min_stepsize:
        xp, mxp, step, loops = descent._backtrack(x_n, d, sigma, omega, sc, cfg)
        res = (omega, xp, mxp, float(np.max(np.abs(step))))
    else:
        res = (0, x_n.copy(), sg.eval_container_objectives_at_scaled_site(sc, None, x_n), 0)
    ref = descent.compute_descent_step_sd(cfg, sc, None, x, x_n, delta, lb, ub, omega, d, lin)
    assert ref[0] == res[0] and ref[3] == res[3] and np.array_equal(ref[1], res[1]) and np.array_equal(ref[2], res[2])
    return sigma, branch, loops, res


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1e-300, np.maximum(np.abs(a), np.abs(b)))))


def _close(a, b, tol):
    """|a - b| <= tol max(|a|, |b|, 1) entrywise (values of the model near zero are compared on the unit scale)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.maximum(np.abs(a), np.abs(b)))))


def _armijo_margin(cfg, sc, x_n, d, sigma, omega, loops):
    """relative margin of the Armijo test at the index the loop stopped at and at the one before (ties would make the comparison
    meaningless)"""
    steps = [sigma]
    for _ in range(loops):
        steps.append(steps[-1] * cfg.armijo_const_shrink)
    mx = sg.eval_container_objectives_at_scaled_site(sc, None, x_n)
    worst = np.inf
    for i in range(max(0, loops - 1), loops + 1):
        if i >= cfg.max_loops:
            continue
        mp = sg.eval_container_objectives_at_scaled_site(sc, None, x_n + steps[i] * d)
        lhs = (mx - mp) if cfg.strict_backtracking else np.array([np.max(mx) - np.max(mp)])
        rhs = steps[i] * cfg.armijo_const_rhs * omega
        worst = min(worst, float(np.min(np.abs(lhs - rhs) / np.maximum(np.abs(lhs), 1e-300))))
    return worst


def check(cfg, sc, x, x_n, delta, lb, ub, omega, d, lin=None, branch=None, loops=None, margin=True):
    """mrbf_sd_step against the host mirror; returns the device info"""
    sigma, hbranch, hloops, (hom, hxp, hmxp, hnorm) = host_step(cfg, sc, x, x_n, delta, lb, ub, omega, d, lin)
    plan = sg.container_plan(sc)
    rc, xp, mxp, info = descent.sd_step_device(plan, cfg, x, x_n, delta, lb, ub, omega, d, lin)
    tag = (hbranch, sigma, hloops, info)
    assert rc == 0, tag
    assert info["branch_name"] == hbranch, tag
    if branch is not None:
        assert hbranch == branch, tag
    assert info["loops"] == hloops, tag
    if loops is not None:
        assert hloops == loops, tag
    if hbranch == "intersect":
        assert info["sigma"] == sigma or _rel(info["sigma"], sigma) <= 1e-13, tag
    else:
        assert np.array_equal(info["sigma"], sigma, equal_nan=True), tag
    if np.array_equal(info["sigma"], sigma, equal_nan=True):
        assert np.array_equal(xp, hxp), tag
    else:
        assert _rel(xp, hxp) <= 1e-13, tag
    assert _close(mxp, hmxp, 1e-14), tag
    assert _close(mxp, sg.eval_container_objectives_at_scaled_site(sc, None, xp), 1e-14), tag
    assert info["omega"] == hom and (info["step_norm"] == hnorm or _rel(info["step_norm"], hnorm) <= 1e-13), tag
    assert info["ms_total"] > 0
    if margin and sigma > cfg.min_stepsize:
        assert _armijo_margin(cfg, sc, x_n, d, sigma, omega, hloops) > 1e-9, tag
    # the routed call returns exactly what the host mirror returns up to sigma's rounding on "intersect"
    r = descent.compute_descent_step_sd_routed(cfg, sc, None, x, x_n, delta, lb, ub, omega, d, lin)
    assert r[0] == hom and np.array_equal(r[1], xp) and np.array_equal(r[2], mxp)
    return info


def descent_dir(sc, x_n, scale=1.0):
    """-(sum of the objective gradients), scaled to ||d||_inf = scale, and an omega that the strict Armijo test can meet"""
    G = sg.eval_container_objectives_jacobian_at_scaled_site(sc, None, x_n)
    d = -G.sum(axis=0)
    d = d / np.max(np.abs(d))
    if scale != 1.0:
        d = d * scale
    omega = 0.5 * max(1e-3, float(np.min(-(G @ d))))
    return d, omega


@pytest.mark.parametrize("d", [2, 12, 64])
@pytest.mark.parametrize("name", ["in_order", "three_models", "out_of_order", "shared", "two_models_con"])
def test_parity_with_the_host_mirror(d, name):
    sc = containers(d)[name]
    rng = np.random.default_rng(d * 7 + len(name))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    for strict in (True, False):
        cfg = descent.SteepestDescentConfig(strict_backtracking=strict)
        for _ in range(2):
            x = rng.uniform(-1.0, 1.0, d)
            dd, om = descent_dir(sc, x)
            check(cfg, sc, x, x, 0.3, lb, ub, om, dd, branch="delta")
            x_n = x + rng.uniform(-0.02, 0.02, d)
            dd, om = descent_dir(sc, x_n)
            check(cfg, sc, x, x_n, 0.3, lb, ub, om, dd, branch="delta")
            dd, om = descent_dir(sc, x_n, 0.5)
            check(cfg, sc, x, x_n, 3.0, lb, ub, om, dd, branch="one")
            dd, om = descent_dir(sc, x_n)
            check(cfg, sc, x, x_n, 3.0, lb, ub, om, dd, branch="intersect")


def test_linear_rows():
    d = 12
    sc = containers(d)["three_models"]
    rng = np.random.default_rng(4)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    cfg = descent.SteepestDescentConfig()
    x = rng.uniform(-0.5, 0.5, d)
    dd, om = descent_dir(sc, x)
    # linear inequalities: one that cuts the ray before the box, one inactive; an equality the ray meets at sigma = 0.7
    a1 = dd / np.linalg.norm(dd)
    lin = (np.zeros((0, d)), np.zeros(0), np.stack([a1, -a1]), np.array([a1 @ x + 0.5 * (a1 @ dd), 10.0]))
    info = check(cfg, sc, x, x, 3.0, lb, ub, om, dd, lin, branch="intersect")
    assert abs(info["sigma"] - 0.5) <= 1e-12
    A_eq = np.stack([a1, 2.0 * a1])                                        # two consistent equalities
    lin = (A_eq, A_eq @ (x + 0.7 * dd), np.zeros((0, d)), np.zeros(0))
    info = check(cfg, sc, x, x, 3.0, lb, ub, om, dd, lin, branch="intersect")
    assert abs(info["sigma"] - 0.7) <= 1e-12
    lin = (A_eq, np.array([a1 @ (x + 0.7 * dd), 2.0 * (a1 @ (x + 0.4 * dd))]), np.zeros((0, d)), np.zeros(0))   # inconsistent
    info = check(cfg, sc, x, x, 3.0, lb, ub, om, dd, lin, branch="intersect")
    assert info["sigma"] == 0.0 and info["omega"] == 0.0 and info["step_norm"] == 0.0 and info["loops"] == 0
    # the same rows on the "delta" branch do not matter
    check(cfg, sc, x, x, 0.3, lb, ub, om, dd, lin, branch="delta")


def test_intersect_limits():
    d = 12
    M = models(d)
    rng = np.random.default_rng(6)
    cfg = descent.SteepestDescentConfig()
    # the box: x_n close to the upper bound along the direction
    sc = containers(d)["in_order"]
    x = rng.uniform(-0.5, 0.5, d)
    dd, om = descent_dir(sc, x)
    j = int(np.argmax(np.abs(dd)))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    (ub if dd[j] > 0 else lb)[j] = x[j] + 0.25 * dd[j]
    info = check(cfg, sc, x, x, 3.0, lb, ub, om, dd, branch="intersect")
    assert abs(info["sigma"] - 0.25) <= 1e-12
    # a modelled inequality whose linearisation at x cuts the ray (g(x) < 0 there)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["ab"], [0, 1])], nl_ineq_constraints=[sg.RefSurrogate(M["con"], [0])])
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    for _ in range(20):
        x = rng.uniform(-0.6, 0.6, d)
        gx = sg.eval_container_nl_ineq_constraints_at_scaled_site(sc, None, x)[0]
        Dg = sg.eval_container_nl_ineq_constraints_jacobian_at_scaled_site(sc, None, x)[0]
        dd, om = descent_dir(sc, x)
        if gx < -0.05 and Dg @ dd > 0 and -gx / (Dg @ dd) < 1.3:
            break
    else:
        raise AssertionError("no point with an active linearised constraint")
    info = check(cfg, sc, x, x, 3.0, lb, ub, om, dd, branch="intersect")
    assert abs(info["sigma"] - (-gx / (Dg @ dd))) <= 1e-12 * max(1.0, info["sigma"])
    # a modelled equality and equality rows (consistent by construction: the linear row is met at the same sigma)
    sc = containers(d)["shared"]
    x = rng.uniform(-0.5, 0.5, d)
    dd, om = descent_dir(sc, x)
    he = sg.eval_container_nl_eq_constraints_at_scaled_site(sc, None, x)[0]
    De = sg.eval_container_nl_eq_constraints_jacobian_at_scaled_site(sc, None, x)[0]
    s_eq = -he / (De @ dd)
    A_eq = (dd / np.linalg.norm(dd))[None, :]
    lin = (A_eq, A_eq @ (x + s_eq * dd), np.zeros((0, d)), np.zeros(0))
    check(cfg, sc, x, x, 3.0, np.full(d, -50.0), np.full(d, 50.0), om, dd, lin, branch="intersect", margin=False)


def test_zero_direction_and_tiny_sigma():
    d = 12
    sc = containers(d)["three_models"]
    cfg = descent.SteepestDescentConfig()
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    x = np.linspace(-0.5, 0.5, d)
    z = np.zeros(d)
    info = check(cfg, sc, x, x, 0.0, lb, ub, 0.0, z, branch="delta", margin=False)       # 0 / 0: sigma NaN
    assert np.isnan(info["sigma"]) and info["omega"] == 0.0 and info["loops"] == 0
    dd, om = descent_dir(sc, x)
    info = check(cfg, sc, x, x, 1e-17, lb, ub, om, dd, branch="delta", margin=False)   # sigma <= min_stepsize
    assert info["omega"] == 0.0 and info["step_norm"] == 0.0


def test_loop_ends():
    d = 12
    sc = containers(d)["three_models"]
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.5, 0.5, d)
    dd, om = descent_dir(sc, x)
    # an ascent direction: the test never holds; the loop stops at min_stepsize or runs out of loops
    cfg = descent.SteepestDescentConfig(min_stepsize=1e-3)
    info = check(cfg, sc, x, x, 0.5, lb, ub, om, -dd, margin=False)
    steps, i = [0.5], 0
    while steps[-1] > 1e-3:
        steps.append(steps[-1] * cfg.armijo_const_shrink)
        i += 1
    assert info["loops"] == i < cfg.max_loops
    cfg = descent.SteepestDescentConfig(max_loops=5)
    info = check(cfg, sc, x, x, 0.5, lb, ub, om, -dd, margin=False, loops=5)
    assert info["step_norm"] == 0.5 * 0.75 ** 5 * np.max(np.abs(dd))
    cfg = descent.SteepestDescentConfig(max_loops=0)
    check(cfg, sc, x, x, 0.5, lb, ub, om, -dd, margin=False, loops=0)
    check(cfg, sc, x, x, 0.5, lb, ub, om, dd, margin=False, loops=0)
    # a demanding Armijo constant: several loops before the test holds, strict and not
    for strict in (True, False):
        cfg = descent.SteepestDescentConfig(strict_backtracking=strict, armijo_const_rhs=0.5)
        info = check(cfg, sc, x, x, 1.0, lb, ub, om * 3, dd)
        assert info["loops"] >= 1


def test_determinism_and_pointers():
    d = 64
    sc = containers(d)["shared"]
    plan = sg.container_plan(sc)
    cfg = descent.SteepestDescentConfig()
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.5, 0.5, d)
    x_n = x + rng.uniform(-0.01, 0.01, d)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    lin = (np.zeros((0, d)), np.zeros(0), rng.standard_normal((3, d)) / np.sqrt(d), np.full(3, 2.0))
    for delta in (0.3, 3.0):
        dd, om = descent_dir(sc, x_n)
        a = descent.sd_step_device(plan, cfg, x, x_n, delta, lb, ub, om, dd, lin)
        b = descent.sd_step_device(plan, cfg, x, x_n, delta, lb, ub, om, dd, lin)
        dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
        out = (torch.empty(d, dtype=torch.float64, device="cuda"), torch.empty(plan["k"], dtype=torch.float64, device="cuda"))
        torch.cuda.synchronize()
        c = descent.sd_step_device(plan, cfg, dev(x), dev(x_n), delta, dev(lb), dev(ub), om, dev(dd), lin, out=out)
        torch.cuda.synchronize()
        for r in (b, c):
            assert r[0] == 0
            assert np.array_equal(a[1], np.asarray(r[1].cpu() if hasattr(r[1], "cpu") else r[1]))
            assert np.array_equal(a[2], np.asarray(r[2].cpu() if hasattr(r[2], "cpu") else r[2]))
            for key in ("branch", "loops", "sigma", "omega", "step_norm"):
                assert a[3][key] == r[3][key], key


def _raw_device_loop(sc, lin, x0, lb, ub, delta, iters, cfg, use_device_step):
    """normal step -> criticality -> descent step, ten times; with use_device_step every array lives on the device and the step is
    mrbf_sd_step, else the arrays are host arrays and the step is compute_descent_step_sd"""
    import ctypes

    plan = sg.container_plan(sc)
    ctx = plan["models"][0].ctx
    d = x0.size
    prob, keep = descent._sd_problem(plan, lin)
    dev = (lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")) if use_device_step else (lambda v: np.array(v, dtype=np.float64))
    lbv, ubv = dev(lb), dev(ub)
    x = dev(x0)
    xs, infos = [], []
    for _ in range(iters):
        n = dev(np.zeros(d))
        ninfo = _lib.NormalInfo()
        if use_device_step:
            torch.cuda.synchronize()
        ctx.check(ctx.lib.mrbf_normal_step(ctx.h, ctypes.byref(prob), d, _lib.as_ptr(x), _lib.as_ptr(lbv), _lib.as_ptr(ubv), float(delta),
                                           1.0, float(np.inf), 0, _lib.as_ptr(n), None, ctypes.byref(ninfo)))
        assert ninfo.status == _lib.NS_OK
        x_n = x + n
        dirv = dev(np.zeros(d))
        sinfo = _lib.SdInfo()
        if use_device_step:
            torch.cuda.synchronize()
        ctx.check(ctx.lib.mrbf_sd_criticality(ctx.h, ctypes.byref(prob), _lib.as_ptr(x), _lib.as_ptr(x_n), _lib.as_ptr(lbv), _lib.as_ptr(ubv),
                                              1, _lib.as_ptr(dirv), None, ctypes.byref(sinfo)))
        om = sinfo.omega
        if use_device_step:
            xp = torch.empty(d, dtype=torch.float64, device="cuda")
            mxp = torch.empty(plan["k"], dtype=torch.float64, device="cuda")
            rc, xp, mxp, info = descent.sd_step_device(plan, cfg, x, x_n, delta, lbv, ubv, om, dirv, lin, out=(xp, mxp))
            assert rc == 0
            infos.append(info)
            x = xp
        else:
            _, xp, _, _ = descent.compute_descent_step_sd(cfg, sc, None, x, x_n, delta, lb, ub, om, dirv, lin)
            infos.append(None)
            x = np.array(xp)
        xs.append(np.asarray(x.cpu()) if use_device_step else x.copy())
    return xs, infos


@pytest.mark.parametrize("d", [8, 64])
def test_chained_loop_on_device_buffers(d):
    sc = containers(d)["two_models_con"]
    rng = np.random.default_rng(20 + d)
    lin = (np.zeros((0, d)), np.zeros(0), (rng.standard_normal(d) / np.sqrt(d))[None, :], np.array([0.8]))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    cfg = descent.SteepestDescentConfig()
    x0 = rng.uniform(-0.8, 0.8, d)
    # a trust region below 1: sigma comes from the "delta" branch, which the device reproduces bit for bit -- ten iterations agree
    dev_x, infos = _raw_device_loop(sc, lin, x0, lb, ub, 0.4, 10, cfg, True)
    host_x, _ = _raw_device_loop(sc, lin, x0, lb, ub, 0.4, 10, cfg, False)
    for it, (a, b, info) in enumerate(zip(dev_x, host_x, infos)):
        assert info["branch_name"] == "delta"
        assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b))), (d, it)
        assert np.all(a >= lb) and np.all(a <= ub), (d, it)
    # beyond 1: the "intersect" branch.  Once an iterate reaches the modelled constraint, sigma is the ratio of two cancelled
    # quantities (-m(x) / Dm(x) d with m(x) ~ 0), which the host's BLAS and the device's fixed order round differently, so the
    # two loops may part; the device loop's own invariants are checked instead: box, and the linearisation at x that sigma keeps
    dev_x, infos = _raw_device_loop(sc, lin, x0, lb, ub, 1.5, 10, cfg, True)
    x_prev = x0
    for it, (a, info) in enumerate(zip(dev_x, infos)):
        assert np.all(a >= lb) and np.all(a <= ub), (d, it)
        if info["branch_name"] == "intersect" and info["sigma"] > cfg.min_stepsize:
            g = sg.eval_container_nl_ineq_constraints_at_scaled_site(sc, None, x_prev)
            Dg = sg.eval_container_nl_ineq_constraints_jacobian_at_scaled_site(sc, None, x_prev)
            lhs = g + Dg @ (a - x_prev)
            if np.all(g <= 0):
                assert np.all(lhs <= 1e-10 * (1.0 + np.abs(g) + np.abs(Dg) @ np.abs(a - x_prev))), (d, it, lhs)
        x_prev = a


def test_fallback_outside_the_table():
    d = 4
    rng = np.random.default_rng(12)
    mod = _fit([f_a, f_b], d, rng)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])])
    plan = sg.container_plan(sc)
    cfg = descent.SteepestDescentConfig()
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    x = rng.uniform(-0.5, 0.5, d)
    dd, om = descent_dir(sc, x)
    lin = (np.zeros((0, d)), np.zeros(0), rng.standard_normal((257, d)), np.full(257, 50.0))       # 257 rows
    rc, _, _, _ = descent.sd_step_device(plan, cfg, x, x, 3.0, lb, ub, om, dd, lin)
    assert rc == -2 and _lib.load().mrbf_dispatch_after(_lib.ENTRY_SD_STEP, rc) == 1
    stats = {}
    got = descent.compute_descent_step_sd_routed(cfg, sc, None, x, x, 3.0, lb, ub, om, dd, lin, stats=stats)
    ref = descent.compute_descent_step_sd(cfg, sc, None, x, x, 3.0, lb, ub, om, dd, lin)
    assert stats["path"] == "reference"
    assert got[0] == ref[0] and got[3] == ref[3] and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    # 65 objectives
    C = rng.uniform(-2.0, 2.0, (30, 2))
    big = pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, np.stack([np.sum((C - t / 65.0) ** 2, axis=1)
                                                                                              for t in range(65)], axis=1))
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(big, list(range(65)))])
    plan = sg.container_plan(sc)
    x2 = np.array([0.3, -0.2])
    d2 = np.array([-1.0, 0.5])
    rc, _, _, _ = descent.sd_step_device(plan, cfg, x2, x2, 0.5, np.full(2, -2.0), np.full(2, 2.0), 0.1, d2)
    assert rc == -2
    stats = {}
    got = descent.compute_descent_step_sd_routed(cfg, sc, None, x2, x2, 0.5, np.full(2, -2.0), np.full(2, 2.0), 0.1, d2, stats=stats)
    ref = descent.compute_descent_step_sd(cfg, sc, None, x2, x2, 0.5, np.full(2, -2.0), np.full(2, 2.0), 0.1, d2)
    assert stats["path"] == "reference"
    assert got[0] == ref[0] and got[3] == ref[3] and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
