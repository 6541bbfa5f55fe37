"""The normal step on the device (run with -m gpu): mrbf_normal_direction against the HiGHS fixture, the closed form of one violated
row and the steepest-descent LP as an independent device solver, bit identity across batch positions and runs, mrbf_normal_step
through a container against the host pattern (device values / Jacobians + the HiGHS LP), and short constrained iterations in which
both LPs run on the device."""
import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg


def _fixture():
    from tests.test_normal_step import load_normal_fixture

    return load_normal_fixture()


def solve(lps):
    """one mrbf_normal_direction call for LPs of one shape; returns n, alpha, duals, status, iterations"""
    c0 = lps[0]
    N, d, meq, mi = len(lps), c0["x"].size, c0["b_eq"].size, c0["b_ineq"].size
    for c in lps:
        assert (c["x"].size, c["b_eq"].size, c["b_ineq"].size) == (d, meq, mi)
    st = lambda key: np.ascontiguousarray(np.stack([c[key] for c in lps]), dtype=np.float64)
    x, lb, ub, A_eq, b_eq, A_in, b_in = (st(k) for k in ("x", "lb", "ub", "A_eq", "b_eq", "A_ineq", "b_ineq"))
    m = meq + mi
    n, al, Y = np.empty((N, d)), np.empty(N), np.empty((N, m))
    status, iters = np.empty(N, dtype=np.int32), np.empty((N, 2), dtype=np.int32)
    ctx = _lib.default_context()
    p = _lib.as_ptr
    ctx.check(ctx.lib.mrbf_normal_direction(ctx.h, N, d, meq, mi, p(x), p(lb), p(ub), p(A_eq) if meq else None, p(b_eq) if meq else None,
                                            p(A_in) if mi else None, p(b_in) if mi else None, p(n), p(al), p(Y), p(status), p(iters)))
    return n, al, Y, status, iters


def row_scale(c, alpha):
    C = np.vstack([c["A_eq"], c["A_ineq"]])
    b = np.concatenate([c["b_eq"], c["b_ineq"]])
    return np.maximum(1.0, np.abs(b) + max(1.0, alpha) * np.abs(C).sum(axis=1)), C, b


def _groups(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c["x"].size, c["b_eq"].size, c["b_ineq"].size), []).append(c)
    return groups.values()


def test_fixture_against_highs():
    cases = _fixture()
    worst = dict(alpha=0.0, res=0.0, gap=0.0)
    for grp in _groups(cases):
        n, al, Y, status, iters = solve(grp)
        print("d = %d, m = %d + %d: iterations %s" % (grp[0]["d"], grp[0]["m_eq"], grp[0]["m_ineq"], iters[:, 0].tolist()))
        for i, c in enumerate(grp):
            tag = (c["idx"], c["tag"], c["d"], c["m_eq"], c["m_ineq"])
            assert status[i] == c["status"], (tag, status[i], c["status"], iters[i])
            if c["status"] != _lib.NS_OK:
                assert np.all(np.isnan(n[i])) and al[i] == np.inf, tag
                continue
            scale, C, b = row_scale(c, c["alpha"])
            sc = float(scale.max()) if scale.size else 1.0
            assert abs(al[i] - c["alpha"]) <= 1e-10 * sc, (tag, al[i], c["alpha"])
            # alpha is ||n||_inf of the returned n, which lies inside [max(l', -alpha), min(u', alpha)] exactly
            lo, hi = c["lb"] - c["x"], c["ub"] - c["x"]
            assert al[i] == np.max(np.abs(n[i]))
            assert np.all(n[i] >= np.maximum(lo, -al[i])) and np.all(n[i] <= np.minimum(hi, al[i])), tag
            r = C @ n[i] - b
            res = np.concatenate([np.abs(r[:c["m_eq"]]), np.maximum(r[c["m_eq"]:], 0.0)]) / scale
            assert res.max() <= 1e-14, (tag, res.max())
            y = Y[i]
            assert np.all(y[c["m_eq"]:] >= 0.0), (tag, y)                   # inequality multipliers
            phi = descent.normal_lp_dual_bound(y, c["x"], c["lb"], c["ub"], c["A_eq"], c["b_eq"], c["A_ineq"], c["b_ineq"])
            assert al[i] - phi <= 1e-13 * sc, (tag, al[i], phi)
            assert 0 <= iters[i, 0] <= 32 * (c["d"] + C.shape[0])
            worst["alpha"] = max(worst["alpha"], abs(al[i] - c["alpha"]) / sc)
            worst["res"] = max(worst["res"], float(res.max()))
            worst["gap"] = max(worst["gap"], (al[i] - phi) / sc)
    print("fixture: worst |alpha - HiGHS| %.1e, residual %.1e, gap %.1e (relative to the row scale)" % tuple(worst.values()))


def test_alpha_zero_takes_no_iteration():
    cases = [c for c in _fixture() if c["tag"] == "alpha0"]
    assert cases
    for c in cases:
        n, al, _, status, iters = solve([c])
        assert status[0] == _lib.NS_OK and al[0] == 0.0 and not n[0].any() and iters[0, 0] == 0


@pytest.mark.parametrize("d", [1, 5, 64, 1000, 4096])
def test_closed_form_one_row(d):
    rng = np.random.default_rng(d)
    cases = []
    for _ in range(4):
        c = rng.standard_normal(d)
        b = -0.5 - rng.random()
        x = np.zeros(d) if len(cases) % 2 == 0 else rng.random(d) - 0.5
        cases.append(dict(x=x, lb=np.full(d, -1e3), ub=np.full(d, 1e3), A_eq=np.zeros((0, d)), b_eq=np.zeros(0), A_ineq=c[None, :],
                          b_ineq=np.array([b])))
    n, al, _, status, _ = solve(cases)
    for i, c in enumerate(cases):
        ref = -c["b_ineq"][0] / np.abs(c["A_ineq"]).sum()
        # with x != 0 the returned n = (x + n) - x carries the rounding of x + n: eps |x| on top
        tol = 1e-14 * ref * max(1.0, np.sqrt(d) / 8) + np.finfo(float).eps * np.abs(c["x"]).max()
        assert status[i] == _lib.NS_OK and abs(al[i] - ref) <= tol, (d, al[i], ref)


def test_cross_check_with_the_steepest_descent_lp():
    """min alpha with -alpha <= n_j <= alpha is the direction LP with the 2d objective rows +-e_j (normalize = 0) when the box lies
    inside [-1, 1]: alpha = -omega"""
    from tests.test_gpu_sd import solve as sd_solve

    rng = np.random.default_rng(9)
    for d, m in ((1, 1), (3, 2), (8, 6), (20, 12), (28, 8)):
        cases, sd_cases = [], []
        for _ in range(4):
            lb, ub = -rng.random(d) * 0.9, rng.random(d) * 0.9
            x = np.zeros(d)
            meq = m // 3
            A = rng.standard_normal((m, d))
            n0 = lb + rng.random(d) * (ub - lb)
            b = A @ n0 + np.concatenate([np.zeros(meq), rng.random(m - meq) * 0.1])
            c = dict(x=x, lb=lb, ub=ub, A_eq=A[:meq], b_eq=b[:meq], A_ineq=A[meq:], b_ineq=b[meq:])
            cases.append(c)
            sd_cases.append(dict(c, G=np.vstack([np.eye(d), -np.eye(d)]), normalize=False))
        n, al, _, status, _ = solve(cases)
        D, om, _, sst, _ = sd_solve(sd_cases)
        for i in range(len(cases)):
            assert status[i] == _lib.NS_OK and sst[i] == _lib.SD_OK
            assert abs(al[i] + om[i]) <= 1e-13, (d, m, al[i], om[i])


def test_bit_identity_across_batch_positions_and_runs():
    cases = [c for c in _fixture() if c["d"] == 12 and c["tag"] == "mixed"]
    groups = [g for g in _groups(cases) if len(g) >= 2]
    assert groups
    rng = np.random.default_rng(4)
    for grp in groups:
        d, meq, mi = grp[0]["d"], grp[0]["m_eq"], grp[0]["m_ineq"]
        filler = []
        for _ in range(5):
            lb, ub = -rng.random(d), rng.random(d)
            filler.append(dict(x=(lb + ub) / 2, lb=lb, ub=ub, A_eq=rng.standard_normal((meq, d)), b_eq=np.zeros(meq),
                               A_ineq=rng.standard_normal((mi, d)), b_ineq=-rng.random(mi) * 0.1))
        batch = solve(grp)
        shifted = solve(filler + grp[::-1])
        again = solve(grp)
        for i, c in enumerate(grp):
            alone = solve([c])
            j = len(filler) + len(grp) - 1 - i
            for a, b, s, r in zip(alone, batch, shifted, again):
                assert np.array_equal(a[0], b[i], equal_nan=True) and np.array_equal(a[0], s[j], equal_nan=True)
                assert np.array_equal(a[0], r[i], equal_nan=True), c["idx"]


def test_bit_identity_across_pointer_kinds():
    """One mrbf_normal_direction call with every array in host memory, the same call with every array a device tensor, and once more
    with n_out and status on the device, the rest in host memory and the duals and iterations NULL: every output given has the same bits."""
    import torch

    rng = np.random.default_rng(10)
    N, d = 3, 5
    lb, ub = -rng.random((N, d)) * 0.9, rng.random((N, d)) * 0.9
    x = np.zeros((N, d))
    A = rng.standard_normal((N, 2, d))                                      # one equality row, one inequality row
    n0 = lb + rng.random((N, d)) * (ub - lb)
    b = np.einsum("nrd,nd->nr", A, n0) + np.array([0.0, 0.05])
    host = [np.ascontiguousarray(a) for a in (x, lb, ub, A[:, :1], b[:, :1], A[:, 1:], b[:, 1:])]
    ctx = _lib.default_context()
    p = _lib.as_ptr

    def call(kind):
        outs = [np.empty((N, d)), np.empty(N), np.empty((N, 2)), np.empty(N, dtype=np.int32), np.empty((N, 2), dtype=np.int32)]
        ins, bufs = host, outs
        if kind == "device":
            ins, bufs = [torch.from_numpy(a).cuda() for a in host], [torch.from_numpy(a).cuda() for a in outs]
        elif kind == "mixed":
            bufs = [torch.from_numpy(outs[0]).cuda(), outs[1], None, torch.from_numpy(outs[3]).cuda(), None]
        ctx.check(ctx.lib.mrbf_normal_direction(ctx.h, N, d, 1, 1, *[p(a) for a in ins], *[None if o is None else p(o) for o in bufs]))
        torch.cuda.synchronize()
        return [o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in bufs]

    first = call("host")
    assert np.all(first[3] == _lib.NS_OK) and np.all(first[1] > 0.0) and np.all(first[4][:, 0] > 0)
    for kind in ("device", "mixed"):
        for a, o in zip(first, call(kind)):
            assert o is None or np.array_equal(a, o, equal_nan=True), kind


def two_parabolas(X):
    X = np.atleast_2d(X)
    return np.stack([np.sum((X - 1.0) ** 2, axis=1), np.sum((X + 1.0) ** 2, axis=1)], axis=1)


def _fit(f, d, n, rng, lo=-2.0, hi=2.0):
    C = lo + rng.random((n, d)) * (hi - lo)
    return pkg.update_model(pkg.RbfConfig(kernel="multiquadric", polynomial_degree=1), C, f(C))


@pytest.mark.parametrize("d", [2, 12, 64, 128])
def test_normal_step_through_the_container(d):
    rng = np.random.default_rng(200 + d)
    npts = max(40, 2 * d + 20)
    mod = _fit(two_parabolas, d, npts, rng)
    con = _fit(lambda X: np.concatenate([np.atleast_2d(X)[:, :1] + 0.3 * np.sum(np.atleast_2d(X) ** 2, axis=1, keepdims=True) / d - 0.1,
                                         np.atleast_2d(X)[:, -1:] - 0.2], axis=1), d, npts, rng)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])], nl_eq_constraints=[sg.RefSurrogate(con, [1])],
                               nl_ineq_constraints=[sg.RefSurrogate(con, [0])])
    lin = (np.ones((1, d)) / d, np.array([0.05]), rng.standard_normal((2, d)) / np.sqrt(d), np.array([0.1, -0.2]))
    plan = sg.container_plan(sc)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    worst = 0.0
    for _ in range(3):
        x = rng.uniform(-0.8, 0.8, d)
        A_eq, b_eq, A_in, b_in = descent._ns_host_rows(sc, None, x, lin)
        hn, ha, hst, _ = descent._normal_step_lp(x, lb, ub, A_eq, b_eq, A_in, b_in)
        assert hst == _lib.NS_OK
        rc, n, dl, info, y = descent.normal_step_device(plan, x, lb, ub, 0.25, lin, want_duals=True)
        assert rc == 0 and info["status"] == _lib.NS_OK and dl == 0.25, (rc, info)
        assert abs(info["alpha"] - ha) <= 1e-10 * max(1.0, ha), (info["alpha"], ha)
        assert info["alpha"] == np.max(np.abs(n)) and info["ms_total"] > 0
        worst = max(worst, abs(info["alpha"] - ha) / max(1.0, ha))
        # variable radius: alpha / kappa_delta, infeasible above delta_max
        rc, n2, dl2, info2 = descent.normal_step_device(plan, x, lb, ub, 0.25, lin, 0.5, 10.0, True)
        assert rc == 0 and dl2 == info2["alpha"] / 0.5 and np.array_equal(n2, n)
        rc, n3, dl3, _ = descent.normal_step_device(plan, x, lb, ub, 0.25, lin, 0.5, 0.5 * info["alpha"], True)
        assert rc == 0 and dl3 == -np.inf and np.all(np.isnan(n3))
        # the routed call gives the same
        stats = {}
        n4, dl4 = descent.compute_normal_step(sc, None, x, 0.25, lb, ub, lin, stats=stats)
        assert stats["path"] == "device" and np.array_equal(n4, n) and dl4 == 0.25
    # infeasible rows: NaN / -Inf
    bad = (np.zeros((0, d)), np.zeros(0), np.vstack([np.ones((1, d)), -np.ones((1, d))]), np.array([-1.0, -1.0]))
    rc, n, dl, info = descent.normal_step_device(plan, np.zeros(d), lb, ub, 0.25, bad)
    assert rc == 0 and info["status"] == _lib.NS_INFEASIBLE and dl == -np.inf and np.all(np.isnan(n))
    print("d = %d: worst |alpha - host| %.1e" % (d, worst))


def test_linear_rows_only_step_lands_on_the_rows():
    rng = np.random.default_rng(21)
    d = 6
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(_fit(two_parabolas, d, 40, rng), [0, 1])])
    A_eq, A_in = rng.standard_normal((1, d)), rng.standard_normal((3, d))
    b_eq, b_in = np.array([0.3]), np.array([-0.2, 0.1, 0.4])
    lb, ub = np.full(d, -3.0), np.full(d, 3.0)
    x = rng.uniform(-1, 1, d)
    stats = {}
    n, dl = descent.compute_normal_step(sc, None, x, 0.5, lb, ub, (A_eq, b_eq, A_in, b_in), stats=stats)
    assert stats["path"] == "device"
    xn = x + n
    assert abs(A_eq @ xn - b_eq).max() <= 1e-13 and (A_in @ xn - b_in).max() <= 1e-13


def test_linear_rows_without_a_device_model():
    """the decision table admits linear rows only: no model in the plan (n_models = 0), the context is the default one"""
    rng = np.random.default_rng(23)
    d = 9
    sc = sg.SurrogateContainer()
    assert not sg.container_plan(sc)["models"]
    A_in, b_in = rng.standard_normal((3, d)), np.array([-0.4, 0.2, -0.1])
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    x = rng.uniform(-1, 1, d)
    stats = {}
    n, dl = descent.compute_normal_step(sc, None, x, 0.5, lb, ub, (None, None, A_in, b_in), stats=stats)
    assert stats["path"] == "device" and stats["status"] == _lib.NS_OK and dl == 0.5
    _, ha, hst, _ = descent._normal_step_lp(x, lb, ub, A_ineq=A_in, b_ineq=b_in - A_in @ x)
    assert hst == _lib.NS_OK and abs(np.max(np.abs(n)) - ha) <= 1e-10 * max(1.0, ha)
    assert (A_in @ (x + n) - b_in).max() <= 1e-13


def test_chained_constrained_iterations():
    """normal step -> steepest-descent criticality at x_n = x + n -> step, on two parabolas with the modelled inequality
    x_1 + x_2 >= 0.5 (as 0.5 - x_1 - x_2 <= 0): both LPs on the device, the constraint violation goes down"""
    rng = np.random.default_rng(31)
    mod = _fit(two_parabolas, 2, 80, rng, lo=-4.0, hi=4.0)
    con = _fit(lambda X: 0.5 - np.atleast_2d(X).sum(axis=1, keepdims=True), 2, 40, rng, lo=-4.0, hi=4.0)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])], nl_ineq_constraints=[sg.RefSurrogate(con, [0])])
    cfg = descent.SteepestDescentConfig()
    lb, ub = np.full(2, -4.0), np.full(2, 4.0)
    x, delta = np.array([-2.0, -1.5]), 0.5
    viol = [max(0.0, 0.5 - x.sum())]
    for _ in range(6):
        stats = {}
        n, dl = descent.compute_normal_step(sc, None, x, delta, lb, ub, stats=stats)
        assert stats["path"] == "device" and np.isfinite(dl)
        x_n = x + n
        st2 = {}
        om, dd = descent.get_criticality_sd(cfg, sc, None, x, x_n, lb, ub, stats=st2)
        assert st2["path"] == "device"
        if om > 1e-8:
            _, x_n, _, _ = descent.compute_descent_step_sd(cfg, sc, None, x, x_n, delta, lb, ub, om, dd)
        x = x_n
        viol.append(max(0.0, 0.5 - x.sum()))
    assert max(viol[1:]) <= 1e-6 < viol[0], viol
