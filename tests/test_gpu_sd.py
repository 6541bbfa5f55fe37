"""Steepest-descent criticality on the device (run with -m gpu): mrbf_sd_direction against the HiGHS fixture and against exact
oracles, bit identity across batch positions and runs, mrbf_sd_criticality through a container against the host pattern (device
Jacobians + the HiGHS direction LP), and a short steepest-descent loop on two parabolas."""
import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg


def _fixture():
    from tests.test_sd_direction import load_sd_fixture

    out = load_sd_fixture()
    for c in out:
        c["omega"] = -np.inf if c["omega"] is None else c["omega"]
    return out


def solve(lps):
    """one mrbf_sd_direction call for LPs of one shape; returns D, omega, duals, status, iterations"""
    c0 = lps[0]
    n, d, k, meq, mi = len(lps), c0["x"].size, c0["G"].shape[0], c0["b_eq"].size, c0["b_ineq"].size
    for c in lps:
        assert (c["x"].size, c["G"].shape[0], c["b_eq"].size, c["b_ineq"].size, c["normalize"]) == (d, k, meq, mi, c0["normalize"])
    st = lambda key: np.ascontiguousarray(np.stack([c[key] for c in lps]), dtype=np.float64)
    G = np.ascontiguousarray(np.stack([c["G"].T for c in lps]))          # mrbf_eval's jac layout: k x d column-major
    x, lb, ub = st("x"), st("lb"), st("ub")
    A_eq, b_eq, A_in, b_in = st("A_eq"), st("b_eq"), st("A_ineq"), st("b_ineq")
    m = k + meq + mi
    D, om, Y = np.empty((n, d)), np.empty(n), np.empty((n, m))
    status, iters = np.empty(n, dtype=np.int32), np.empty((n, 2), dtype=np.int32)
    ctx = _lib.default_context()
    p = _lib.as_ptr
    ctx.check(ctx.lib.mrbf_sd_direction(ctx.h, n, d, k, meq, mi, p(G), p(x), p(lb), p(ub), p(A_eq) if meq else None,
                                        p(b_eq) if meq else None, p(A_in) if mi else None, p(b_in) if mi else None,
                                        int(c0["normalize"]), p(D), p(om), p(Y), p(status), p(iters)))
    return D, om, Y, status, iters


def certificate(c, d, omega, y):
    """(row residual / scale, duality gap / scale) of a returned solution: primal rows, multiplier signs, sum_i<k w_i y_i = 1 and
    the dual value sum_j min(c_j l_j, c_j u_j) - y . b against -omega"""
    G, A_eq, b_eq, A_in, b_in = c["G"], c["A_eq"], c["b_eq"], c["A_ineq"], c["b_ineq"]
    k = G.shape[0]
    w = np.linalg.norm(G, axis=1) if c["normalize"] else np.ones(k)
    lo, hi = descent._sd_box(c["x"], c["lb"], c["ub"])
    assert np.all(d >= lo) and np.all(d <= hi)                              # exactly inside the box
    res = 0.0
    if b_eq.size:
        sc = 1.0 + np.abs(b_eq) + np.abs(A_eq).sum(axis=1)
        res = max(res, float(np.max(np.abs(A_eq @ d - b_eq) / sc)))
    if b_in.size:
        sc = 1.0 + np.abs(b_in) + np.abs(A_in).sum(axis=1)
        res = max(res, float(np.max(np.maximum(A_in @ d - b_in, 0.0) / sc)))
    y_obj, y_eq, y_in = y[:k], y[k:k + b_eq.size], y[k + b_eq.size:]
    ysc = 1.0 + np.abs(y).max()
    assert np.all(y_obj >= -1e-12 * ysc) and np.all(y_in >= -1e-12 * ysc), y
    assert abs(float(y_obj @ w) - 1.0) <= 1e-12 * (1.0 + np.abs(y_obj) @ w), (y_obj @ w)
    cc = y_obj @ G + y_eq @ A_eq + y_in @ A_in
    dual = float(np.sum(np.minimum(cc * lo, cc * hi)) - y_eq @ b_eq - y_in @ b_in)
    scale = 1.0 + float(np.abs(cc).sum() + np.abs(y_eq) @ np.abs(b_eq) + np.abs(y_in) @ np.abs(b_in)) + abs(omega)
    return res, abs(dual + omega) / scale


def _groups(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c["x"].size, c["G"].shape[0], c["b_eq"].size, c["b_ineq"].size, c["normalize"]), []).append(c)
    return groups.values()


def test_fixture_against_highs():
    cases = _fixture()
    assert len(cases) >= 200
    worst_res = worst_gap = worst_om = 0.0
    for grp in _groups(cases):
        D, om, Y, status, iters = solve(grp)
        for i, c in enumerate(grp):
            tag = (c["idx"], c["tag"], c["x"].size, c["G"].shape[0])
            assert status[i] == c["status"], (tag, status[i], c["status"])
            if c["status"] != _lib.SD_OK:
                assert om[i] == -np.inf and not D[i].any(), tag
                continue
            res, gap = certificate(c, D[i], om[i], Y[i])
            assert res <= 1e-12 and gap <= 1e-12, (tag, res, gap)
            assert abs(om[i] - c["omega"]) <= 1e-9 * max(1.0, abs(c["omega"])), (tag, om[i], c["omega"])
            # omega is recomputed from the returned d in a fixed order
            w = np.linalg.norm(c["G"], axis=1) if c["normalize"] else np.ones(c["G"].shape[0])
            assert abs(om[i] - descent._sd_omega(c["G"], w, D[i])) <= 1e-14 * max(1.0, abs(om[i])), tag
            assert 0 <= iters[i, 0] <= 8 * (c["x"].size + Y.shape[1])
            worst_res, worst_gap = max(worst_res, res), max(worst_gap, gap)
            worst_om = max(worst_om, abs(om[i] - c["omega"]))
    print("fixture: worst residual %.1e, gap %.1e, |omega - HiGHS| %.1e" % (worst_res, worst_gap, worst_om))


def _k2_oracle(g1, g2, lo, hi):
    """min over the box of max(g1 . d, g2 . d) = max over lam in [0, 1] of sum_j min((lam g1 + (1 - lam) g2)_j [l_j, u_j]): a concave
    piecewise-linear function of lam, maximal at an end or at a breakpoint (a coordinate whose combined gradient vanishes)"""
    den = g1 - g2
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = -g2 / den
    cand = np.concatenate([[0.0, 1.0], lam[np.isfinite(lam) & (lam > 0) & (lam < 1)]])
    C = cand[:, None] * g1[None, :] + (1 - cand[:, None]) * g2[None, :]
    return float(np.max(np.sum(np.minimum(C * lo, C * hi), axis=1)))


@pytest.mark.parametrize("d", [1, 7, 64, 300, 2048])
def test_exact_oracles(d):
    rng = np.random.default_rng(d)
    for k in (1, 2):
        for normalize in (True, False):
            cases = []
            for _ in range(6):
                lb, ub = -rng.random(d) * 2, rng.random(d) * 2
                x = lb + rng.random(d) * (ub - lb)
                G = rng.standard_normal((k, d))
                cases.append(dict(x=x, lb=lb, ub=ub, G=G, A_eq=np.zeros((0, d)), b_eq=np.zeros(0), A_ineq=np.zeros((0, d)),
                                  b_ineq=np.zeros(0), normalize=normalize))
            D, om, Y, status, _ = solve(cases)
            for i, c in enumerate(cases):
                assert status[i] == _lib.SD_OK
                lo, hi = descent._sd_box(c["x"], c["lb"], c["ub"])
                w = np.linalg.norm(c["G"], axis=1) if normalize else np.ones(k)
                gh = c["G"] / w[:, None]
                if k == 1:
                    ref = -float(np.sum(np.minimum(gh[0] * lo, gh[0] * hi)))
                else:
                    ref = -_k2_oracle(gh[0], gh[1], lo, hi)
                assert abs(om[i] - ref) <= 1e-13 * max(1.0, abs(ref)) * max(1.0, np.sqrt(d) / 8), (d, k, normalize, om[i], ref)


def test_bit_identity_across_batch_positions_and_runs():
    cases = [c for c in _fixture() if c["x"].size == 64 and c["G"].shape[0] == 3 and not c["b_eq"].size and not c["b_ineq"].size
             and c["normalize"]]
    assert len(cases) >= 3
    rng = np.random.default_rng(3)
    filler = []
    for _ in range(5):
        lb, ub = -rng.random(64), rng.random(64)
        filler.append(dict(x=(lb + ub) / 2, lb=lb, ub=ub, G=rng.standard_normal((3, 64)), A_eq=np.zeros((0, 64)), b_eq=np.zeros(0),
                           A_ineq=np.zeros((0, 64)), b_ineq=np.zeros(0), normalize=True))
    batch = solve(cases)
    shifted = solve(filler + cases[::-1])
    again = solve(cases)
    for i, c in enumerate(cases):
        alone = solve([c])
        j = len(filler) + len(cases) - 1 - i
        for a, b, s, r in zip(alone, batch, shifted, again):
            assert np.array_equal(a[0], b[i]) and np.array_equal(a[0], s[j]) and np.array_equal(a[0], r[i]), c["idx"]


def test_bit_identity_across_pointer_kinds():
    """One mrbf_sd_direction call with every array in host memory, the same call with every array a device tensor, and once more with
    d_out and status on the device, the rest in host memory and the duals and iterations NULL: every output given has the same bits."""
    import torch

    rng = np.random.default_rng(6)
    N, d, k = 3, 5, 2
    lb, ub = -rng.random((N, d)), rng.random((N, d))
    x = (lb + ub) / 2
    G = rng.standard_normal((N, k, d))
    A = rng.standard_normal((N, 2, d))                                      # one equality row, one inequality row
    lo, hi = descent._sd_box(x, lb, ub)
    d0 = lo + rng.random((N, d)) * (hi - lo)                                # a feasible direction of every LP
    b = np.einsum("nrd,nd->nr", A, d0) + np.array([0.0, 0.05])
    host = [np.ascontiguousarray(a) for a in (np.transpose(G, (0, 2, 1)), x, lb, ub, A[:, :1], b[:, :1], A[:, 1:], b[:, 1:])]
    ctx = _lib.default_context()
    p = _lib.as_ptr

    def call(kind):
        outs = [np.empty((N, d)), np.empty(N), np.empty((N, k + 2)), np.empty(N, dtype=np.int32), np.empty((N, 2), dtype=np.int32)]
        ins, bufs = host, outs
        if kind == "device":
            ins, bufs = [torch.from_numpy(a).cuda() for a in host], [torch.from_numpy(a).cuda() for a in outs]
        elif kind == "mixed":
            bufs = [torch.from_numpy(outs[0]).cuda(), outs[1], None, torch.from_numpy(outs[3]).cuda(), None]
        ctx.check(ctx.lib.mrbf_sd_direction(ctx.h, N, d, k, 1, 1, *[p(a) for a in ins], 1, *[None if o is None else p(o) for o in bufs]))
        torch.cuda.synchronize()
        return [o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in bufs]

    first = call("host")
    assert np.all(first[3] == _lib.SD_OK) and np.all(np.isfinite(first[0])) and np.all(first[4][:, 0] > 0)
    for kind in ("device", "mixed"):
        for a, o in zip(first, call(kind)):
            assert o is None or np.array_equal(a, o, equal_nan=True), kind


def two_parabolas(X):
    X = np.atleast_2d(X)
    return np.stack([np.sum((X - 1.0) ** 2, axis=1), np.sum((X + 1.0) ** 2, axis=1)], axis=1)


def _fit(f, d, n, rng, lo=-2.0, hi=2.0, kernel="multiquadric"):
    C = lo + rng.random((n, d)) * (hi - lo)
    return pkg.update_model(pkg.RbfConfig(kernel=kernel, polynomial_degree=1), C, f(C))


@pytest.mark.parametrize("d", [2, 64, 128])
def test_criticality_through_the_container(d):
    rng = np.random.default_rng(100 + d)
    mod = _fit(two_parabolas, d, max(40, 2 * d + 20), rng)
    con = _fit(lambda X: np.atleast_2d(X)[:, :1] + 0.3 * np.sum(np.atleast_2d(X) ** 2, axis=1, keepdims=True) / d - 0.1, d,
               max(40, 2 * d + 20), rng)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    cfg = descent.SteepestDescentConfig()
    worst = 0.0
    for variant in ("plain", "normal_step", "linear", "modelled"):
        sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])],
                                   nl_ineq_constraints=[sg.RefSurrogate(con, [0])] if variant == "modelled" else ())
        lin = None
        if variant == "linear":
            lin = (np.ones((1, d)) / d, np.array([0.1]), rng.standard_normal((2, d)) / np.sqrt(d), np.array([0.5, 0.3]))
        plan = sg.container_plan(sc)
        for normalize in (True, False):
            for _ in range(3):
                x_n = rng.uniform(-0.8, 0.8, d)
                x = x_n - (rng.uniform(-0.05, 0.05, d) if variant in ("normal_step", "modelled") else 0.0)
                rc, om, dd, info, y = descent.sd_criticality_device(plan, x, x_n, lb, ub, normalize, lin, want_duals=True)
                G, A_eq, b_eq, A_in, b_in = descent._sd_host_rows(sc, None, x, x_n, lin)
                hd, hom, hst = descent._steepest_descent_direction(x_n, G, lb, ub, A_eq, b_eq, A_in, b_in, normalize, want_status=True)
                assert rc == 0 and info["status"] == hst == _lib.SD_OK, (variant, rc, info, hst)
                assert abs(om - hom) <= 1e-9 * max(1.0, abs(hom)), (variant, normalize, om, hom)
                c = dict(x=x_n, lb=lb, ub=ub, G=G, A_eq=A_eq, b_eq=b_eq, A_ineq=A_in, b_ineq=b_in, normalize=normalize)
                res, gap = certificate(c, dd, om, y)
                assert res <= 1e-12 and gap <= 1e-12, (variant, res, gap)
                assert info["omega"] == om and info["ms_total"] > 0
                worst = max(worst, abs(om - hom))
                # the routed call gives the same
                cfg.normalize = normalize
                om2, d2 = descent.get_criticality_sd(cfg, sc, None, x, x_n, lb, ub, lin=lin)
                assert om2 == om and np.array_equal(d2, dd)
    print("d = %d: worst |omega - host| %.1e" % (d, worst))


def test_routing_falls_back_beyond_the_device_path():
    rng = np.random.default_rng(5)
    mod = _fit(two_parabolas, 3, 30, rng)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])])
    lin = (np.zeros((0, 3)), np.zeros(0), rng.standard_normal((63, 3)), np.full(63, 5.0))    # 2 + 63 rows: beyond 64
    stats = {}
    om, d = descent.get_criticality_sd(descent.SteepestDescentConfig(), sc, None, np.zeros(3), np.zeros(3), np.full(3, -2.0),
                                       np.full(3, 2.0), lin=lin, stats=stats)
    assert stats["path"] == "reference" and np.isfinite(om) and d.shape == (3,)


def test_short_steepest_descent_loop():
    rng = np.random.default_rng(11)
    mod = _fit(two_parabolas, 2, 80, rng, lo=-4.0, hi=4.0)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])])
    cfg = descent.SteepestDescentConfig()
    lb, ub = np.full(2, -4.0), np.full(2, 4.0)
    x, delta = np.array([2.5, -1.5]), 0.5
    omegas = []
    for _ in range(20):
        stats = {}
        om, d = descent.get_criticality_sd(cfg, sc, None, x, x, lb, ub, stats=stats)
        assert stats["path"] == "device"
        omegas.append(om)
        if om <= 1e-6:
            break
        om2, xp, mxp, step = descent.compute_descent_step_sd(cfg, sc, None, x, x, delta, lb, ub, om, d)
        assert om2 == om and step <= delta * (1 + 1e-12)
        assert np.all(mxp <= mod.eval_sites(x[None, :])[0][0])   # strict Armijo on the models: no modelled objective got worse
        x = xp
    assert abs(x[0] - x[1]) < 0.05, x
    assert omegas[-1] < 0.1 * omegas[0], omegas
