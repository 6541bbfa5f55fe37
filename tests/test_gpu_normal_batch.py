"""Many-start normal step on the device (run with -m gpu): mrbf_normal_step_batch against mrbf_normal_step per start.  Bit identity is
the contract: n, x + n and the duals with np.array_equal (NaN rows compared as NaN), every record field with ==.  Shapes: d = 3 (dpad
64, odd row length), 65 (first dpad 128: the one-row evaluation does not split the centre range at n = 150), 129 (first dpad 256: it
splits at n = 278) -- the smallest at which the per-start offsets and the grouping of the evaluations can go wrong."""
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg
    from tests import test_gpu_sd_step as base          # its cached models (the chain's container) and objective functions

DIMS = [3, 65, 129]
NS = 5
RECORD_FIELDS = ("status", "iterations", "bound_flips", "alpha", "delta")
DELTAS = np.array([0.3, 0.25, 0.4, 0.35, 0.3])


def g_pair(X):
    """the two constraint functions of tests/test_gpu_normal.py's container: an inequality row and an equality row"""
    X = np.atleast_2d(X)
    return np.concatenate([X[:, :1] + 0.3 * np.sum(X ** 2, axis=1, keepdims=True) / X.shape[1] - 0.1, X[:, -1:] - 0.2], axis=1)


def g_second(X):
    X = np.atleast_2d(X)
    return (0.5 * X[:, 1 % X.shape[1]] - 0.2 * np.sum(X, axis=1) / X.shape[1] - 0.3)[:, None]


_MODELS = {}


def _fit(f, d, rng, kernel="multiquadric", n=None, **cfg):
    n = n or max(40, 2 * d + 20)
    C = rng.uniform(-2.0, 2.0, (n, d))
    return pkg.update_model(pkg.RbfConfig(kernel=kernel, polynomial_degree=1, **cfg), C, f(C))


def models(d):
    if d not in _MODELS:
        rng = np.random.default_rng(3000 + d)
        _MODELS[d] = dict(obj=_fit(lambda X: np.stack([base.f_a(X), base.f_b(X)], axis=1), d, rng), pair=_fit(g_pair, d, rng),
                          second=_fit(g_second, d, rng, "cubic"))
    return _MODELS[d]


def _lin(d):
    """one linear equality and two linear inequalities that leave the modelled rows of g_pair room: every row holds, the inequalities
    with slack, at x* = (-0.3, c, ..., c, 0.2) with mean(x*) = 0.05 -- g_pair's inequality is convex and negative there, its equality
    is x_last = 0.2 -- so the LP of every start is feasible, at d = 3 too (two equalities leave one free direction there)"""
    rng = np.random.default_rng(77 + d)
    xs = np.full(d, (0.05 * d + 0.1) / (d - 2))
    xs[0], xs[-1] = -0.3, 0.2
    A = rng.standard_normal((2, d)) / np.sqrt(d)
    return (np.ones((1, d)) / d, np.array([0.05]), A, A @ xs + np.array([0.1, 0.05]))


def container(d, name):
    """(container, linear rows)"""
    M = models(d)
    obj = [sg.RefSurrogate(M["obj"], [0, 1])]
    if name == "one_model":       # the container of test_normal_step_through_the_container: an equality and an inequality row on one model
        return sg.SurrogateContainer(objectives=obj, nl_eq_constraints=[sg.RefSurrogate(M["pair"], [1])],
                                     nl_ineq_constraints=[sg.RefSurrogate(M["pair"], [0])]), _lin(d)
    if name == "two_models":
        return sg.SurrogateContainer(objectives=obj, nl_eq_constraints=[sg.RefSurrogate(M["pair"], [1])],
                                     nl_ineq_constraints=[sg.RefSurrogate(M["pair"], [0]), sg.RefSurrogate(M["second"], [0])]), None
    assert name == "linear_only"
    return sg.SurrogateContainer(objectives=obj), _lin(d)


def _starts(d, ns=NS, seed=0):
    return np.random.default_rng(700 + 13 * d + seed).uniform(-0.8, 0.8, (ns, d))


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def singles(scs, X, deltas, lb, ub, lin, **kw):
    """mrbf_normal_step per start: (n, x + n, duals, records) the batch has to reproduce"""
    N, XN, Y, recs = [], [], [], []
    for p, sc in enumerate(scs):
        rc, n, dl, info, y = descent.normal_step_device(sg.container_plan(sc), X[p], lb, ub, float(deltas[p]), lin, want_duals=True, **kw)
        assert rc == 0 and info["status"] != _lib.NS_GAVE_UP, (p, rc, info)
        assert dl == info["delta"]
        N.append(n), XN.append(X[p] + n), Y.append(y), recs.append(info)
    return np.array(N), np.array(XN), np.array(Y), recs


def batch(scs, X, deltas, lb, ub, lin, out=None, expect_rc=0, **kw):
    plans = [sg.container_plan(sc) for sc in scs]
    rc, n, x_n, recs, ms, y = descent.normal_step_batch_device(plans, X, lb, ub, deltas, lin, out=out, want_duals=True, **kw)
    assert rc == expect_rc, rc
    if rc == 0:
        assert ms > 0
    return n, x_n, y, recs


def assert_identical(got, ref, tag=None):
    (n, x_n, y, recs), (rn, rx_n, ry, rrecs) = got, ref
    assert np.array_equal(n, rn, equal_nan=True), tag
    assert np.array_equal(x_n, rx_n, equal_nan=True), tag
    assert np.array_equal(y, ry, equal_nan=True), tag
    assert len(recs) == len(rrecs)
    for p, (a, b) in enumerate(zip(recs, rrecs)):
        for f in RECORD_FIELDS:
            assert _same(a[f], b[f]), (tag, p, f, a[f], b[f])
        assert a["reserved"] == 0


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", ["one_model", "two_models", "linear_only"])
def test_bit_identity_with_the_single_calls(d, name):
    sc, lin = container(d, name)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d)
    # fixed radius
    ref = singles([sc] * NS, X, DELTAS, lb, ub, lin)
    print("d = %d %s: status %s iterations %s" % (d, name, [r["status"] for r in ref[3]], [r["iterations"] for r in ref[3]]))
    assert any(r["status"] == _lib.NS_OK and r["iterations"] > 0 for r in ref[3])
    got = batch([sc] * NS, X, DELTAS, lb, ub, lin)
    assert_identical(got, ref, (d, name, "fixed"))
    assert [r["delta"] for r in got[3] if r["status"] == _lib.NS_OK] == [float(DELTAS[p]) for p, r in enumerate(got[3]) if r["status"] == _lib.NS_OK]
    # variable radius: delta_max between the radii the single calls return, so that one batch holds accepted and rejected starts
    kappa = 0.5
    radii = sorted(r["alpha"] / kappa for r in ref[3] if r["status"] == _lib.NS_OK)
    assert len(radii) >= 2 and radii[0] < radii[-1], radii
    mid = len(radii) // 2
    delta_max = 0.5 * (radii[mid - 1] + radii[mid])
    assert radii[mid - 1] < delta_max < radii[mid]
    kw = dict(kappa_delta=kappa, delta_max=delta_max, variable_radius=True)
    vref = singles([sc] * NS, X, DELTAS, lb, ub, lin, **kw)
    accepted = [r["status"] == _lib.NS_OK and r["delta"] == r["alpha"] / kappa for r in vref[3]]
    rejected = [r["status"] == _lib.NS_OK and r["delta"] == -np.inf for r in vref[3]]
    assert any(accepted) and any(rejected), vref[3]
    vgot = batch([sc] * NS, X, DELTAS, lb, ub, lin, **kw)
    assert_identical(vgot, vref, (d, name, "variable"))
    for p in range(NS):
        assert np.all(np.isnan(vgot[0][p])) == np.all(np.isnan(vgot[1][p])) == (not accepted[p])


@pytest.mark.parametrize("d", [9, 300])
def test_linear_rows_without_a_model(d):
    """no model at all (the default context); linear rows alone are admitted beyond d = 256"""
    rng = np.random.default_rng(23 + d)
    sc = sg.SurrogateContainer()
    assert not sg.container_plan(sc)["models"]
    lin = (None, None, rng.standard_normal((3, d)) / np.sqrt(d), np.array([-0.4, 0.2, -0.1]))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d, seed=1)
    ref = singles([sc] * NS, X, DELTAS, lb, ub, lin)
    assert all(r["status"] == _lib.NS_OK for r in ref[3])
    assert_identical(batch([sc] * NS, X, DELTAS, lb, ub, lin), ref, d)


@pytest.mark.parametrize("d", [3, 129])
def test_zero_iteration_and_iterating_starts_in_one_batch(d):
    """starts that already satisfy every row (n = 0 after zero iterations) beside starts that do not: two linear inequalities, x on
    either side of them"""
    sc, _ = container(d, "linear_only")
    rng = np.random.default_rng(41 + d)
    A = rng.standard_normal((2, d)) / np.sqrt(d)
    lin = (None, None, A, np.array([0.1, 0.2]))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    a0 = A[0] / np.linalg.norm(A[0])
    X = np.stack([np.zeros(d), 0.9 * a0, 0.01 * rng.standard_normal(d), -0.5 * a0 + 0.01 * rng.standard_normal(d), 1.2 * a0])
    ref = singles([sc] * NS, X, DELTAS, lb, ub, lin)
    its = [r["iterations"] for r in ref[3]]
    print("d = %d iterations:" % d, its)
    inside = [bool(np.all(A @ x <= lin[3])) for x in X]
    assert any(inside) and not all(inside)
    for p in range(NS):
        assert ref[3][p]["status"] == _lib.NS_OK
        assert (its[p] == 0 and not ref[0][p].any()) == inside[p], (p, its[p], inside[p])
    assert_identical(batch([sc] * NS, X, DELTAS, lb, ub, lin), ref, d)


def test_infeasible_rows():
    d = 3
    sc, _ = container(d, "one_model")
    bad = (np.zeros((0, d)), np.zeros(0), np.vstack([np.ones((1, d)), -np.ones((1, d))]), np.array([-1.0, -1.0]))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d, seed=5)
    X[0] = 0.0
    got = batch([sc] * NS, X, DELTAS, lb, ub, bad)           # return code 0 (asserted inside)
    n, x_n, y, recs = got
    assert all(r["status"] == _lib.NS_INFEASIBLE and r["delta"] == -np.inf for r in recs), recs
    assert np.all(np.isnan(n)) and np.all(np.isnan(x_n))
    assert_identical(got, singles([sc] * NS, X, DELTAS, lb, ub, bad))


def test_starts_whose_models_differ():
    """the number of centres (40 and 57) and one start's shape parameter differ: members of one model slot fall into different launch
    groups, and every start still reproduces its own single call"""
    d = 3
    rng = np.random.default_rng(91)
    mods = [_fit(g_pair, d, rng, n=n, shape_parameter=sp) for n, sp in ((40, 1.0), (57, 1.0), (40, 2.5), (57, 1.0), (40, 1.0))]
    obj = [sg.RefSurrogate(models(d)["obj"], [0, 1])]
    scs = [sg.SurrogateContainer(objectives=obj, nl_eq_constraints=[sg.RefSurrogate(m, [1])], nl_ineq_constraints=[sg.RefSurrogate(m, [0])])
           for m in mods]
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d, seed=3)
    ref = singles(scs, X, DELTAS, lb, ub, None)
    assert any(r["status"] == _lib.NS_OK and r["iterations"] > 0 for r in ref[3])
    assert_identical(batch(scs, X, DELTAS, lb, ub, None), ref)
    for m in mods:
        m.free()


@pytest.mark.parametrize("d", DIMS)
def test_position_independence(d):
    sc, lin = container(d, "two_models")
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d, seed=9)
    a = batch([sc] * NS, X, DELTAS, lb, ub, lin)
    perm = np.array([3, 0, 4, 2, 1])
    b = batch([sc] * NS, X[perm], DELTAS[perm], lb, ub, lin)
    assert_identical(b, (a[0][perm], a[1][perm], a[2][perm], [a[3][i] for i in perm]), "permutation")
    one = batch([sc], X[2:3], DELTAS[2:3], lb, ub, lin)
    assert_identical(one, (a[0][2:3], a[1][2:3], a[2][2:3], a[3][2:3]), "batch of one")


def test_device_pointers_and_allocation():
    d = 65
    sc, lin = container(d, "one_model")
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d, seed=11)
    ctx = sg.container_plan(sc)["models"][0].ctx
    a = batch([sc] * NS, X, DELTAS, lb, ub, lin)
    arena = ctx.get_option(_lib.OPT_ARENA_BYTES)
    b = batch([sc] * NS, X, DELTAS, lb, ub, lin)
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) == arena          # a second identical call allocates nothing
    assert_identical(b, a, "second call")
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    out = tuple(torch.empty((NS, d), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    c = batch([sc] * NS, dev(X), dev(DELTAS), dev(lb), dev(ub), lin, out=out)
    torch.cuda.synchronize()
    assert_identical((np.asarray(c[0].cpu()), np.asarray(c[1].cpu()), c[2], c[3]), a, "device pointers")


def test_chain_into_the_batched_descent():
    """normal_steps_many leaves x + n on the device; that tensor is the X_n of sd_iterate_batch_device.  Bit for bit the per-start chain
    compute_normal_step -> x + n -> mrbf_sd_criticality -> mrbf_sd_step."""
    d = 3
    sc = base.containers(d)["shared"]
    plan = sg.container_plan(sc)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d, seed=13)
    cfg = descent.SteepestDescentConfig()
    x_n_dev = torch.empty((NS, d), dtype=torch.float64, device="cuda")
    stats = {}
    res = descent.normal_steps_many([sc] * NS, None, X, DELTAS, lb, ub, stats=stats, x_n_out=x_n_dev)
    assert stats["path"] == "batch" and stats["rerouted"] == [] and len(stats["records"]) == NS and stats["ms_total"] > 0
    deltas = np.array([dl for _, dl in res])
    assert np.all(np.isfinite(deltas))
    rc, D, XP, MXP, recs, _ = descent.sd_iterate_batch_device([plan] * NS, cfg, X, x_n_dev, deltas, lb, ub)
    assert rc == 0
    for p in range(NS):
        n, dl = descent.compute_normal_step(sc, None, X[p], float(DELTAS[p]), lb, ub)
        assert np.array_equal(n, res[p][0]) and dl == res[p][1] == DELTAS[p]
        x_n = X[p] + n
        assert np.array_equal(x_n, np.asarray(x_n_dev[p].cpu()))
        rc, om, dd, cinfo = descent.sd_criticality_device(plan, X[p], x_n, lb, ub, cfg.normalize)
        assert rc == 0
        rc, xp, mxp, sinfo = descent.sd_step_device(plan, cfg, X[p], x_n, dl, lb, ub, om, dd)
        assert rc == 0
        assert np.array_equal(D[p], dd) and np.array_equal(XP[p], xp) and np.array_equal(MXP[p], mxp)
        assert recs[p]["omega"] == om and recs[p]["sigma"] == sinfo["sigma"] and recs[p]["loops"] == sinfo["loops"]
        assert recs[p]["step_norm"] == sinfo["step_norm"] and recs[p]["sd_status"] == cinfo["status"]


def test_refused_shape_takes_the_loop():
    d = 300
    rng = np.random.default_rng(15)
    C = rng.uniform(-2.0, 2.0, (40, d))             # the tail is not unisolvent on 40 sites: no tail, the shape is what matters here
    mod = pkg.update_model(pkg.RbfConfig(kernel="gaussian", polynomial_degree=-1), C, g_second(C))
    sc = sg.SurrogateContainer(nl_ineq_constraints=[sg.RefSurrogate(mod, [0])])
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X = _starts(d, ns=2, seed=17)
    deltas = np.full(2, 0.3)
    plans = [sg.container_plan(sc)] * 2
    rc = descent.normal_step_batch_device(plans, X, lb, ub, deltas)[0]
    assert rc == -2
    assert _lib.load().mrbf_dispatch_after(_lib.ENTRY_NORMAL_BATCH, -2) == 1
    stats = {}
    res = descent.normal_steps_many([sc] * 2, None, X, deltas, lb, ub, stats=stats)
    assert stats["path"] == "loop" and stats["rerouted"] == []
    for p, (n, dl) in enumerate(res):
        rn, rdl = descent.compute_normal_step(sc, None, X[p], 0.3, lb, ub)
        assert np.array_equal(n, rn, equal_nan=True) and dl == rdl
    mod.free()


def test_single_call_unchanged_against_the_host_lp():
    """the single call runs through the kernels that now carry a start index: mrbf_normal_step against the HiGHS LP on container values
    and Jacobians, to the tolerance tests/test_gpu_normal.py uses"""
    text = open(os.path.join(ROOT, "tests", "test_gpu_normal.py")).read()
    tol = float(re.search(r'abs\(info\["alpha"\] - ha\) <= (1e-\d+) \* max\(1\.0, ha\)', text).group(1))
    d = 12
    rng = np.random.default_rng(200 + d)
    mod = _fit(lambda X: np.stack([base.f_a(X), base.f_b(X)], axis=1), d, rng)
    con = _fit(g_pair, d, rng)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])], nl_eq_constraints=[sg.RefSurrogate(con, [1])],
                               nl_ineq_constraints=[sg.RefSurrogate(con, [0])])
    lin = (np.ones((1, d)) / d, np.array([0.05]), rng.standard_normal((2, d)) / np.sqrt(d), np.array([0.1, -0.2]))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    x = rng.uniform(-0.8, 0.8, d)
    A_eq, b_eq, A_in, b_in = descent._ns_host_rows(sc, None, x, lin)
    hn, ha, hst, _ = descent._normal_step_lp(x, lb, ub, A_eq, b_eq, A_in, b_in)
    assert hst == _lib.NS_OK
    rc, n, dl, info = descent.normal_step_device(sg.container_plan(sc), x, lb, ub, 0.25, lin)
    assert rc == 0 and info["status"] == _lib.NS_OK and dl == 0.25, (rc, info)
    assert abs(info["alpha"] - ha) <= tol * max(1.0, ha), (info["alpha"], ha)
    assert info["alpha"] == np.max(np.abs(n))
    mod.free(), con.free()
