"""Directed search on the device (run with -m gpu): mrbf_ds_direction on seeded QPs of 36 shapes against the stored results of the
host method (tests/golden/ds_host.npz, written by tests/golden/make_ds_host.py) and against SLSQP, with the certificate of every
solution; bit identity across runs, batch positions and pointer kinds; mrbf_ds_criticality against mrbf_eval + mrbf_ds_direction;
the refusals; and one whole step (get_criticality_ds -> compute_descent_step_ds) on two parabolas and on ZDT1.

The bound on z: |z_dev - z_host|_i <= MARGIN (d + k) 2^-52 (sum_j |G_ij| + |r_i|) with MARGIN = 28.9 >= 8 x 3.603, the largest ratio of
the host method against itself with the columns of G permuted (which reorders its sums) on these same QPs -- measured by
tests/golden/make_ds_host.py at (d, k) = (7, 5); every other shape stayed below 0.3 (tests/ds_util.py: MARGIN)."""
import ctypes

import numpy as np
import pytest

from tests import ds_util
from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg


@pytest.fixture(scope="module")
def golden():
    return ds_util.load_golden()


@pytest.mark.parametrize("d,k", ds_util.GPU_SHAPES)
def test_direction_shapes(d, k, golden):
    G, r, X, lb, ub = ds_util.make_batch(d, k)
    rc, D, Z, om, mu, status, iters = descent.ds_directions_many(G, r, X, lb, ub)
    assert rc == 0
    assert np.all(status == _lib.DS_OK), status          # no GAVE_UP: the host method solves all of them
    assert np.all(iters[:, 0] <= 8 * (d + k) + 16) and np.all(iters[:, 1] <= iters[:, 0])
    key = "d%d_k%d" % (d, k)
    worst = worst_f = 0.0
    for p in range(ds_util.N_QP):
        lo, hi = descent._sd_box(X[p], lb, ub)
        ds_util.check_solution(G[p], r[p], lo, hi, D[p], Z[p], om[p], mu[p], (d, k, p))
        bound = ds_util.z_bound(G[p], r[p])
        diff = np.abs(Z[p] - golden[key + "_z"][p])
        worst = max(worst, float(np.max(diff / bound)) * ds_util.MARGIN)
        assert np.all(diff <= bound), (d, k, p, diff, bound)
        assert abs(om[p] - golden[key + "_omega"][p]) <= float(np.max(bound)), (d, k, p, om[p])
        if d <= 65 and p % 6 == 0:
            f = ds_util.value(G[p], r[p], D[p])
            _, fs = ds_util.slsqp(G[p], r[p], lo, hi)
            worst_f = max(worst_f, (f - fs) / (1 + f))
            assert f <= fs + 1e-9 * (1 + f), (d, k, p, f, fs)
    print("d = %d, k = %d: |z - z_host| <= %.2g (d + k) eps scale, f - f_SLSQP <= %.1e, iterations <= %.2f (d + k)"
          % (d, k, worst, worst_f, iters[:, 0].max() / (d + k)))


def _call(ctx, G, r, X, lb, ub, device=False, want_mult=True):
    """mrbf_ds_direction with host arrays or with device tensors for every array; returns host copies of all six outputs"""
    nq, k, n = G.shape
    host = [np.ascontiguousarray(np.transpose(G, (0, 2, 1))), np.ascontiguousarray(r), np.ascontiguousarray(X),
            np.ascontiguousarray(np.broadcast_to(lb, (nq, n))), np.ascontiguousarray(np.broadcast_to(ub, (nq, n)))]
    outs = [np.empty((nq, n)), np.empty((nq, k)), np.empty(nq), np.empty((nq, k)), np.empty(nq, dtype=np.int32), np.empty((nq, 2), dtype=np.int32)]
    if device:
        ins = [torch.from_numpy(a).cuda() for a in host]
        bufs = [torch.from_numpy(a).cuda() for a in outs]
    else:
        ins, bufs = host, outs
    p = _lib.as_ptr
    rc = ctx.lib.mrbf_ds_direction(ctx.h, nq, n, k, *[p(a) for a in ins], p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]) if want_mult else None,
                                   p(bufs[4]), p(bufs[5]))
    assert rc == 0
    if device:
        torch.cuda.synchronize()
        return [b.cpu().numpy() for b in bufs]
    return bufs


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(x[rows_a], y[rows_b], equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("d,k", [(65, 3), (7, 16), (300, 5)])
def test_bits(d, k):
    ctx = _lib.default_context()
    G, r, X, lb, ub = ds_util.make_batch(d, k)
    first = _call(ctx, G, r, X, lb, ub)
    assert _same(first, _call(ctx, G, r, X, lb, ub))                       # the same call twice
    assert _same(first, _call(ctx, G, r, X, lb, ub, device=True))          # host and device pointers
    rev = slice(None, None, -1)
    shifted = _call(ctx, G[rev], r[rev], X[rev], lb, ub)                   # QP p at position 36 - p, among other neighbours
    assert _same(first, shifted, rows_b=rev)
    for p in (0, 17, 36):                                                  # ... and alone
        alone = _call(ctx, G[p:p + 1], r[p:p + 1], X[p:p + 1], lb, ub)
        assert _same(alone, first, rows_b=slice(p, p + 1)), p
    # mult_out and iters_out may be NULL: the other outputs keep their bits
    ctx2 = _lib.default_context()
    nq = G.shape[0]
    Gl = np.ascontiguousarray(np.transpose(G, (0, 2, 1)))
    LB, UB = np.ascontiguousarray(np.broadcast_to(lb, (nq, d))), np.ascontiguousarray(np.broadcast_to(ub, (nq, d)))
    D, Z, om, st = np.empty((nq, d)), np.empty((nq, k)), np.empty(nq), np.empty(nq, dtype=np.int32)
    p_ = _lib.as_ptr
    assert ctx2.lib.mrbf_ds_direction(ctx2.h, nq, d, k, p_(Gl), p_(np.ascontiguousarray(r)), p_(np.ascontiguousarray(X)), p_(LB), p_(UB), p_(D),
                                      p_(Z), p_(om), None, p_(st), None) == 0
    assert np.array_equal(D, first[0]) and np.array_equal(Z, first[1]) and np.array_equal(om, first[2]) and np.array_equal(st, first[4])


def test_statuses_on_the_device():
    rng = np.random.default_rng(4)
    d, k = 9, 3
    G = rng.standard_normal((6, k, d))
    r = -rng.uniform(0.1, 1.0, (6, k))
    X = np.full((6, d), 0.5)
    lb, ub = np.zeros(d), np.ones(d)
    r[1, 0] = 0.0          # CRITICAL: a zero
    r[2, 2] = 0.7          # CRITICAL: a positive entry
    r[3, 1] = np.nan       # CRITICAL: a NaN
    X[4, 5] = 2.5          # INFEASIBLE: l_5 = 1.5 - ... > u_5
    X[5, 0] = -0.25        # x outside [lb, ub] by less than one: d = 0 is no start (GAVE_UP; the bindings take the host method)
    rc, D, Z, om, mu, status, iters = descent.ds_directions_many(G, r, X, lb, ub)
    assert rc == 0
    assert list(status) == [_lib.DS_OK, _lib.DS_CRITICAL, _lib.DS_CRITICAL, _lib.DS_CRITICAL, _lib.DS_INFEASIBLE, _lib.DS_GAVE_UP]
    for p in (1, 2, 3):
        assert not D[p].any() and not Z[p].any() and om[p] == 0.0 and not mu[p].any()
    assert not D[4].any() and om[4] == -np.inf
    assert np.all(np.isnan(D[5])) and np.isnan(om[5]) and np.all(np.isnan(Z[5]))
    lo, hi = descent._sd_box(X[0], lb, ub)
    ds_util.check_solution(G[0], r[0], lo, hi, D[0], Z[0], om[0], mu[0], "ok")
    # every status is the host method's
    for p in range(6):
        lo, hi = descent._sd_box(X[p], lb, ub)
        assert descent._ds_active_set(G[p], r[p], lo, hi)[4] == status[p], p


def test_refusals_write_nothing():
    ctx = _lib.default_context()
    d, k, nq = 5, 2, 3
    rng = np.random.default_rng(1)
    Gl, r, X = rng.standard_normal((nq, d, k)), -np.ones((nq, k)), np.full((nq, d), 0.5)
    LB, UB = np.zeros((nq, d)), np.ones((nq, d))
    p = _lib.as_ptr

    def call(h=ctx.h, n_qp=nq, dd=d, kk=k, G=Gl, d_out=True):
        outs = [np.full((nq, d), 7.0), np.full((nq, 17), 7.0), np.full(nq, 7.0), np.full((nq, 17), 7.0), np.full(nq, 7, dtype=np.int32),
                np.full((nq, 2), 7, dtype=np.int32)]
        rc = ctx.lib.mrbf_ds_direction(h, n_qp, dd, kk, p(G), p(r), p(X), p(LB), p(UB), p(outs[0]) if d_out else None, p(outs[1]), p(outs[2]),
                                       p(outs[3]), p(outs[4]), p(outs[5]))
        assert all(np.all(o == 7) for o in outs), rc
        return rc

    assert call(h=None) == -1
    assert call(n_qp=0) == -3 and call(n_qp=-2) == -3
    assert call(dd=0) == -4 and call(dd=4097) == -4
    assert call(kk=17) == -5 and call(kk=0) == -5
    assert call(G=None) == -6
    assert call(d_out=False) == -11
    for rc in (-3, -4, -5, -6, -11):
        assert ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DS, rc) == 0          # errors, not "take the host method"


def two_parabolas(X):
    X = np.atleast_2d(X)
    return np.stack([np.sum((X - 1.0) ** 2, axis=1), np.sum((X + 1.0) ** 2, axis=1)], axis=1)


def zdt1(X):
    X = np.atleast_2d(X)
    g = 1.0 + 9.0 / (X.shape[1] - 1) * np.sum(X[:, 1:], axis=1)
    return np.stack([X[:, 0], g * (1.0 - np.sqrt(X[:, 0] / g))], axis=1)


def _fit(f, C, kernel="cubic"):
    return pkg.update_model(pkg.RbfConfig(kernel=kernel, polynomial_degree=1), C, f(C))


def _jac(mod, x):
    """the Jacobian mrbf_eval returns at x (k x d), nothing else asked for -- what mrbf_ds_criticality evaluates"""
    return mod.eval_sites(x[None, :], want_values=False, want_jac=True)[1][0]


def test_criticality_equals_eval_plus_direction():
    rng = np.random.default_rng(21)
    d = 7
    C = rng.uniform(-2.0, 2.0, (40, d))
    both = _fit(two_parabolas, C)                                           # a fitted two-output model (d = 7, n = 40, cubic)
    one = _fit(lambda X: two_parabolas(X)[:, :1], C)
    two = _fit(lambda X: two_parabolas(X)[:, 1:] + 0.1 * np.atleast_2d(X)[:, :1], rng.uniform(-2.0, 2.0, (45, d)))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    containers = [(sg.SurrogateContainer(objectives=[sg.RefSurrogate(both, [0, 1])]), lambda x: _jac(both, x)),
                  (sg.SurrogateContainer(objectives=[sg.RefSurrogate(two, [0]), sg.RefSurrogate(one, [0])]),      # two models, out of order
                   lambda x: np.vstack([_jac(two, x), _jac(one, x)]))]
    for sc, jac in containers:
        plan = sg.container_plan(sc)
        for trial in range(4):
            x_n = rng.uniform(-1.5, 1.5, d)
            if trial >= 2:
                x_n[::2] = -2.0                                              # on the lower bound
            r = -rng.uniform(0.1, 1.0, 2) * (1.0 if trial % 2 else 30.0)
            rc, om, dd, info, mu = descent.ds_criticality_device(plan, x_n, lb, ub, r, want_mult=True)
            assert rc == 0 and info["status"] == _lib.DS_OK and info["ms_total"] > 0, (rc, info)
            G = jac(x_n)
            rc2, D, Z, om2, mu2, status, iters = descent.ds_directions_many(G[None], r[None], x_n[None], lb, ub, ctx=plan["models"][0].ctx)
            assert rc2 == 0 and status[0] == _lib.DS_OK
            assert np.array_equal(dd, D[0]) and om == om2[0] and np.array_equal(mu, mu2[0])          # bit for bit
            assert (info["iterations"], info["dropped"]) == tuple(iters[0]) and info["omega"] == om
            lo, hi = descent._sd_box(x_n, lb, ub)
            ds_util.check_solution(G, r, lo, hi, D[0], Z[0], om, mu, trial)
    # a container with a linear row: -2, the table's "take the host method" -- from the call itself and through the routing
    sc, _ = containers[0]
    plan = sg.container_plan(sc)
    lin = (np.ones((1, d)), np.zeros(1), None, None)
    prob, keep = descent._sd_problem(plan, lin)
    ctx = plan["models"][0].ctx
    x_n, r = np.linspace(-1.5, 1.5, d), -np.ones(2)                              # on the linear row, off the parabolas' Pareto set
    out, info = np.full(d, 7.0), _lib.DsInfo()
    p = _lib.as_ptr
    rc = ctx.lib.mrbf_ds_criticality(ctx.h, ctypes.byref(prob), p(x_n), p(lb), p(ub), p(r), p(out), None, ctypes.byref(info))
    assert rc == -2 and np.all(out == 7.0) and ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DS, rc) == 1
    stats = {}
    cfg = descent.DirectedSearchConfig(reference_point=[-1.0, -1.0])
    fx = two_parabolas(x_n)[0]
    om, dn = descent.get_criticality_ds(cfg, sc, None, x_n, x_n, fx, 0.5, lb, ub, lin=lin, stats=stats)
    assert stats["path"] == "reference" and stats["method"] == "slsqp" and om > 0 and abs(float(np.sum(dn))) <= 1e-8


def _whole_step(cfg, mod, f, x, delta, lb, ub, rng=None):
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])])
    s1, s2 = {}, {}
    om, dn = descent.get_criticality_ds(cfg, sc, None, x, x, f(x)[0], delta, lb, ub, stats=s1, rng=rng)
    assert s1["path"] == "device" and s1["status"] == _lib.DS_OK, s1
    assert om > 0 and abs(float(np.max(np.abs(dn))) - 1.0) <= 1e-15
    om2, xp, mxp, step = descent.compute_descent_step_ds(cfg, sc, None, x, x, delta, lb, ub, om, dn, stats=s2)
    assert s2["path"] == "device", s2
    assert om2 == om > 0
    assert np.all(xp >= lb) and np.all(xp <= ub)                                      # inside the box ...
    assert 0 < step and np.max(np.abs(xp - x)) <= delta * (1 + 1e-12)                 # ... and the trust region
    mx = mod.eval_sites(x[None, :])[0][0]
    assert np.allclose(mxp, mod.eval_sites(xp[None, :])[0][0], rtol=1e-12, atol=1e-12)
    # every model objective decreases by at least the Armijo right-hand side (descent.jl:137-139; ||d||_inf = 1, so the step's
    # norm is its size)
    assert np.all(mx - mxp >= step * cfg.armijo_const_rhs * om), (mx, mxp, step, om)
    return om, xp, s1


def test_whole_step_two_parabolas():
    rng = np.random.default_rng(11)
    mod = _fit(two_parabolas, rng.uniform(-4.0, 4.0, (80, 2)), kernel="multiquadric")
    lb, ub = np.full(2, -4.0), np.full(2, 4.0)
    x = np.array([2.5, -1.5])
    _whole_step(descent.DirectedSearchConfig(reference_point=[0.0, 0.0]), mod, two_parabolas, x, 0.5, lb, ub)
    _whole_step(descent.DirectedSearchConfig(reference_direction=[1.0, 3.0]), mod, two_parabolas, x, 0.5, lb, ub)
    # no reference given: the local ideal point (descent.jl:404-412), here with a small budget
    om, xp, stats = _whole_step(descent.DirectedSearchConfig(max_ideal_point_problem_evals=400), mod, two_parabolas, x, 0.5, lb, ub,
                                rng=np.random.default_rng(2))
    assert stats["ideal_point_evals"] > 0


def test_whole_step_zdt1():
    rng = np.random.default_rng(12)
    d = 30
    C = rng.uniform(0.0, 1.0, (200, d))
    C[:40, 1::2] = 0.0                                       # sites on the face the start lies on
    C[:, 0] = np.maximum(C[:, 0], 1e-3)
    mod = _fit(zdt1, C)
    lb, ub = np.zeros(d), np.ones(d)
    x = np.full(d, 0.5)
    x[1::2] = 0.0                                            # half the coordinates at 0
    om, xp, stats = _whole_step(descent.DirectedSearchConfig(reference_point=[0.0, 0.0]), mod, zdt1, x, 0.25, lb, ub)
    assert np.all(xp[1::2] >= 0.0)
