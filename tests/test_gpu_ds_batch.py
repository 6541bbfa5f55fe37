"""Many-start directed search on the device (run with -m gpu): mrbf_ds_iterate_batch against mrbf_ds_criticality -> _ds_normalise ->
mrbf_sd_step chained per start on the same context.  Bit identity is the contract: every output array with np.array_equal (NaN
positions equal), every record field with ==.  Shapes: d = 2, 7 (dpad 64, even and odd row length) and 65 (first dpad 128); k = 1, 2,
3; 1, 5 and 33 starts -- the smallest at which the per-start offsets, the grouping of the evaluations and the padding of the arena's
pieces can go wrong.  The models are built from coefficients (no fit): a linear tail with slopes of order one plus small kernel terms
on 12 .. 40 centres, so every objective has a gradient of order one everywhere in the box.  The reference chain of the 33 starts of a
shape is computed once and shared."""

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import rbf_model as rm
    from morbit.jl_amd import surrogates as sg

NS_MAX = 33
RECORD_FIELDS = ("ds_status", "iterations", "dropped", "branch", "loops", "omega", "omega_step", "sigma", "step_norm", "dnorm")


def _model(d, k, n, kernel, seed, positive=False):
    """a k-output model on n centres in [0, 1]^d: tail coefficients of order one (all positive, with kernel weights too small to turn
    a sign, where `positive`), kernel weights that leave the gradient of order one"""
    rng = np.random.default_rng(seed)
    C = rng.uniform(0.0, 1.0, (n, d))
    W = rng.standard_normal((n, k)) * (1e-4 if positive else 0.05) / n
    Lp = rng.uniform(0.5, 1.5, (d + 1, k)) if positive else rng.standard_normal((d + 1, k))
    return rm.model_from_coeffs(pkg.RbfConfig(kernel=kernel, polynomial_degree=1), C, W, Lp)


_MODELS = {}


def models(d):
    if d not in _MODELS:
        _MODELS[d] = dict(m1=_model(d, 1, 12, "cubic", 10 * d + 1), m2=_model(d, 2, 24, "cubic", 10 * d + 2),
                          m3=_model(d, 3, 40, "multiquadric", 10 * d + 3), a=_model(d, 2, 30, "gaussian", 10 * d + 4),
                          b=_model(d, 2, 17, "multiquadric", 10 * d + 5), pos=_model(d, 2, 24, "cubic", 10 * d + 6, positive=True),
                          other=_model(d, 2, 37, "gaussian", 10 * d + 7))
    return _MODELS[d]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the cached models live on the default context, whose handle count other test files look at: freed when this file is done"""
    yield
    for M in _MODELS.values():
        for m in M.values():
            m.free()
    _MODELS.clear()
    _REFS.clear()


def containers(d, k):
    """"in_order": one model whose k outputs are the objectives in order.  "out_of_order": two two-output models -- objective 0 is the
    second output of the first, objectives 1 .. are outputs of the second, backwards at k = 3 (roles [NONE, 0 | 2, 1]); at k = 1 a second
    model would carry no objective row, so the one model has an unused output in front of its objective (roles [NONE, 0])"""
    M = models(d)
    one = M["m%d" % k]
    second = {1: [], 2: [sg.RefSurrogate(M["b"], [1])], 3: [sg.RefSurrogate(M["b"], [1, 0])]}[k]
    return {"in_order": sg.SurrogateContainer(objectives=[sg.RefSurrogate(one, list(range(k)))]),
            "out_of_order": sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["a"], [1])] + second)}


def inputs(d, k, ns=NS_MAX, seed=0):
    """x_n at least 0.1 inside [0, 1]^d, x within 0.02 of it, r < 0 drawn as tests/ds_util.make_qp draws its targets (p % 7 in (3, 4)
    / (5, 6): stretched by 3 sqrt(d) / by d, out of the box's reach), deltas around 0.3"""
    rng = np.random.default_rng(7000 + 101 * d + 11 * k + seed)
    X_n = rng.uniform(0.1, 0.9, (ns, d))
    X = np.clip(X_n + rng.uniform(-0.02, 0.02, (ns, d)), 0.0, 1.0)
    stretch = (1.0, 1.0, 1.0, 3.0 * np.sqrt(d), 3.0 * np.sqrt(d), float(d), float(d))
    R = np.stack([-rng.uniform(0.05, 1.0, k) * stretch[p % 7] for p in range(ns)])
    deltas = rng.uniform(0.2, 0.4, ns)
    return X, X_n, deltas, np.zeros(d), np.ones(d), R


def _cfg(max_loops=None, **kw):
    return descent.DirectedSearchConfig(reference_point=[0.0], max_loops=max_loops, **kw)


def _same(a, b):
    """== that also holds for NaN == NaN and -Inf == -Inf"""
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def chain_one(cfg, sc, x, x_n, delta, lb, ub, r):
    """the single calls chained for one start: (d', x+, mx+, mu, record) as the batch has to return them"""
    plan = sg.container_plan(sc)
    n, k = x_n.size, plan["k"]
    rc, om, dd, info, mu = descent.ds_criticality_device(plan, x_n, lb, ub, r, want_mult=True)
    status = info["status"]
    assert rc == (-2 if status == _lib.DS_GAVE_UP else 0), (rc, info)
    om_s, d_s = descent._ds_normalise(om, dd, status, n)
    nrm = float(np.max(np.abs(dd))) if status == _lib.DS_OK else 0.0
    rc, xp, mxp, sinfo = descent.sd_step_device(plan, cfg, x, x_n, float(delta), lb, ub, om_s, d_s)
    assert rc == 0, rc
    rec = dict(ds_status=status, iterations=info["iterations"], dropped=info["dropped"], branch=sinfo["branch"], loops=sinfo["loops"],
               omega=om, omega_step=sinfo["omega"], sigma=sinfo["sigma"], step_norm=sinfo["step_norm"], dnorm=nrm,
               branch_name=sinfo["branch_name"])
    if status == _lib.DS_GAVE_UP:          # the batch marks the rows; its step ran on (0, zeros), as this one did
        d_s, xp, mxp, mu = np.full(n, np.nan), np.full(n, np.nan), np.full(k, np.nan), np.full(k, np.nan)
    return d_s, xp, mxp, mu, rec


def chain(cfg, scs, X, X_n, deltas, lb, ub, R):
    rows = [chain_one(cfg, scs[p], X[p], X_n[p], deltas[p], lb, ub, R[p]) for p in range(len(scs))]
    return tuple(np.array([row[i] for row in rows]) for i in range(4)) + ([row[4] for row in rows],)


def batch(cfg, scs, X, X_n, deltas, lb, ub, R, out=None, expect_rc=0):
    plans = [sg.container_plan(sc) for sc in scs]
    rc, D, XP, MXP, MU, recs, ms = descent.ds_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, R, out=out)
    ctx = plans[0]["models"][0].ctx
    assert rc == expect_rc, (rc, ctx.lib.mrbf_last_error(ctx.h))
    if rc == 0:
        assert ms > 0
    return D, XP, MXP, MU, recs


def rows_of(res, idx):
    return tuple(a[idx] for a in res[:4]) + ([res[4][i] for i in idx],)


def assert_identical(got, ref, tag=None):
    assert len(got[4]) == len(ref[4]) and got[0].shape == ref[0].shape, tag
    for name, a, b in zip(("d", "x_plus", "mx_plus", "mu"), got[:4], ref[:4]):
        assert np.array_equal(a, b, equal_nan=True), (tag, name, np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:4])
    for p, (a, b) in enumerate(zip(got[4], ref[4])):
        for f in RECORD_FIELDS:
            assert _same(a[f], b[f]), (tag, p, f, a[f], b[f])


_REFS = {}


def reference(d, k, name, max_loops):
    """the chained single calls of the NS_MAX starts of one shape, computed once"""
    key = (d, k, name, max_loops)
    if key not in _REFS:
        sc = containers(d, k)[name]
        _REFS[key] = chain(_cfg(max_loops), [sc] * NS_MAX, *inputs(d, k))
    return _REFS[key]


@pytest.mark.parametrize("ns", [1, 5, 33])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("d", [2, 7, 65])
def test_bit_identity_with_the_chained_single_calls(d, k, ns):
    X, X_n, deltas, lb, ub, R = inputs(d, k)
    for name in ("in_order", "out_of_order"):
        sc = containers(d, k)[name]
        assert sg.container_plan(sc)["k"] == k
        for max_loops in (0, 6, 117):
            cfg = _cfg(max_loops if max_loops != 117 else None)
            assert cfg.max_loops == max_loops
            ref = reference(d, k, name, cfg.max_loops)
            got = batch(cfg, [sc] * ns, X[:ns], X_n[:ns], deltas[:ns], lb, ub, R[:ns])
            assert_identical(got, rows_of(ref, list(range(ns))), (d, k, ns, name, max_loops))       # every start, none left out
            # no planted start here: a GAVE_UP would be a finding about the QP
            assert [r["ds_status"] for r in got[4]] == [_lib.DS_OK] * ns, [(p, r["ds_status"]) for p, r in enumerate(got[4])]


def test_planted_starts_in_one_batch():
    d, k, ns = 7, 2, 9
    M = models(d)
    generic = sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["m2"], [0, 1])])
    positive = sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["pos"], [0, 1])])
    X, X_n, deltas, lb, ub, R = inputs(d, k, ns=ns, seed=1)
    R = -np.abs(R) / np.abs(R).max()             # within reach: the unplanted starts are plain OK starts
    scs = [generic] * ns
    CRIT_ZERO, CRIT_NAN, INFEAS, GAVE_UP, ZERO_D, HALF = 1, 3, 4, 6, 7, 8
    R[CRIT_ZERO, 1] = 0.0
    R[CRIT_NAN, 0] = np.nan
    X_n[INFEAS, 2] = ub[2] + 1.5
    X_n[GAVE_UP, 5] = ub[5] + 0.25
    scs[ZERO_D] = positive                       # every entry of G positive and x_n = lb: d >= 0 and G d <= 0 leave d = 0
    X_n[ZERO_D] = lb
    X_n[HALF, ::2] = np.where(np.arange(d)[::2] % 4 == 0, lb[::2], ub[::2])
    X = X_n.copy()
    X[INFEAS], X[GAVE_UP] = np.clip(X_n[INFEAS], lb, ub), np.clip(X_n[GAVE_UP], lb, ub)
    cfg = _cfg(6)
    got = batch(cfg, scs, X, X_n, deltas, lb, ub, R)
    ref = chain(cfg, scs, X, X_n, deltas, lb, ub, R)
    assert_identical(got, ref, "planted")
    D, XP, MXP, MU, recs = got
    expected = {CRIT_ZERO: _lib.DS_CRITICAL, CRIT_NAN: _lib.DS_CRITICAL, INFEAS: _lib.DS_INFEASIBLE, GAVE_UP: _lib.DS_GAVE_UP}
    assert [r["ds_status"] for r in recs] == [expected.get(p, _lib.DS_OK) for p in range(ns)]
    G = sg.eval_container_objectives_jacobian_at_scaled_site(positive, None, X_n[ZERO_D])
    assert np.all(G > 0)
    for p in (CRIT_ZERO, CRIT_NAN, INFEAS, ZERO_D):
        assert not D[p].any() and np.array_equal(XP[p], X_n[p]) and recs[p]["omega_step"] == 0.0 and recs[p]["dnorm"] == 0.0, p
    assert recs[CRIT_ZERO]["omega"] == 0.0 and recs[CRIT_NAN]["omega"] == 0.0 and recs[ZERO_D]["omega"] == 0.0
    assert recs[INFEAS]["omega"] == -np.inf
    for a in (D, XP, MXP, MU):
        assert np.all(np.isnan(a[GAVE_UP]))
    assert np.isnan(recs[GAVE_UP]["omega"])
    for p in (0, 2, 5, HALF):
        assert recs[p]["dnorm"] > 0 and np.max(np.abs(D[p])) == 1.0 and recs[p]["omega"] == recs[p]["omega_step"] > 0, (p, recs[p])
    # the neighbours of the start that gave up are bit-equal to a batch run without it
    keep = [p for p in range(ns) if p != GAVE_UP]
    without = batch(cfg, [scs[p] for p in keep], X[keep], X_n[keep], deltas[keep], lb, ub, R[keep])
    assert_identical(without, rows_of(got, keep), "without the start that gave up")


def test_both_sigma_branches_and_the_min_stepsize_rule():
    d, k, ns = 7, 2, 5
    sc = containers(d, k)["in_order"]
    _, X_n, _, lb, ub, R = inputs(d, k, ns=ns, seed=2)
    R = -np.abs(R) / np.abs(R).max()
    deltas = np.array([0.3, 2.5, 0.3, 2.5, 2.5])
    cfg = _cfg()
    got = batch(cfg, [sc] * ns, X_n, X_n, deltas, lb, ub, R)
    assert_identical(got, chain(cfg, [sc] * ns, X_n, X_n, deltas, lb, ub, R), "branches")
    for p, r in enumerate(got[4]):
        assert r["ds_status"] == _lib.DS_OK and np.max(np.abs(got[0][p])) == 1.0        # after normalisation ||d||_inf is exactly 1
        assert r["branch_name"] == ("delta" if deltas[p] == 0.3 else "intersect"), (p, r)
    big = _cfg(6, min_stepsize=10.0)
    got = batch(big, [sc] * ns, X_n, X_n, deltas, lb, ub, R)
    assert_identical(got, chain(big, [sc] * ns, X_n, X_n, deltas, lb, ub, R), "min_stepsize")
    for p, r in enumerate(got[4]):
        assert r["sigma"] <= 10.0 and r["omega_step"] == 0.0 and r["step_norm"] == 0.0 and r["loops"] == 0 and r["omega"] > 0
        assert np.array_equal(got[1][p], X_n[p])


def test_starts_whose_models_differ():
    """centre counts (24, 30, 37) and kernels (cubic, gaussian) differ from start to start: several launch groups per site"""
    d, k, ns = 7, 2, 5
    M = models(d)
    mods = [M["m2"], M["a"], M["other"], M["m2"], M["pos"]]
    scs = [sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])]) for m in mods]
    args = inputs(d, k, ns=ns, seed=3)
    cfg = _cfg(6)
    assert_identical(batch(cfg, scs, *args), chain(cfg, scs, *args), "models differ")


@pytest.mark.parametrize("d", [2, 65])
def test_position_independence(d):
    k, ns = 3, 5
    sc = containers(d, k)["out_of_order"]
    X, X_n, deltas, lb, ub, R = inputs(d, k, ns=ns, seed=4)
    cfg = _cfg(6)
    a = batch(cfg, [sc] * ns, X, X_n, deltas, lb, ub, R)
    assert_identical(batch(cfg, [sc] * ns, X, X_n, deltas, lb, ub, R), a, "the same call twice")
    perm = [3, 0, 4, 2, 1]
    b = batch(cfg, [sc] * ns, X[perm], X_n[perm], deltas[perm], lb, ub, R[perm])
    assert_identical(b, rows_of(a, perm), "permutation")


def test_device_pointers_and_arena_reuse():
    d, k = 65, 2
    sc = containers(d, k)["in_order"]
    X, X_n, deltas, lb, ub, R = inputs(d, k)
    cfg = _cfg(6)
    ref = reference(d, k, "in_order", 6)
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    ns = NS_MAX
    out = tuple(torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((ns, d), (ns, d), (ns, k), (ns, k)))
    torch.cuda.synchronize()
    c = batch(cfg, [sc] * ns, dev(X), dev(X_n), dev(deltas), dev(lb), dev(ub), dev(R), out=out)
    torch.cuda.synchronize()
    assert_identical(tuple(np.asarray(t.cpu()) for t in c[:4]) + (c[4],), ref, "device pointers")
    # 33 starts, then 1 start on the same context: the arena is laid out anew
    one = batch(cfg, [sc], X[4:5], X_n[4:5], deltas[4:5], lb, ub, R[4:5])
    assert_identical(one, rows_of(ref, [4]), "one start after 33")


def test_refused_shape_takes_the_loop():
    d, k, ns = 2, 2, 2
    M = models(d)
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(M["m2"], [0, 1])], nl_ineq_constraints=[sg.RefSurrogate(M["m1"], [0])])
    assert sg.container_plan(sc)["n_con"] == 1
    X, X_n, deltas, lb, ub, R = inputs(d, k, ns=ns, seed=5)
    cfg = descent.DirectedSearchConfig(reference_direction=[1.0, 1.0], max_loops=6)
    out = (np.full((ns, d), 7.0), np.full((ns, d), 7.0), np.full((ns, k), 7.0), np.full((ns, k), 7.0))
    batch(cfg, [sc] * ns, X, X_n, deltas, lb, ub, R, out=out, expect_rc=-2)
    assert all(np.all(o == 7.0) for o in out)                          # nothing is written on a negative code
    assert _lib.load().mrbf_dispatch_after(_lib.ENTRY_DS_BATCH, -2) == 1
    FX_n = np.stack([sg.eval_container_objectives_at_scaled_site(sc, None, x) for x in X_n])
    stats = {}
    res = descent.ds_iterate_many(cfg, [sc] * ns, None, X, X_n, FX_n, deltas, lb, ub, stats=stats)
    assert stats["path"] == "loop" and stats["rerouted"] == [] and len(res) == ns
    for p, (om, dd, xp, mxp, nrm) in enumerate(res):
        hom, hd = descent.get_criticality_ds(cfg, sc, None, X[p], X_n[p], FX_n[p], float(deltas[p]), lb, ub)
        ref = descent.compute_descent_step_ds(cfg, sc, None, X[p], X_n[p], float(deltas[p]), lb, ub, hom, hd)
        assert om == ref[0] and nrm == ref[3] and np.array_equal(dd, hd) and np.array_equal(xp, ref[1]) and np.array_equal(mxp, ref[2])


def test_ds_iterate_many_takes_the_batch():
    d, k, ns = 7, 2, 5
    sc = containers(d, k)["in_order"]
    X, X_n, deltas, lb, ub, _ = inputs(d, k, ns=ns, seed=6)
    FX_n = np.stack([sg.eval_container_objectives_at_scaled_site(sc, None, x) for x in X_n])
    cfg = descent.DirectedSearchConfig(reference_point=list(FX_n.min(axis=0) - 0.5))
    stats = {}
    res = descent.ds_iterate_many(cfg, [sc] * ns, None, X, X_n, FX_n, deltas, lb, ub, stats=stats)
    assert stats["path"] == "batch" and stats["rerouted"] == [] and stats["image_direction"] == "reference_point"
    assert len(stats["records"]) == ns and stats["ms_total"] > 0 and len(res) == ns
    for p, (om, dd, xp, mxp, nrm) in enumerate(res):
        hom, hd = descent.get_criticality_ds(cfg, sc, None, X[p], X_n[p], FX_n[p], float(deltas[p]), lb, ub)
        ref = descent.compute_descent_step_ds(cfg, sc, None, X[p], X_n[p], float(deltas[p]), lb, ub, hom, hd)
        assert om == ref[0] and nrm == ref[3] and np.array_equal(dd, hd) and np.array_equal(xp, ref[1]) and np.array_equal(mxp, ref[2])
        assert om > 0 and nrm > 0, (p, om, nrm)
