"""Many-start steepest descent on the device (run with -m gpu): mrbf_sd_iterate_batch against mrbf_sd_criticality + mrbf_sd_step
chained per start.  Bit identity is the contract: every output array with np.array_equal, every record field with ==.  Shapes: d = 3
(dpad 64, odd row length), 65 (first dpad 128: unsplit centre range at n = 150), 129 (first dpad 256: split centre range at n = 278)
-- the smallest at which the per-start offsets and the grouping of the evaluations can go wrong."""
import ctypes
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
    from tests import test_gpu_sd_step as base          # its models (cached per dimension) and its host-mirror check

DIMS = [3, 65, 129]
NS = 5
RECORD_FIELDS = ("sd_status", "iterations", "bound_flips", "branch", "loops", "omega", "omega_step", "sigma", "step_norm")


def _lin(name, d):
    if name != "shared":
        return None
    rng = np.random.default_rng(77 + d)
    return (np.zeros((0, d)), np.zeros(0), rng.standard_normal((2, d)) / np.sqrt(d), np.full(2, 2.0))


def _starts(d, ns=NS, seed=0, spread=0.02):
    rng = np.random.default_rng(500 + 13 * d + seed)
    X = rng.uniform(-1.0, 1.0, (ns, d))
    return X, X + rng.uniform(-spread, spread, (ns, d))


def _same(a, b):
    """== that also holds for NaN == NaN and -Inf == -Inf (sigma of a zero direction, omega of an infeasible LP)"""
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def chain(cfg, scs, X, X_n, deltas, lb, ub, lin):
    """the two single calls chained per start: (d, x+, mx+) arrays and the records the batch has to reproduce"""
    ns, n = X.shape
    D, XP, MXP, recs = np.empty((ns, n)), np.empty((ns, n)), [], []
    for p in range(ns):
        plan = sg.container_plan(scs[p])
        rc, om, dd, cinfo = descent.sd_criticality_device(plan, X[p], X_n[p], lb, ub, cfg.normalize, lin)
        assert rc == 0 and cinfo["status"] != _lib.SD_GAVE_UP, (p, rc, cinfo)
        rc, xp, mxp, sinfo = descent.sd_step_device(plan, cfg, X[p], X_n[p], float(deltas[p]), lb, ub, om, dd, lin)
        assert rc == 0, (p, rc)
        D[p], XP[p] = dd, xp
        MXP.append(mxp)
        recs.append(dict(sd_status=cinfo["status"], iterations=cinfo["iterations"], bound_flips=cinfo["bound_flips"], branch=sinfo["branch"],
                         loops=sinfo["loops"], omega=om, omega_step=sinfo["omega"], sigma=sinfo["sigma"], step_norm=sinfo["step_norm"],
                         branch_name=sinfo["branch_name"]))
    return D, XP, np.array(MXP), recs


def batch(cfg, scs, X, X_n, deltas, lb, ub, lin, out=None, expect_rc=0):
    plans = [sg.container_plan(sc) for sc in scs]
    rc, D, XP, MXP, recs, ms = descent.sd_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, lin, out=out)
    assert rc == expect_rc, (rc, plans[0]["models"][0].ctx.lib.mrbf_last_error(plans[0]["models"][0].ctx.h))
    if rc == 0:
        assert ms > 0
    return D, XP, MXP, recs


def assert_identical(got, ref, tag=None):
    (D, XP, MXP, recs), (rD, rXP, rMXP, rrecs) = got, ref
    assert np.array_equal(D, rD), tag
    assert np.array_equal(XP, rXP), tag
    assert np.array_equal(MXP, rMXP), tag
    assert len(recs) == len(rrecs)
    for p, (a, b) in enumerate(zip(recs, rrecs)):
        for f in RECORD_FIELDS:
            assert _same(a[f], b[f]), (tag, p, f, a[f], b[f])


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", ["in_order", "three_models", "shared"])
def test_bit_identity_with_the_chained_single_calls(d, name):
    sc = base.containers(d)[name]
    lin = _lin(name, d)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X, X_n = _starts(d)
    deltas = np.array([0.3, 0.25, 0.4, 0.35, 0.3])
    for max_loops in (12, None):
        for strict in (True, False):
            cfg = descent.SteepestDescentConfig(strict_backtracking=strict, max_loops=max_loops)
            assert cfg.max_loops == (12 if max_loops else 117)
            ref = chain(cfg, [sc] * NS, X, X_n, deltas, lb, ub, lin)
            got = batch(cfg, [sc] * NS, X, X_n, deltas, lb, ub, lin)
            assert_identical(got, ref, (d, name, max_loops, strict))
            assert all(r["sd_status"] == _lib.SD_OK for r in got[3]), got[3]


def test_starts_whose_models_differ():
    """the number of centres (40 and 57) and one start's shape parameter differ: members of one model slot fall into different launch
    groups, and every start still reproduces its own chain"""
    d = 3
    rng = np.random.default_rng(91)

    def fit(n, sp):
        C = rng.uniform(-2.0, 2.0, (n, d))
        cfgm = pkg.RbfConfig(kernel="multiquadric", shape_parameter=sp, polynomial_degree=1)
        return pkg.update_model(cfgm, C, np.stack([base.f_a(C), base.f_b(C)], axis=1))

    mods = [fit(40, 1.0), fit(57, 1.0), fit(40, 2.5), fit(57, 1.0), fit(40, 1.0)]
    scs = [sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])]) for m in mods]
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X, X_n = _starts(d, seed=3)
    deltas = np.full(NS, 0.3)
    cfg = descent.SteepestDescentConfig()
    assert_identical(batch(cfg, scs, X, X_n, deltas, lb, ub, None), chain(cfg, scs, X, X_n, deltas, lb, ub, None))
    for m in mods:
        m.free()


@pytest.mark.parametrize("d", DIMS)
def test_all_three_sigma_branches_in_one_batch(d):
    """delta = 0.3 gives "delta"; delta = 1.5 at x = x_n gives "intersect" where the LP's direction reaches a bound at +-1 and "one"
    where it stays inside.  The global box is wide in coordinate 0 only ([-2, 2]; elsewhere every iterate has less than 1 of room
    on either side), so ||d||_inf = 1 iff d_0 = +-1: the objectives f_c and f_a agree on coordinate 0 below -0.5 and pull against each
    other above.  Which candidate lands on which branch is read off the chained single calls (the reference), not assumed."""
    sc = base.containers(d)["shared"]
    lin = _lin("shared", d)
    lb, ub = np.full(d, -0.45), np.full(d, 0.45)
    lb[0], ub[0] = -2.0, 2.0
    cfg = descent.SteepestDescentConfig()
    rng = np.random.default_rng(40 + d)
    x0s = [-1.5, -1.2, -0.9, 0.0, 0.25, 0.5]      # (the modelled inequality x_0 + ... <= 0.1 caps d_0 at about 0.1 - x_0: below 1 from -0.9 on)
    P = rng.uniform(-0.4, 0.4, (1 + len(x0s), d))
    P[1:, 0] = x0s
    deltas = np.array([0.3] + [1.5] * len(x0s))
    ref = chain(cfg, [sc] * len(P), P, P, deltas, lb, ub, lin)
    names = [r["branch_name"] for r in ref[3]]
    print("d = %d branches:" % d, names, "||d||_inf:", [float(np.max(np.abs(v))) for v in ref[0]])
    assert names[0] == "delta" and {"one", "intersect"} <= set(names[1:]), names
    pick = [0, names.index("one"), names.index("intersect")]
    sub = (ref[0][pick], ref[1][pick], ref[2][pick], [ref[3][i] for i in pick])
    got = batch(cfg, [sc] * 3, P[pick], P[pick], deltas[pick], lb, ub, lin)
    assert [r["branch_name"] for r in got[3]] == ["delta", "one", "intersect"]
    assert_identical(got, sub, d)


def test_empty_box():
    d = 3
    sc = base.containers(d)["in_order"]
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    lb[0], ub[0] = 1.0, 0.5
    X, X_n = _starts(d, seed=7)
    deltas = np.full(NS, 0.3)
    cfg = descent.SteepestDescentConfig()
    got = batch(cfg, [sc] * NS, X, X_n, deltas, lb, ub, None)       # return code 0 (asserted inside)
    D, XP, MXP, recs = got
    assert all(r["sd_status"] == _lib.SD_INFEASIBLE and r["omega"] == -np.inf for r in recs), recs
    assert np.array_equal(D, np.zeros((NS, d))) and np.array_equal(XP, X_n)
    assert_identical(got, chain(cfg, [sc] * NS, X, X_n, deltas, lb, ub, None))


@pytest.mark.parametrize("d", DIMS)
def test_position_independence(d):
    sc = base.containers(d)["three_models"]
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X, X_n = _starts(d, seed=9)
    deltas = np.array([0.3, 0.25, 0.4, 0.35, 0.3])
    cfg = descent.SteepestDescentConfig(max_loops=12)
    a = batch(cfg, [sc] * NS, X, X_n, deltas, lb, ub, None)
    perm = np.array([3, 0, 4, 2, 1])
    b = batch(cfg, [sc] * NS, X[perm], X_n[perm], deltas[perm], lb, ub, None)
    assert_identical(b, (a[0][perm], a[1][perm], a[2][perm], [a[3][i] for i in perm]), "permutation")
    one = batch(cfg, [sc], X[2:3], X_n[2:3], deltas[2:3], lb, ub, None)
    assert_identical(one, (a[0][2:3], a[1][2:3], a[2][2:3], a[3][2:3]), "batch of one")


def test_device_pointers_and_allocation():
    d = 65
    sc = base.containers(d)["shared"]
    lin = _lin("shared", d)
    k = sg.container_plan(sc)["k"]
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X, X_n = _starts(d, seed=11)
    deltas = np.array([0.3, 0.25, 1.5, 0.35, 0.3])
    cfg = descent.SteepestDescentConfig()
    ctx = sg.container_plan(sc)["models"][0].ctx
    a = batch(cfg, [sc] * NS, X, X_n, deltas, lb, ub, lin)
    arena = ctx.get_option(_lib.OPT_ARENA_BYTES)
    b = batch(cfg, [sc] * NS, X, X_n, deltas, lb, ub, lin)
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) == arena          # a second identical call allocates nothing
    assert_identical(b, a, "second call")
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    out = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in ((NS, d), (NS, d), (NS, k)))
    torch.cuda.synchronize()
    c = batch(cfg, [sc] * NS, dev(X), dev(X_n), dev(deltas), dev(lb), dev(ub), lin, out=out)
    torch.cuda.synchronize()
    assert_identical(tuple(np.asarray(t.cpu()) for t in c[:3]) + (c[3],), a, "device pointers")


def test_refused_shape_takes_the_loop():
    d = 300
    rng = np.random.default_rng(15)
    C = rng.uniform(-2.0, 2.0, (40, d))             # the tail is not unisolvent on 40 sites: no tail, the shape is what matters here
    mod = pkg.update_model(pkg.RbfConfig(kernel="gaussian", polynomial_degree=-1), C, np.stack([base.f_a(C), base.f_b(C)], axis=1))
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, [0, 1])])
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X, X_n = _starts(d, ns=2, seed=17)
    deltas = np.full(2, 0.3)
    cfg = descent.SteepestDescentConfig(max_loops=12)
    batch(cfg, [sc] * 2, X, X_n, deltas, lb, ub, None, expect_rc=-2)
    assert _lib.load().mrbf_dispatch_after(_lib.ENTRY_SD_BATCH, -2) == 1
    stats = {}
    res = descent.sd_iterate_many(cfg, [sc] * 2, None, X, X_n, deltas, lb, ub, stats=stats)
    assert stats["path"] == "loop" and stats["rerouted"] == []
    for p, (om, dd, xp, mxp, nrm) in enumerate(res):
        hom, hd = descent.get_criticality_sd(cfg, sc, None, X[p], X_n[p], lb, ub)
        ref = descent.compute_descent_step_sd_routed(cfg, sc, None, X[p], X_n[p], 0.3, lb, ub, hom, hd)
        assert om == ref[0] and nrm == ref[3] and np.array_equal(dd, hd) and np.array_equal(xp, ref[1]) and np.array_equal(mxp, ref[2])
    mod.free()


def test_sd_iterate_many_takes_the_batch():
    d = 3
    sc = base.containers(d)["in_order"]
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X, X_n = _starts(d, seed=19)
    deltas = np.full(NS, 0.3)
    cfg = descent.SteepestDescentConfig()
    stats = {}
    res = descent.sd_iterate_many(cfg, [sc] * NS, None, X, X_n, deltas, lb, ub, stats=stats)
    assert stats["path"] == "batch" and stats["rerouted"] == []
    for p, (om, dd, xp, mxp, nrm) in enumerate(res):
        hom, hd = descent.get_criticality_sd(cfg, sc, None, X[p], X_n[p], lb, ub)
        ref = descent.compute_descent_step_sd_routed(cfg, sc, None, X[p], X_n[p], 0.3, lb, ub, hom, hd)
        assert om == ref[0] and nrm == ref[3] and np.array_equal(dd, hd) and np.array_equal(xp, ref[1]) and np.array_equal(mxp, ref[2])


def test_single_calls_unchanged_against_the_host_mirror():
    """the single calls run through the kernels that now carry a start index: mrbf_sd_criticality against the HiGHS direction LP to
    the tolerance tests/test_gpu_sd.py uses, mrbf_sd_step against the host mirror by tests/test_gpu_sd_step.py's own check()"""
    text = open(os.path.join(ROOT, "tests", "test_gpu_sd.py")).read()
    tol = float(re.search(r"abs\(om - hom\) <= (1e-\d+) \* max\(1\.0, abs\(hom\)\)", text).group(1))
    assert "_rel(xp, hxp) <= 1e-13" in open(os.path.join(ROOT, "tests", "test_gpu_sd_step.py")).read()    # what check() applies
    d = 3
    sc = base.containers(d)["in_order"]
    plan = sg.container_plan(sc)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    X, X_n = _starts(d, seed=21)
    for strict in (True, False):
        cfg = descent.SteepestDescentConfig(strict_backtracking=strict)
        for p in range(NS):
            rc, om, dd, info = descent.sd_criticality_device(plan, X[p], X_n[p], lb, ub, True)
            G, A_eq, b_eq, A_in, b_in = descent._sd_host_rows(sc, None, X[p], X_n[p], None)
            hd, hom, hst = descent._steepest_descent_direction(X_n[p], G, lb, ub, A_eq, b_eq, A_in, b_in, True, want_status=True)
            assert rc == 0 and info["status"] == hst == _lib.SD_OK
            assert abs(om - hom) <= tol * max(1.0, abs(hom)), (om, hom)
            base.check(cfg, sc, X[p], X_n[p], 0.3, lb, ub, om, dd, branch="delta", margin=False)
            base.check(cfg, sc, X[p], X_n[p], 3.0, lb, ub, om, dd)
