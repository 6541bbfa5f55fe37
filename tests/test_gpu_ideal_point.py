"""Local ideal points on the device (run with -m gpu): mrbf_ideal_point_problem / mrbf_ideal_point_batch, the ideal-point phase of the
Pascoletti-Serafini step as calls of their own, and the default image direction of directed search through them.  Two contracts, both
bit identity on one context:
  A  against the existing phase: mrbf_ps_step_problem with r_or_null = NULL, the same max_ideal_evals, xtol_rel and seed returns
     r_out == fx_n - ideal_out element by element for every fx_n, the same evals_ideal, and for a critical start mx_trial == mx_out;
  B  batch against loop: every output of the batch call for start p is the single call's on p's container with seeds[p] (ms_total aside).
Models: cubic, degree-1 tail, random sites in the unit box, boxes +- 0.1 around x_n.  Shapes (d, n, k), the smallest at which something
different happens:
  (3, 40, 2)     dpad 64
  (50, 120, 2)   lambda = 1020, below 1024
  (51, 120, 2)   lambda = 1040: the several-compute-unit ranking
  (65, 131, 2)   dpad 128
  (129, 259, 3)  dpad 256, two outputs per values pass
Budgets (max_ideal_evals): 200 (below 260: nothing is kept back, no refinement runs); 4 * 20 (d + 1) (a tenth kept back, the refinement
runs); -1, the default, at d = 3 only.
Measured on an MI355X, the largest |mrbf_eval(x_ideal_l)_l - ideal_l| / (1 + |ideal_l|) over every start, shape and budget here
(test_x_ideal_lies_in_the_box_and_carries_the_value, bound 1e-10): 0 at d = 3, 50, 51, 65; 5.0e-16 at d = 129."""
import ctypes
import os

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import pascoletti_serafini as ps
    from morbit.jl_amd import surrogates as sg

SHAPES = [(3, 40, 2), (50, 120, 2), (51, 120, 2), (65, 131, 2), (129, 259, 3)]
NS = 9
INFO_FIELDS = ("evals_ideal", "generations", "found", "refined")


def budgets(d):
    return [200, 4 * 20 * (d + 1)] + ([-1] if d == 3 else [])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _handle(m):
    return m.model.value if hasattr(m.model, "value") else m.model


def _opts(budget, seed=1, max_ps=0):
    return _lib.PsOptions(budget, max_ps, 0, 0, seed, -0.5, 1e-3)


def _problem(rows, roles, k, lin, eq_tol, with_models):
    """mrbf_ps_problem for model rows `rows` (a list of model lists); the second value keeps the arrays alive"""
    A_eq, b_eq, A_in, b_in = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (lin or (None,) * 4)]
    hs = [_handle(m) for row in rows for m in row]
    handles = (ctypes.c_void_p * len(hs))(*hs)
    roles_c = (ctypes.c_int32 * len(roles))(*roles)
    prob = _lib.PsProblem(n_models=len(rows[0]), n_objectives=k, models=handles if with_models else None, roles=roles_c,
                          n_lin_eq=0 if b_eq is None else b_eq.size, n_lin_ineq=0 if b_in is None else b_in.size,
                          A_eq=None if b_eq is None else A_eq.ctypes.data, b_eq=None if b_eq is None else b_eq.ctypes.data,
                          A_ineq=None if b_in is None else A_in.ctypes.data, b_ineq=None if b_in is None else b_in.ctypes.data, eq_tol=float(eq_tol))
    return prob, (handles, roles_c, A_eq, b_eq, A_in, b_in)


def ideal_single(row, roles, k, x_n, lb, ub, budget, seed, lin=None, eq_tol=-1.0, want_x=True, want_mx=True):
    """one mrbf_ideal_point_problem call: (ideal, x_ideal, mx, info dict)"""
    ctx = row[0].ctx
    d = x_n.size
    prob, keep = _problem([row], roles, k, lin, eq_tol, True)
    opts = _opts(budget, seed, max_ps=-1)
    ideal, xi, mx = np.full(k, np.nan), np.full((k, d), np.nan) if want_x else None, np.full(k, np.nan) if want_mx else None
    info = _lib.IdealInfo()
    P = _lib.as_ptr
    rc = ctx.lib.mrbf_ideal_point_problem(ctx.h, ctypes.byref(prob), P(np.ascontiguousarray(x_n)), P(np.ascontiguousarray(lb)),
                                          P(np.ascontiguousarray(ub)), ctypes.byref(opts), P(ideal), P(xi), P(mx), ctypes.byref(info))
    assert rc == 0, (rc, ctx.lib.mrbf_last_error(ctx.h))
    assert info.ms_total > 0
    return ideal, xi, mx, info.asdict()


def ideal_loop(rows, roles, k, X_n, LB, UB, budget, seeds, lin=None, eq_tol=-1.0):
    """the loop of single calls the batch has to reproduce: (ideal, x_ideal, mx, infos)"""
    outs = [ideal_single(rows[p], roles, k, X_n[p], LB[p], UB[p], budget, seeds[p], lin, eq_tol) for p in range(len(rows))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]), [o[3] for o in outs]


def ideal_batch(rows, roles, k, X_n, LB, UB, budget, seeds, lin=None, eq_tol=-1.0, device=False, opt_seed=1, want_x=True, want_mx=True):
    ctx = rows[0][0].ctx
    ns, d = X_n.shape
    prob, keep = _problem(rows, roles, k, lin, eq_tol, False)
    seeds_c = None if seeds is None else (ctypes.c_uint64 * ns)(*[int(s) for s in seeds])
    opts = _opts(budget, opt_seed, max_ps=-1)
    infos = (_lib.IdealInfo * ns)()
    ms = ctypes.c_float()
    if device:
        ins = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X_n, LB, UB)]
        outs = [torch.empty((ns, k), dtype=torch.float64, device="cuda"), torch.empty((ns, k, d), dtype=torch.float64, device="cuda"),
                torch.empty((ns, k), dtype=torch.float64, device="cuda")]
        torch.cuda.synchronize()
    else:
        ins = [np.ascontiguousarray(a) for a in (X_n, LB, UB)]
        outs = [np.full((ns, k), np.nan), np.full((ns, k, d), np.nan), np.full((ns, k), np.nan)]
    if not want_x:
        outs[1] = None
    if not want_mx:
        outs[2] = None
    rc = ctx.lib.mrbf_ideal_point_batch(ctx.h, ns, ctypes.byref(prob), keep[0], *[_lib.as_ptr(a) for a in ins], ctypes.byref(opts), seeds_c,
                                        *[_lib.as_ptr(a) for a in outs], infos, ctypes.byref(ms))
    assert rc == 0, (rc, ctx.lib.mrbf_last_error(ctx.h))
    assert ms.value > 0 and all(i.ms_total == ms.value for i in infos)
    if device:
        outs = [None if o is None else o.cpu().numpy() for o in outs]
    return outs[0], outs[1], outs[2], [i.asdict() for i in infos]


def assert_identical(got, ref, tag=None, rows=None):
    sel = slice(None) if rows is None else rows
    for a, b, name in zip(got[:3], ref[:3], ("ideal", "x_ideal", "mx")):
        if a is not None:
            assert np.array_equal(_bits(a), _bits(b[sel])), (tag, name)
    rinfos = ref[3] if rows is None else [ref[3][p] for p in rows]
    assert len(got[3]) == len(rinfos)
    for p, (a, b) in enumerate(zip(got[3], rinfos)):
        for f in INFO_FIELDS:
            assert a[f] == b[f], (tag, p, f, a[f], b[f])


def _fun(C, k):
    cols = [np.sum((C - 0.3) ** 2, axis=1), np.sum((C - 0.7) ** 2, axis=1) + 0.1 * np.sin(3.0 * C[:, 0]),
            np.sum((C - 0.5) ** 2 * np.linspace(0.5, 1.5, C.shape[1])[None, :], axis=1) + 0.2 * np.cos(2.0 * C[:, -1])]
    return np.stack(cols[:k], axis=1)


_CASES = {}
_OWN = []      # models fitted outside `case`


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the cached models live on the default context, whose handle count other test files look at: freed when this file is done"""
    yield
    for c in _CASES.values():
        for row in c["rows"]:
            for m in row:
                m.free()
    for m in _OWN:
        m.free()
    _CASES.clear()
    _OWN.clear()


def case(d, n, k):
    """NS starts of one problem: every start its own sites, the odd starts p more of them (the models differ in n), its own box and
    seed; fitted once.  refs[budget]: the loop of single calls, computed once and shared by the tests that compare with it."""
    key = (d, n, k)
    if key not in _CASES:
        rng = np.random.default_rng(2400 + 7 * d)
        rows = []
        for p in range(NS):
            C = rng.random((n + (p if p % 2 else 0), d))
            rows.append([pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, _fun(C, k))])
        X_n = rng.uniform(0.2, 0.8, (NS, d))
        LB, UB = X_n - 0.1, X_n + 0.1
        seeds = [11 + 3 * p for p in range(NS)]
        _CASES[key] = dict(rows=rows, roles=list(range(k)), k=k, X_n=X_n, LB=LB, UB=UB, seeds=seeds, refs={})
    return _CASES[key]


def reference(c, budget):
    if budget not in c["refs"]:
        c["refs"][budget] = ideal_loop(c["rows"], c["roles"], c["k"], c["X_n"], c["LB"], c["UB"], budget, c["seeds"])
    return c["refs"][budget]


def ps_single(row, roles, k, x_n, lb, ub, fx, budget, seed, lin=None, eq_tol=-1.0):
    """mrbf_ps_step_problem with r_or_null = NULL and the smallest max_ps_evals the call accepts (0): (x_trial, mx_trial, r_out, info)"""
    ctx = row[0].ctx
    d = x_n.size
    prob, keep = _problem([row], roles, k, lin, eq_tol, True)
    opts = _opts(budget, seed, max_ps=0)
    xt, mt, ro = np.empty(d), np.empty(k), np.empty(k)
    info = _lib.PsInfo()
    P = _lib.as_ptr
    rc = ctx.lib.mrbf_ps_step_problem(ctx.h, ctypes.byref(prob), P(np.ascontiguousarray(x_n)), P(np.ascontiguousarray(lb)), P(np.ascontiguousarray(ub)),
                                      P(np.ascontiguousarray(fx)), None, ctypes.byref(opts), P(xt), P(mt), P(ro), ctypes.byref(info))
    assert rc == 0, (rc, ctx.lib.mrbf_last_error(ctx.h))
    return xt, mt, ro, info.asdict()


def assert_contract_a(row, roles, k, x_n, lb, ub, budget, seed, got, tag, lin=None, eq_tol=-1.0):
    """`got` = the ideal-point call's outputs; two fx_n: one above the ideal point (the PS phase is entered) and one far below it
    (r <= 0: the start is critical and mx_trial is m(x_n))"""
    ideal, _, mx, info = got
    for fx in (mx + np.linspace(0.25, 0.75, k), np.full(k, -1e6)):
        xt, mt, ro, pinfo = ps_single(row, roles, k, x_n, lb, ub, fx, budget, seed, lin, eq_tol)
        assert np.array_equal(_bits(fx - ideal), _bits(ro)), (tag, fx, ideal, ro)
        assert pinfo["evals_ideal"] == info["evals_ideal"], (tag, pinfo, info)
        if fx[0] < 0:
            assert pinfo["status"] == _lib.PS_CRITICAL and np.array_equal(_bits(mt), _bits(mx)), (tag, pinfo)


@pytest.mark.parametrize("d, n, k", SHAPES)
def test_contract_a_the_phase_of_the_ps_step(d, n, k):
    c = case(d, n, k)
    for budget in budgets(d):
        ref = reference(c, budget)
        for p in (0, 3):
            got = tuple(a[p] for a in ref[:3]) + (ref[3][p],)
            assert_contract_a(c["rows"][p], c["roles"], k, c["X_n"][p], c["LB"][p], c["UB"][p], budget, c["seeds"][p], got, (d, budget, p))
        full = (1 << k) - 1
        for info in ref[3]:
            assert info["found"] == full and info["generations"] > 0, info
            assert info["refined"] == (0 if budget == 200 else full), (budget, info)
            cap = 500 * (d + 1) if budget < 0 else budget
            assert 0 < info["evals_ideal"] <= k * cap, (budget, info)


@pytest.mark.parametrize("d, n, k", SHAPES)
def test_contract_b_batch_against_the_loop(d, n, k):
    c = case(d, n, k)
    arrs = lambda idx: ([c["rows"][p] for p in idx], c["roles"], k, c["X_n"][idx], c["LB"][idx], c["UB"][idx])
    for budget in budgets(d)[:2] if d <= 50 else budgets(d)[1:2]:
        ref = reference(c, budget)
        for ns in (1, 5, 9):
            idx = list(range(ns))
            assert_identical(ideal_batch(*arrs(idx), budget, [c["seeds"][p] for p in idx]), ref, (d, budget, ns), rows=idx)
        # 9 starts followed by 1 on the same context
        assert_identical(ideal_batch(*arrs([2]), budget, [c["seeds"][2]]), ref, (d, budget, "one after nine"), rows=[2])
    # a permutation and a repetition of starts
    perm = [3, 0, 4, 2, 1, 3, 3]
    assert_identical(ideal_batch(*arrs(perm), budget, [c["seeds"][p] for p in perm]), ref, "permutation", rows=perm)


def test_seeds_against_the_options_seed_and_device_pointers():
    d, n, k = SHAPES[0]
    c = case(d, n, k)
    budget = budgets(d)[1]
    args = (c["rows"], c["roles"], k, c["X_n"], c["LB"], c["UB"])
    ref77 = ideal_loop(*args, budget, [77] * NS)
    assert_identical(ideal_batch(*args, budget, None, opt_seed=77), ref77, "seeds NULL")
    ref = reference(c, budget)
    assert not np.array_equal(_bits(ref77[0]), _bits(ref[0]))            # the seed is the generator's key
    assert_identical(ideal_batch(*args, budget, c["seeds"], opt_seed=77), ref, "seeds win")
    assert_identical(ideal_batch(*args, budget, c["seeds"], device=True), ref, "device pointers")
    # NULL x_ideal_out and NULL mx_out are accepted, by both calls
    got = ideal_batch(*args, budget, c["seeds"], want_x=False, want_mx=False)
    assert got[1] is None and got[2] is None
    assert_identical(got, ref, "optional outputs")
    one = ideal_single(c["rows"][1], c["roles"], k, c["X_n"][1], c["LB"][1], c["UB"][1], budget, c["seeds"][1], want_x=False, want_mx=False)
    assert_identical((one[0][None], None, None, [one[3]]), ref, "optional outputs, single", rows=[1])


@pytest.mark.parametrize("d, n, k", [SHAPES[0], SHAPES[3]])
def test_a_batch_processed_in_chunks_of_starts(d, n, k):
    """MRBF_PS_CHUNK_KB sets the limit the batch is cut by: with 1 KiB every start is a chunk of its own, with the second limit the
    nine starts go in chunks of a few (a start takes about 100 KiB at d = 3 and 2.5 MiB at d = 65)"""
    c = case(d, n, k)
    budget = budgets(d)[1]
    ref = reference(c, budget)
    keep = os.environ.get("MRBF_PS_CHUNK_KB")
    try:
        for kb in (1, 400 if d == 3 else 8000):
            os.environ["MRBF_PS_CHUNK_KB"] = str(kb)
            assert_identical(ideal_batch(c["rows"], c["roles"], k, c["X_n"], c["LB"], c["UB"], budget, c["seeds"]), ref, ("chunks", kb))
    finally:
        if keep is None:
            os.environ.pop("MRBF_PS_CHUNK_KB", None)
        else:
            os.environ["MRBF_PS_CHUNK_KB"] = keep


def _eval(m, X):
    return pkg.eval_models_at_sites(m, None, np.atleast_2d(X))


class batch_from:
    """`with batch_from(2):` -- the bindings take the batch call from that many starts on (IDEAL_BATCH_MIN_STARTS is a measured
    routing constant; the tests of the routing must not depend on its value)"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.keep = ps.IDEAL_BATCH_MIN_STARTS
        ps.IDEAL_BATCH_MIN_STARTS = self.n

    def __exit__(self, *exc):
        ps.IDEAL_BATCH_MIN_STARTS = self.keep


@pytest.mark.parametrize("d, n, k", SHAPES)
def test_x_ideal_lies_in_the_box_and_carries_the_value(d, n, k):
    """x_ideal inside [lb_eff, ub_eff] by exact comparison; mrbf_eval of objective l at x_ideal[l] against ideal[l] within the
    project's value tolerance 1e-10 (1 + |ideal_l|) -- two evaluation paths over the same weights, the fit's conditioning does not
    enter; mx against mrbf_eval at x_n likewise"""
    c = case(d, n, k)
    worst = 0.0
    for budget in budgets(d):
        ideal, xi, mx, infos = reference(c, budget)
        for p in range(NS):
            assert np.all(xi[p] >= c["LB"][p][None, :]) and np.all(xi[p] <= c["UB"][p][None, :]), (budget, p)
            V = _eval(c["rows"][p][0], xi[p])
            for l in range(k):
                dev = abs(V[l, l] - ideal[p, l]) / (1.0 + abs(ideal[p, l]))
                worst = max(worst, dev)
                assert dev <= 1e-10, (budget, p, l, V[l, l], ideal[p, l])
            m_xn = _eval(c["rows"][p][0], c["X_n"][p])[0]
            assert np.all(np.abs(m_xn - mx[p]) <= 1e-10 * (1.0 + np.abs(mx[p])))
            assert np.all(ideal[p] <= mx[p] + 1e-10 * (1.0 + np.abs(mx[p])))     # x_n is an individual of every run
    print("ideal-point value deviation (d = %d): %.3e" % (d, worst))


def _constrained_case():
    """objectives from two grouped models, a modelled inequality and a modelled equality (rows of the first model), linear rows"""
    if "con" not in _CASES:
        rng = np.random.default_rng(12)
        d, n, ns = 12, 150, 5
        rows = []
        for p in range(ns):
            C = rng.random((n + 10 * p, d))
            Ya = np.stack([np.sum((C - 0.3) ** 2, axis=1), C[:, 0] - 0.52, C[:, 2] - C[:, 4]], axis=1)     # objective 0 | g(x) <= 0 | h(x) = 0
            Yb = np.sum((C - 0.7) ** 2, axis=1, keepdims=True)                                               # objective 1
            rows.append([pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, Ya),
                         pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, Yb)])
        X_n = np.tile(np.array([0.5, 0.85, 0.4, 0.2, 0.4, 0.5] * 2), (ns, 1)) + rng.uniform(-0.01, 0.01, (ns, d))
        X_n[:, 4] = X_n[:, 2]
        A = np.zeros((1, d))
        A[0, 1] = A[0, 3] = 1.0
        _CASES["con"] = dict(rows=rows, roles=[0, _lib.ROLE_INEQ, _lib.ROLE_EQ, 1], k=2, X_n=X_n, LB=X_n - 0.1, UB=X_n + 0.1,
                             seeds=[5, 6, 7, 8, 9], lin=(None, None, A, np.array([1.1])), refs={})
    return _CASES["con"]


def test_container_with_two_models_constraints_and_linear_rows():
    c = _constrained_case()
    d, k = 12, 2
    for budget in (200, 4 * 20 * (d + 1)):
        args = (c["rows"], c["roles"], k, c["X_n"], c["LB"], c["UB"], budget, c["seeds"])
        ref = ideal_loop(*args, lin=c["lin"], eq_tol=0.02)
        assert_identical(ideal_batch(*args, lin=c["lin"], eq_tol=0.02), ref, ("container", budget))
        for p in (0, 4):
            got = tuple(a[p] for a in ref[:3]) + (ref[3][p],)
            assert_contract_a(c["rows"][p], c["roles"], k, c["X_n"][p], c["LB"][p], c["UB"][p], budget, c["seeds"][p], got, ("container", budget, p),
                              lin=c["lin"], eq_tol=0.02)
        assert all(i["found"] == 3 for i in ref[3]), ref[3]
        # the points found satisfy what the runs carried
        for p in range(len(c["rows"])):
            for l in range(k):
                x = ref[1][p, l]
                g = _eval(c["rows"][p][0], x)[0]
                assert g[1] <= 0.0 and abs(g[2]) <= 0.02 and x[1] + x[3] <= 1.1, (budget, p, l, g, x[1] + x[3])


def test_a_box_no_point_of_which_is_feasible():
    """a linear inequality x_0 <= 0.3 that no point of start 2's box satisfies: found == 0, ideal == mx, x_ideal == x_n for every
    objective of that start; the clean starts beside it are what they are in a batch without it"""
    d, n, k = SHAPES[0]
    c = case(d, n, k)
    budget = budgets(d)[1]
    A = np.zeros((1, d))
    A[0, 0] = 1.0
    lin = (None, None, A, np.array([0.3]))
    X_n = c["X_n"][:5].copy()
    X_n[:, 0] = 0.25                              # the clean starts: part of the box is feasible
    X_n[2, 0] = 0.6                               # the planted one: lb_0 = 0.5 > 0.3
    LB, UB = X_n - 0.1, X_n + 0.1
    rows, seeds = c["rows"][:5], c["seeds"][:5]
    one = ideal_single(rows[2], c["roles"], k, X_n[2], LB[2], UB[2], budget, seeds[2], lin=lin)
    assert one[3]["found"] == 0 and one[3]["refined"] == 0 and one[3]["evals_ideal"] > 0
    assert np.array_equal(_bits(one[0]), _bits(one[2])) and np.array_equal(_bits(one[1]), _bits(np.tile(X_n[2], (k, 1))))
    got = ideal_batch(rows, c["roles"], k, X_n, LB, UB, budget, seeds, lin=lin)
    assert_identical(tuple(a[2:3] for a in got[:3]) + ([got[3][2]],), tuple(a[None] for a in one[:3]) + ([one[3]],), "planted")
    keep = [0, 1, 3, 4]
    without = ideal_batch([rows[p] for p in keep], c["roles"], k, X_n[keep], LB[keep], UB[keep], budget, [seeds[p] for p in keep], lin=lin)
    assert_identical(tuple(a[keep] for a in got[:3]) + ([got[3][p] for p in keep],), without, "clean starts beside it")
    assert all(i["found"] == 3 for i in without[3])
    assert np.all(without[1][:, :, 0] <= 0.3)


def test_refusals_and_return_codes():
    d, n, k = SHAPES[0]
    c = case(d, n, k)
    ns = 5
    rows = c["rows"][:ns]
    ctx = rows[0][0].ctx
    lib = ctx.lib
    opts = _opts(200)
    prob, keep = _problem(rows, c["roles"], k, None, -1.0, False)
    hs = keep[0]
    X_n, LB, UB = [np.ascontiguousarray(c[key][:ns]) for key in ("X_n", "LB", "UB")]
    outs = [np.full((ns, k), 7.0), np.full((ns, k, d), 7.0), np.full((ns, k), 7.0)]
    infos = (_lib.IdealInfo * ns)()
    ctypes.memset(infos, 0x55, ctypes.sizeof(infos))
    ms = ctypes.c_float(7.0)
    P = _lib.as_ptr

    def call(n_starts=ns, prob=prob, hs=hs, x=X_n, lb=LB, ub=UB, opts=opts, ideal=outs[0], infos=infos):
        return lib.mrbf_ideal_point_batch(ctx.h, n_starts, None if prob is None else ctypes.byref(prob), hs, P(x), P(lb), P(ub),
                                          None if opts is None else ctypes.byref(opts), None, P(ideal), P(outs[1]), P(outs[2]), infos,
                                          ctypes.byref(ms))

    assert call(prob=None) == -3 and call(hs=None) == -4 and call(x=None) == -5 and call(lb=None) == -6 and call(ub=None) == -7
    assert call(opts=None) == -8 and call(ideal=None) == -9 and call(infos=None) == -10
    assert call(lb=UB + 1.0) == -6                                              # an empty box
    for bad in (0, -3, 65536, 1 << 40):                                         # the table refuses the start count
        assert call(n_starts=bad) == -2
        assert lib.mrbf_dispatch_after(_lib.ENTRY_IDEAL_BATCH, -2) == 1
    assert call(prob=_problem(rows, [0, 1], k, (None, None, np.zeros((257, d)), np.ones(257)), -1.0, False)[0]) == -2   # 257 linear rows
    assert call(prob=_problem(rows, [0, -7], k, None, -1.0, False)[0]) == -3    # no role
    assert call(prob=_problem(rows, [0, 0], k, None, -1.0, False)[0]) == -3     # objective 1 is no model's output
    norows = _problem(rows, [0, 1], k, None, -1.0, False)[0]
    norows.n_lin_ineq = 2                                                       # linear rows announced, none given
    assert call(prob=norows) == -3
    C = np.random.default_rng(3).random((30, d))
    other = pkg.update_model(pkg.RbfConfig(kernel="cubic"), C, _fun(C, 1))      # one output: does not share the shape
    _OWN.append(other)
    assert call(hs=_problem(rows[:2] + [[other]] + rows[3:], [0, 1], k, None, -1.0, False)[1][0]) == -4
    assert call(hs=(ctypes.c_void_p * ns)(*[_handle(r[0]) if p != 3 else None for p, r in enumerate(rows)])) == -4
    # the single call: its own codes
    sprob = _problem([rows[0]], c["roles"], k, None, -1.0, True)
    info = _lib.IdealInfo()
    ctypes.memset(ctypes.byref(info), 0x55, ctypes.sizeof(info))

    def single(prob=sprob[0], x=X_n[0], lb=LB[0], ub=UB[0], opts=opts, ideal=outs[0][0], info=info):
        return lib.mrbf_ideal_point_problem(ctx.h, None if prob is None else ctypes.byref(prob), P(x), P(lb), P(ub),
                                            None if opts is None else ctypes.byref(opts), P(ideal), P(outs[1][0]), P(outs[2][0]),
                                            None if info is None else ctypes.byref(info))

    assert single(prob=None) == -3 and single(prob=_problem([rows[0]], c["roles"], k, None, -1.0, False)[0]) == -3
    assert single(x=None) == -5 and single(lb=None) == -6 and single(ub=None) == -7 and single(opts=None) == -8 and single(ideal=None) == -9
    assert single(info=None) == -10 and single(lb=UB[0] + 1.0) == -6
    # nothing was written by any of these
    assert all(np.all(o == 7.0) for o in outs) and ms.value == 7.0
    assert bytes(infos) == b"\x55" * ctypes.sizeof(infos) and bytes(info) == b"\x55" * ctypes.sizeof(info)
    # a second identical call allocates nothing and returns the same bits
    assert call() == 0
    before = ctx.get_option(_lib.OPT_ARENA_BYTES)
    first = [o.copy() for o in outs]
    assert call() == 0
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) == before
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, outs))


def test_shapes_the_table_refuses_fall_back():
    """d = 257 in the batch and k = 9 give -2 with the outputs untouched; the binding takes the loop of single calls (d = 257 is
    inside the single call's range) and the host search (k = 9)"""
    rng = np.random.default_rng(5)
    cfg = descent.DirectedSearchConfig(max_ideal_point_problem_evals=200)
    for d, n, k, path in ((257, 300, 2, "loop"), (3, 40, 9, "reference")):
        ns = 2
        mods = []
        for p in range(ns):
            C = rng.random((n, d))
            Y = np.stack([np.sum((C - 0.1 * (l + 1)) ** 2, axis=1) for l in range(k)], axis=1)
            mods.append(pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, Y))
        _OWN.extend(mods)
        ctx = mods[0].ctx
        X_n = rng.uniform(0.3, 0.7, (ns, d))
        LB, UB = X_n - 0.1, X_n + 0.1
        prob, keep = _problem([[m] for m in mods], list(range(k)), k, None, -1.0, False)
        outs = [np.full((ns, k), 7.0), np.full((ns, k, d), 7.0), np.full((ns, k), 7.0)]
        infos = (_lib.IdealInfo * ns)()
        ctypes.memset(infos, 0x55, ctypes.sizeof(infos))
        opts = _opts(200)
        P = _lib.as_ptr
        rc = ctx.lib.mrbf_ideal_point_batch(ctx.h, ns, ctypes.byref(prob), keep[0], P(X_n), P(LB), P(UB), ctypes.byref(opts), None,
                                            P(outs[0]), P(outs[1]), P(outs[2]), infos, None)
        assert rc == -2 and ctx.lib.mrbf_dispatch_after(_lib.ENTRY_IDEAL_BATCH, rc) == 1
        assert all(np.all(o == 7.0) for o in outs) and bytes(infos) == b"\x55" * ctypes.sizeof(infos)
        if k == 9:
            sprob = _problem([[mods[0]]], list(range(k)), k, None, -1.0, True)
            info = _lib.IdealInfo()
            rc = ctx.lib.mrbf_ideal_point_problem(ctx.h, ctypes.byref(sprob[0]), P(X_n[0]), P(LB[0]), P(UB[0]), ctypes.byref(opts),
                                                  P(outs[0][0]), None, None, ctypes.byref(info))
            assert rc == -2 and ctx.lib.mrbf_dispatch_after(_lib.ENTRY_IDEAL, rc) == 1 and np.all(outs[0] == 7.0)
        scs = [sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, list(range(k)))]) for m in mods]
        stats = {}
        with batch_from(2):               # so that the table is what decides
            ideal = ps.compute_local_ideal_points_many(cfg, scs, X_n, LB, UB, seeds=[1, 2], stats=stats)
        assert stats["path"] == path and ideal.shape == (ns, k)
        mx = np.stack([_eval(mods[p], X_n[p])[0] for p in range(ns)])
        assert np.all(ideal <= mx + 1e-10 * (1.0 + np.abs(mx)))
        if path == "loop":
            one = ideal_single([mods[1]], list(range(k)), k, X_n[1], LB[1], UB[1], 200, 2)
            assert np.array_equal(_bits(ideal[1]), _bits(one[0]))


# ---- directed search with the default image direction through the device calls
def _ds_case():
    if "ds" not in _CASES:
        d, n, k, ns = 7, 40, 2, 5
        rng = np.random.default_rng(77)
        rows = []
        for p in range(ns):
            C = rng.random((n, d))
            rows.append([pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, _fun(C, k))])
        X_n = rng.uniform(0.3, 0.7, (ns, d))
        X = np.clip(X_n + rng.uniform(-0.02, 0.02, (ns, d)), 0.0, 1.0)
        _CASES["ds"] = dict(rows=rows, X=X, X_n=X_n, deltas=rng.uniform(0.1, 0.2, ns), lb=np.zeros(d), ub=np.ones(d), seeds=[3, 1, 4, 1, 5],
                            FX_n=np.stack([_eval(rows[p][0], X_n[p])[0] for p in range(ns)]) + 0.01)
    return _CASES["ds"]


def test_ds_iterate_many_with_the_device_ideal_points():
    c = _ds_case()
    ns = len(c["rows"])
    scs = [sg.SurrogateContainer(objectives=[sg.RefSurrogate(row[0], [0, 1])]) for row in c["rows"]]
    cfg = descent.DirectedSearchConfig(ideal_point="device", max_ideal_point_problem_evals=4 * 20 * 8)
    X, X_n, FX_n, deltas, lb, ub = c["X"], c["X_n"], c["FX_n"], c["deltas"], c["lb"], c["ub"]
    stats = {}
    res = descent.ds_iterate_many(cfg, scs, None, X, X_n, FX_n, deltas, lb, ub, stats=stats, seeds=c["seeds"])
    assert stats["path"] == "batch" and stats["ideal_point_path"] == "device" and stats["image_direction"] == "ideal_point"
    own_rule = "batch" if ns >= ps.IDEAL_BATCH_MIN_STARTS else "loop"          # how the ideal points were found: the measured rule
    assert stats["ideal_point_stats"]["path"] == own_rule and stats["rerouted"] == []
    # with the batch admitted at this count: two device calls, and the same bits (contract B)
    with batch_from(2):
        stats2 = {}
        res2 = descent.ds_iterate_many(cfg, scs, None, X, X_n, FX_n, deltas, lb, ub, stats=stats2, seeds=c["seeds"])
    assert stats2["path"] == "batch" and stats2["ideal_point_path"] == "device" and stats2["ideal_point_stats"]["path"] == "batch"
    for a, b in zip(res, res2):
        assert a[0] == b[0] and a[4] == b[4] and all(np.array_equal(_bits(a[i]), _bits(b[i])) for i in (1, 2, 3))
    # chained by hand: the ideal points of all starts, R = ideal - FX_n, the one batch call
    boxes = [descent._local_bounds(X[p], cfg.reference_trust_region_factor * float(deltas[p]), lb, ub) for p in range(ns)]
    LB, UB = np.stack([b[0] for b in boxes]), np.stack([b[1] for b in boxes])
    st = {}
    with batch_from(2):
        ideal = ps.compute_local_ideal_points_many(cfg, scs, X_n, LB, UB, seeds=c["seeds"], carry_constraints=False, stats=st)
    assert st["path"] == "batch"
    R = ideal - FX_n
    plans = [sg.container_plan(sc) for sc in scs]
    rc, dd, xp, mxp, mu, records, ms = descent.ds_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, R)
    assert rc == 0
    for p in range(ns):
        om, d_, x_plus, mx_plus, nrm = res[p]
        r = records[p]
        assert r["ds_status"] == _lib.DS_OK and r["sigma"] > cfg.min_stepsize, r
        assert om == r["omega_step"] and nrm == r["step_norm"]
        assert np.array_equal(_bits(d_), _bits(dd[p])) and np.array_equal(_bits(x_plus), _bits(xp[p])) and np.array_equal(_bits(mx_plus), _bits(mxp[p]))
        assert stats["records"][p] == r
        # m(x+) satisfies the Armijo condition of its record: the accepted step is sigma shrunk `loops` times
        step = r["sigma"]
        for _ in range(r["loops"]):
            step *= cfg.armijo_const_shrink
        assert r["loops"] < cfg.max_loops
        m_xn = _eval(c["rows"][p][0], X_n[p])[0]
        assert descent._armijo_condition(cfg.strict_backtracking, m_xn, mx_plus, step, r["omega_step"], cfg.armijo_const_rhs), (p, r, m_xn, mx_plus)
    # every start's ideal point is the single call's (contract B through the bindings)
    for p in (0, 4):
        one = ideal_single(c["rows"][p], [0, 1], 2, X_n[p], LB[p], UB[p], cfg.max_ideal_point_problem_evals, c["seeds"][p])
        assert np.array_equal(_bits(one[0]), _bits(ideal[p]))
    # a container with one linear inequality: the loop of single-start functions, the ideal points still from the device in one call
    A = np.zeros((1, 7))
    A[0, 0] = 1.0
    stats = {}
    res_lin = descent.ds_iterate_many(cfg, scs, None, X, X_n, FX_n, deltas, lb, ub, lin=(None, None, A, np.array([2.0])), stats=stats,
                                      seeds=c["seeds"])
    assert stats["path"] == "loop" and stats["ideal_point_path"] == "device" and stats["ideal_point_stats"]["path"] == own_rule
    assert len(res_lin) == ns and all(np.all(np.isfinite(r_[2])) for r_ in res_lin)


def test_get_criticality_ds_with_the_device_ideal_point():
    c = _ds_case()
    p = 1
    sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(c["rows"][p][0], [0, 1])])
    cfg = descent.DirectedSearchConfig(ideal_point="device", max_ideal_point_problem_evals=4 * 20 * 8)
    x, x_n, fx_n, delta, lb, ub = c["X"][p], c["X_n"][p], c["FX_n"][p], float(c["deltas"][p]), c["lb"], c["ub"]
    stats = {}
    omega, dn = descent.get_criticality_ds(cfg, sc, None, x, x_n, fx_n, delta, lb, ub, stats=stats, seed=9)
    assert stats["path"] == "device" and stats["ideal_point_path"] == "device"
    lb_eff, ub_eff = descent._local_bounds(x, cfg.reference_trust_region_factor * delta, lb, ub)
    plan = sg.container_plan(sc)
    rc, ideal, x_ideal, mx, info = ps.ideal_point_problem_device(cfg, plan, x_n, lb_eff, ub_eff, seed=9, carry_constraints=False)
    assert rc == 0 and info["found"] == 3
    rc, om, dd, qinfo = descent.ds_criticality_device(plan, x_n, lb, ub, ideal - fx_n)
    assert rc == 0
    om_ref, d_ref = descent._ds_normalise(om, dd, qinfo["status"], x_n.size)
    assert omega == om_ref and np.array_equal(_bits(dn), _bits(d_ref)) and omega > 0
    # a precomputed image direction is taken as it is
    omega2, dn2 = descent.get_criticality_ds(cfg, sc, None, x, x_n, fx_n, delta, lb, ub, r=ideal - fx_n)
    assert omega2 == omega and np.array_equal(_bits(dn2), _bits(dn))
    # the default configuration keeps the host search
    stats = {}
    descent.get_criticality_ds(descent.DirectedSearchConfig(max_ideal_point_problem_evals=200), sc, None, x, x_n, fx_n, delta, lb, ub, stats=stats)
    assert stats["ideal_point_path"] == "reference" and "ideal_point_calls" in stats
