"""Many-start Pascoletti-Serafini step on the device (run with -m gpu): mrbf_ps_step_batch against a loop of mrbf_ps_step_problem on
the same context.  Bit identity is the contract: every output array compared as uint64 words, every info field except ms_total.
Budgets are small (about six generations per run, so the reserve for gradient steps is non-zero) -- a step is a handful of generations
plus a refinement.  Shapes, the smallest at which something different happens:
  d = 3,   n = 40    dpad 64, one centre tile; lambda = 80 / 100: the populations-in-registers ranking inside the one workgroup
  d = 50,  n = 600   lambda_ps = 1040 >= 1024 > lambda_ip = 1020: either side of the several-compute-unit ranking; ten centre tiles
  d = 65,  n = 131   dpad 128
  d = 129, n = 259   dpad 256, five tiles: the population rule of the centre-range split, two outputs per values pass"""
import ctypes

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib
    from morbit.jl_amd import pascoletti_serafini as ps
    from morbit.jl_amd import surrogates as sg

SHAPES = [(3, 40), (50, 600), (65, 131), (129, 259)]
NS = 5
INFO_FIELDS = ("status", "generations", "evals_ideal", "evals_ps", "evals_polish", "tau")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _handle(m):
    return m.model.value if hasattr(m.model, "value") else m.model


def _opts(d, polish=0, seed=1):
    lam = 20 * (d + 2)
    return _lib.PsOptions(6 * lam, 6 * lam, polish, 0, seed, -0.5, 1e-3)


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


def single_loop(rows, roles, k, X_n, LB, UB, FX, R, opts, seeds, lin=None, eq_tol=-1.0):
    """the loop of mrbf_ps_step_problem calls the batch has to reproduce"""
    ctx = rows[0][0].ctx
    ns, d = X_n.shape
    XT, MT, RO, infos = np.empty((ns, d)), np.empty((ns, k)), np.empty((ns, k)), []
    for p in range(ns):
        prob, keep = _problem([rows[p]], roles, k, lin, eq_tol, True)
        o = _lib.PsOptions(opts.max_ideal_evals, opts.max_ps_evals, opts.max_polish_evals, 0, int(seeds[p]), opts.t0, opts.xtol_rel)
        info = _lib.PsInfo()
        r = None if R is None else np.ascontiguousarray(R[p])
        rc = ctx.lib.mrbf_ps_step_problem(ctx.h, ctypes.byref(prob), _lib.as_ptr(np.ascontiguousarray(X_n[p])), _lib.as_ptr(np.ascontiguousarray(LB[p])),
                                          _lib.as_ptr(np.ascontiguousarray(UB[p])), _lib.as_ptr(np.ascontiguousarray(FX[p])), _lib.as_ptr(r),
                                          ctypes.byref(o), _lib.as_ptr(XT[p]), _lib.as_ptr(MT[p]), _lib.as_ptr(RO[p]), ctypes.byref(info))
        assert rc == 0, (p, rc, ctx.lib.mrbf_last_error(ctx.h))
        infos.append(info.asdict())
    return XT, MT, RO, infos


def batch(rows, roles, k, X_n, LB, UB, FX, R, opts, seeds, lin=None, eq_tol=-1.0, device=False, expect_rc=0):
    ctx = rows[0][0].ctx
    ns, d = X_n.shape
    prob, keep = _problem(rows, roles, k, lin, eq_tol, False)
    hs = keep[0]
    seeds_c = None if seeds is None else (ctypes.c_uint64 * ns)(*[int(s) for s in seeds])
    infos = (_lib.PsInfo * ns)()
    ms = ctypes.c_float()
    if device:
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        ins = [up(a) for a in (X_n, LB, UB, FX, R)]
        outs = [torch.empty((ns, d), dtype=torch.float64, device="cuda"), torch.empty((ns, k), dtype=torch.float64, device="cuda"),
                torch.empty((ns, k), dtype=torch.float64, device="cuda")]
        torch.cuda.synchronize()
    else:
        ins = [None if a is None else np.ascontiguousarray(a) for a in (X_n, LB, UB, FX, R)]
        outs = [np.empty((ns, d)), np.empty((ns, k)), np.empty((ns, k))]
    rc = ctx.lib.mrbf_ps_step_batch(ctx.h, ns, ctypes.byref(prob), hs, *[_lib.as_ptr(a) for a in ins], ctypes.byref(opts), seeds_c,
                                    *[_lib.as_ptr(a) for a in outs], infos, ctypes.byref(ms))
    assert rc == expect_rc, (rc, ctx.lib.mrbf_last_error(ctx.h))
    if rc != 0:
        return None
    assert ms.value > 0 and all(i.ms_total == ms.value for i in infos)
    if device:
        outs = [o.cpu().numpy() for o in outs]
    return outs[0], outs[1], outs[2], [i.asdict() for i in infos]


def assert_identical(got, ref, tag=None, rows=None):
    sel = slice(None) if rows is None else rows
    for a, b, name in zip(got[:3], ref[:3], ("x_trial", "mx_trial", "r_out")):
        assert np.array_equal(_bits(a), _bits(b[sel])), (tag, name)
    rinfos = ref[3] if rows is None else [ref[3][p] for p in rows]
    assert len(got[3]) == len(rinfos)
    for p, (a, b) in enumerate(zip(got[3], rinfos)):
        for f in INFO_FIELDS:
            assert _bits(a[f])[0] == _bits(b[f])[0] if f == "tau" else a[f] == b[f], (tag, p, f, a[f], b[f])


def f_a(C):
    return np.sum((C - 0.3) ** 2, axis=1)


def f_b(C):
    return np.sum((C - 0.7) ** 2, axis=1) + 0.1 * np.sin(3.0 * C[:, 0])


_CASES = {}


def case(d, n, ns=NS):
    """ns starts of one problem: every start its own centres, start 2 its own shape parameter, its own box and seed; fitted once"""
    key = (d, n, ns)
    if key not in _CASES:
        rng = np.random.default_rng(1000 + 7 * d + ns)
        rows = []
        for p in range(ns):
            C = rng.random((n, d))
            cfg = pkg.RbfConfig(kernel="multiquadric", shape_parameter=2.5 if p == 2 else 1.0, polynomial_degree=1)
            rows.append([pkg.update_model(cfg, C, np.stack([f_a(C), f_b(C)], axis=1))])
        X_n = 0.5 + rng.uniform(-0.1, 0.1, (ns, d))
        half = rng.uniform(0.05, 0.12, (ns, 1))
        LB, UB = X_n - half, X_n + half
        # "true" values at x_n: the models' own (2 d + 1 random sites do not pin the functions down at d >= 65, and r = fx - ideal must be
        # positive for the PS phase to run)
        FX = np.stack([pkg.eval_models_at_sites(rows[p][0], None, X_n[p][None, :])[0] for p in range(ns)])
        R = rng.uniform(0.5, 1.5, (ns, 2))
        seeds = [11 + 3 * p for p in range(ns)]
        _CASES[key] = dict(rows=rows, X_n=X_n, LB=LB, UB=UB, FX=FX, R=R, seeds=seeds, refs={})
    return _CASES[key]


def reference(c, d, given, polish):
    """the loop of single calls for a case, computed once and shared by the tests that compare with it"""
    key = (given, polish)
    if key not in c["refs"]:
        c["refs"][key] = single_loop(c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], c["R"] if given else None, _opts(d, polish), c["seeds"])
    return c["refs"][key]


@pytest.mark.parametrize("d, n", SHAPES)
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("polish", [0, 40])
def test_bit_identity_with_the_loop_of_single_calls(d, n, given, polish):
    c = case(d, n)
    ref = reference(c, d, given, polish)
    got = batch(c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], c["R"] if given else None, _opts(d, polish), c["seeds"])
    assert_identical(got, ref, (d, n, given, polish))
    assert all(i["status"] == _lib.PS_OK and -1.0 <= i["tau"] <= 0.0 and i["generations"] > 0 for i in got[3]), got[3]
    assert all((i["evals_polish"] > 0) == (polish > 0) for i in got[3]), got[3]
    assert all((i["evals_ideal"] > 0) == (not given) for i in got[3]), got[3]
    # a second identical call returns the same bits
    again = batch(c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], c["R"] if given else None, _opts(d, polish), c["seeds"])
    assert_identical(again, got, "repeat")


@pytest.mark.parametrize("d, n", SHAPES)
def test_batch_of_one_permutation_and_device_pointers(d, n):
    c = case(d, n)
    ref = reference(c, d, False, 0)
    opts = _opts(d)
    arrs = lambda idx: [c[key][idx] for key in ("X_n", "LB", "UB", "FX")]
    for p in (0, 2):
        got = batch([c["rows"][p]], [0, 1], 2, *arrs([p]), None, opts, [c["seeds"][p]])
        assert_identical(got, ref, ("one", p), rows=[p])
    perm = [3, 0, 4, 2, 1]
    got = batch([c["rows"][p] for p in perm], [0, 1], 2, *arrs(perm), None, opts, [c["seeds"][p] for p in perm])
    assert_identical(got, ref, "permutation", rows=perm)
    got = batch(c["rows"], [0, 1], 2, *arrs(slice(None)), None, opts, c["seeds"], device=True)
    assert_identical(got, ref, "device pointers")
    refg = reference(c, d, True, 0)
    got = batch(c["rows"], [0, 1], 2, *arrs(slice(None)), c["R"], opts, c["seeds"], device=True)
    assert_identical(got, refg, "device pointers, r given")


def test_seeds_null_means_the_options_seed():
    d, n = SHAPES[0]
    c = case(d, n)
    opts = _opts(d, seed=77)
    ref = single_loop(c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], None, opts, [77] * NS)
    got = batch(c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], None, opts, None)
    assert_identical(got, ref, "seeds NULL")


@pytest.mark.parametrize("d, n", [SHAPES[0], SHAPES[2]])
def test_a_critical_start_beside_others(d, n):
    c = case(d, n)
    R = c["R"].copy()
    R[1, 0] = 0.0          # not positive: start 1 is critical
    R[3, 1] = -0.25
    opts = _opts(d)
    ref = single_loop(c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], R, opts, c["seeds"])
    got = batch(c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], R, opts, c["seeds"])
    assert_identical(got, ref, "critical")
    for p in (1, 3):
        info = got[3][p]
        assert info["status"] == _lib.PS_CRITICAL and info["tau"] == 0.0 and info["evals_ps"] == 0 and info["generations"] == 0
        assert np.array_equal(got[0][p], c["X_n"][p])
        m = c["rows"][p][0]
        assert np.allclose(got[1][p], pkg.eval_models_at_sites(m, None, c["X_n"][p][None, :])[0], rtol=0.0, atol=1e-13)     # m(x_n)
    # the others are what they are without the critical starts beside them
    keep = [0, 2, 4]
    refg = reference(c, d, True, 0)
    assert_identical(tuple(a[keep] for a in got[:3]) + ([got[3][p] for p in keep],), refg, "others unaffected", rows=keep)


def test_ranking_rule_by_the_launch_total():
    """18 starts at d = 50: the PS phase has 18 runs of lambda = 1040 -- more than the residency rule admits to the several-compute-unit
    ranking (16 compute units per run), so every run is ranked by one workgroup; the same starts in batches of six take the wave
    kernel, as the single calls do.  All three agree."""
    d, n, ns = 50, 600, 18
    c = case(d, n, ns)
    opts = _opts(d)
    args = lambda idx: ([c["rows"][p] for p in idx], [0, 1], 2, c["X_n"][idx], c["LB"][idx], c["UB"][idx], c["FX"][idx], c["R"][idx], opts,
                        [c["seeds"][p] for p in idx])
    allp = list(range(ns))
    ref = single_loop(*args(allp))
    assert_identical(batch(*args(allp)), ref, "18 starts")
    for lo in range(0, ns, 6):
        idx = list(range(lo, lo + 6))
        assert_identical(batch(*args(idx)), ref, ("six", lo), rows=idx)
    assert all(i["status"] == _lib.PS_OK for i in ref[3])


def test_container_with_two_models_constraints_and_linear_rows():
    """objectives from two grouped models, a modelled inequality and a modelled equality (rows of the first model), linear rows of the
    MOP: the score launch of its own (linear rows), several models per start"""
    rng = np.random.default_rng(12)
    d, n, ns = 12, 300, 4
    rows = []
    for p in range(ns):
        C = rng.random((n + 10 * p, d))
        Ya = np.stack([np.sum((C - 0.3) ** 2, axis=1), C[:, 0] - 0.52, C[:, 2] - C[:, 4]], axis=1)     # objective 0 | g(x) <= 0 | h(x) = 0
        Yb = np.sum((C - 0.7) ** 2, axis=1, keepdims=True)                                               # objective 1
        rows.append([pkg.update_model(pkg.RbfConfig(kernel="cubic"), C, Ya), pkg.update_model(pkg.RbfConfig(kernel="multiquadric"), C, Yb)])
    roles = [0, _lib.ROLE_INEQ, _lib.ROLE_EQ, 1]
    X_n = np.tile(np.array([0.5, 0.85, 0.4, 0.2, 0.4, 0.5] * 2), (ns, 1)) + rng.uniform(-0.01, 0.01, (ns, d))
    X_n[:, 4] = X_n[:, 2]
    LB, UB = X_n - 0.12, X_n + 0.12
    A = np.zeros((1, d))
    A[0, 1] = A[0, 3] = 1.0
    lin = (None, None, A, np.array([1.1]))
    FX = np.stack([np.sum((X_n - 0.3) ** 2, axis=1), np.sum((X_n - 0.7) ** 2, axis=1)], axis=1)
    seeds = [5, 6, 7, 8]
    for given, polish in ((False, 0), (True, 30)):
        R = np.full((ns, 2), 1.0) if given else None
        opts = _opts(d, polish)
        ref = single_loop(rows, roles, 2, X_n, LB, UB, FX, R, opts, seeds, lin=lin, eq_tol=0.02)
        got = batch(rows, roles, 2, X_n, LB, UB, FX, R, opts, seeds, lin=lin, eq_tol=0.02)
        assert_identical(got, ref, ("container", given, polish))
    for row in rows:
        for m in row:
            m.free()


def test_starts_in_split_and_unsplit_groups():
    """n = 40 (one centre tile: unsplit) beside n = 300 (five tiles under a small query batch: one tile per workgroup + the combine
    pass): members of one model slot fall into different launch groups, and every start still reproduces its own single call"""
    d = 3
    rng = np.random.default_rng(91)
    rows = []
    for n in (40, 300, 40, 300, 57):
        C = rng.random((n, d))
        rows.append([pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, np.stack([f_a(C), f_b(C)], axis=1))])
    c = case(*SHAPES[0])
    for given in (False, True):
        args = (rows, [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], c["R"] if given else None, _opts(d, 26), c["seeds"])
        assert_identical(batch(*args), single_loop(*args), ("split / unsplit", given))
    for row in rows:
        row[0].free()


def test_return_codes_and_arena():
    d, n = SHAPES[0]
    c = case(d, n)
    ctx = c["rows"][0][0].ctx
    opts = _opts(d)
    prob, keep = _problem(c["rows"], [0, 1], 2, None, -1.0, False)
    hs = keep[0]
    xt, mt, ro = np.empty((NS, d)), np.empty((NS, 2)), np.empty((NS, 2))
    infos = (_lib.PsInfo * NS)()
    P = _lib.as_ptr

    def call(ns=NS, prob=prob, hs=hs, x=c["X_n"], lb=c["LB"], ub=c["UB"], fx=c["FX"], r=None, opts=opts, xt=xt, mt=mt, infos=infos):
        return ctx.lib.mrbf_ps_step_batch(ctx.h, ns, None if prob is None else ctypes.byref(prob), hs, P(x), P(lb), P(ub), P(fx), P(r),
                                          None if opts is None else ctypes.byref(opts), None, P(xt), P(mt), P(ro), infos, None)

    assert ctx.lib.mrbf_ps_step_batch(None, NS, ctypes.byref(prob), hs, P(c["X_n"]), P(c["LB"]), P(c["UB"]), P(c["FX"]), None, ctypes.byref(opts),
                                      None, P(xt), P(mt), P(ro), infos, None) == -1
    assert call(prob=None) == -3 and call(hs=None) == -4 and call(x=None) == -5 and call(lb=None) == -6 and call(ub=None) == -7
    assert call(fx=None) == -8 and call(fx=None, r=c["R"]) == 0 and call(opts=None) == -10 and call(xt=None) == -12 and call(mt=None) == -13
    assert call(infos=None) == -15
    assert call(opts=_lib.PsOptions(-1, -1, 0, 0, 1, 0.5, 1e-3)) == -10         # t0 outside [-1, 0]
    assert call(lb=c["UB"] + 1.0) == -6                                         # an empty box
    assert call(ns=0) == -2                                                     # the table refuses: no start
    many = _problem(c["rows"], [0, 1], 2, (None, None, np.zeros((257, d)), np.ones(257)), -1.0, False)
    assert call(prob=many[0]) == -2                                             # 257 linear rows: outside the device path
    assert ctx.lib.mrbf_dispatch_after(_lib.ENTRY_PS_BATCH, -2) == 1
    bad_role = _problem(c["rows"], [0, -7], 2, None, -1.0, False)
    assert call(prob=bad_role[0]) == -3
    twice = _problem(c["rows"], [0, 0], 2, None, -1.0, False)
    assert call(prob=twice[0]) == -3                                            # objective 1 is no model's output
    C = np.random.default_rng(3).random((30, d))
    other = pkg.update_model(pkg.RbfConfig(kernel="cubic"), C, f_a(C)[:, None])  # one output: does not share the shape
    mixed = _problem(c["rows"][:2] + [[other]] + c["rows"][3:], [0, 1], 2, None, -1.0, False)
    assert call(hs=mixed[1][0]) == -4
    hs_null = (ctypes.c_void_p * NS)(*[_handle(r[0]) if p != 3 else None for p, r in enumerate(c["rows"])])
    assert call(hs=hs_null) == -4
    other.free()
    # a second identical call allocates nothing
    assert call() == 0
    before = ctx.get_option(_lib.OPT_ARENA_BYTES)
    first = (xt.copy(), mt.copy(), ro.copy())
    assert call() == 0
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) == before
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, (xt, mt, ro)))


@pytest.mark.parametrize("d, n", [SHAPES[0], SHAPES[2]])
def test_a_batch_processed_in_chunks_of_starts(d, n):
    """a batch whose state exceeds the limit (2 GiB; MRBF_PS_CHUNK_KB sets another one) is processed in chunks of starts inside the
    call: with 1 KiB every start is a chunk of its own, with the second limit the five starts go in chunks of two or three (a start
    takes about 160 KiB at d = 3 and 3 MiB at d = 65).  Same bits, and every info carries the whole call's event time."""
    import os

    c = case(d, n)
    ref = reference(c, d, False, 0)
    args = (c["rows"], [0, 1], 2, c["X_n"], c["LB"], c["UB"], c["FX"], None, _opts(d), c["seeds"])
    keep = os.environ.get("MRBF_PS_CHUNK_KB")
    try:
        for kb in (1, 400 if d == 3 else 8000):
            os.environ["MRBF_PS_CHUNK_KB"] = str(kb)
            assert_identical(batch(*args), ref, ("chunks", kb))
    finally:
        if keep is None:
            os.environ.pop("MRBF_PS_CHUNK_KB", None)
        else:
            os.environ["MRBF_PS_CHUNK_KB"] = keep


def test_python_get_criticality_many_equals_the_loop():
    d, n = SHAPES[2]
    c = case(d, n)
    R = sg.RefSurrogate
    scs = [sg.SurrogateContainer(objectives=[R(row[0], [0, 1])]) for row in c["rows"]]
    lam = 20 * (d + 2)
    for cfg in (ps.PascolettiSerafiniConfig(max_ps_problem_evals=6 * lam, max_ideal_point_problem_evals=6 * lam),
                ps.PascolettiSerafiniConfig(max_ps_problem_evals=6 * lam, reference_point=[-1.0, -1.0], ps_polish_algo="LD_MMA", max_ps_polish_evals=30)):
        X = c["X_n"] + 0.01
        stats = {}
        many = ps.get_criticality_many(cfg, scs, None, X, c["X_n"], c["FX"], c["LB"], c["UB"], seeds=c["seeds"], stats=stats)
        assert stats["path"] == "batch" and len(stats["infos"]) == NS
        for p in range(NS):
            st = {}
            one = ps.get_criticality_container(cfg, scs[p], None, X[p], c["X_n"][p], c["FX"][p], c["LB"][p], c["UB"][p], seed=c["seeds"][p], stats=st)
            assert st["path"] == "device"
            omega, (xt, mt, sl) = one
            omega_m, (xt_m, mt_m, sl_m) = many[p]
            assert omega == omega_m and sl == sl_m and np.array_equal(_bits(xt), _bits(xt_m)) and np.array_equal(_bits(mt), _bits(mt_m))
            assert np.array_equal(_bits(st["r"]), _bits(stats["r"][p]))
        loop_stats = {}
        keep_rule = ps.PS_BATCH_MIN_STARTS
        ps.PS_BATCH_MIN_STARTS = NS + 1          # below the rule: the loop of single calls
        try:
            loop = ps.get_criticality_many(cfg, scs, None, X, c["X_n"], c["FX"], c["LB"], c["UB"], seeds=c["seeds"], stats=loop_stats)
        finally:
            ps.PS_BATCH_MIN_STARTS = keep_rule
        assert loop_stats["path"] == "loop"
        for a, b in zip(loop, many):
            assert a[0] == b[0] and np.array_equal(_bits(a[1][0]), _bits(b[1][0]))
