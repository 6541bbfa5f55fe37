"""The many-start model update on the device (run with -m gpu): mrbf_fit_batch against mrbf_fit per start.  Bit identity is the
contract: weights, tail coefficients, values and Jacobians of mrbf_eval and the outputs of mrbf_sd_iterate_batch with np.array_equal,
path / fallbacks / n / q with ==.  The residual and max |Pi' w| come from the batch's own check kernel (sums in another order) and
meet the bounds tests/test_gpu_configs.py::test_c4_many_start_batch uses.  Shapes: (n, d) = (20, 3), (129, 3), (257, 65), (140, 65)
-- dpad 64 and 128, npad 128, 256 and 384, odd row lengths: the smallest at which the shared kernels and the per-start offsets into
the call's one allocation can go wrong."""
import ctypes

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg

SHAPES = [(20, 3), (129, 3), (257, 65), (140, 65)]
# kernel, polynomial degree (the shape parameter is the package default: gaussian alpha = 1 on sites spread over [-2, 2]^d, the
# bounded-conditioning setting of tests/test_gpu_sd_step.py and tests/test_gpu_sd_batch.py)
KERNELS = [("cubic", 1), ("multiquadric", 0), ("gaussian", -1)]
INFO_EQUAL = ("path", "fallbacks", "n", "q")
M_QUERIES = 70


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


def _data(n, d, k, seed):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-2.0, 2.0, (n, d))
    Y = np.stack([np.sum((C - 1.0) ** 2, axis=1), np.sum((C + 1.0) ** 2, axis=1) + C[:, 0]], axis=1)[:, :k]
    return C, np.ascontiguousarray(Y)


def _spec(kernel, deg, n, d, k, seed, shape_parameter=float("nan")):
    cfg = pkg.RbfConfig(kernel=kernel, shape_parameter=shape_parameter, polynomial_degree=deg)
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, cfg)
    C, Y = _data(n, d, k, seed)
    return dict(C=C, Y=Y, kid=kid, a=a, b=b, deg=deg)


def _q(d, deg):
    return 0 if deg < 0 else (1 if deg == 0 else d + 1)


def single(ctx, s):
    """mrbf_fit on one start: (status, RbfModel or None)"""
    n, d = s["C"].shape
    k, q = s["Y"].shape[1], _q(s["C"].shape[1], s["deg"])
    W, L = np.full((n, k), np.nan), np.full((max(q, 1), k), np.nan)
    h, info = _lib.c_vp(), _lib.FitInfo()
    rc = ctx.lib.mrbf_fit(ctx.h, n, d, k, _lib.as_ptr(s["C"]), _lib.as_ptr(s["Y"]), s["kid"], s["a"], s["b"], s["deg"], ctypes.byref(h),
                          _lib.as_ptr(W), _lib.as_ptr(L), ctypes.byref(info))
    return rc, (pkg.RbfModel(ctx, h, n, d, k, q, False, W, L[:q], info.asdict()) if rc == 0 else None)


def batch(ctx, specs, expect_rc=0):
    """one mrbf_fit_batch call on host arrays: [(status, RbfModel or None)] in start order"""
    ns = len(specs)
    jobs = (_lib.FitJob * ns)()
    outs = []
    for p, s in enumerate(specs):
        n, d = s["C"].shape
        k, q = s["Y"].shape[1], _q(d, s["deg"])
        W, L = np.full((n, k), np.nan), np.full((max(q, 1), k), np.nan)
        outs.append((n, d, k, q, W, L))
        J = jobs[p]
        J.n, J.d, J.k, J.kernel_id, J.poly_deg, J.a, J.b = n, d, k, s["kid"], s["deg"], s["a"], s["b"]
        J.centres, J.values, J.weights_out, J.poly_out = _lib.as_ptr(s["C"]), _lib.as_ptr(s["Y"]), _lib.as_ptr(W), _lib.as_ptr(L)
    ms = ctypes.c_float(-1.0)
    rc = ctx.lib.mrbf_fit_batch(ctx.h, ns, jobs, ctypes.byref(ms))
    assert rc == expect_rc, (rc, ctx.lib.mrbf_last_error(ctx.h))
    res = []
    for p, (n, d, k, q, W, L) in enumerate(outs):
        J = jobs[p]
        assert (J.model is None) == (J.status != 0), (p, J.status, J.model)
        res.append((int(J.status), pkg.RbfModel(ctx, _lib.c_vp(J.model), n, d, k, q, False, W, L[:q], J.info.asdict()) if J.status == 0 else None))
    return res


def _queries(d, seed=4242):
    return np.random.default_rng(seed + d).uniform(-2.0, 2.0, (M_QUERIES, d))


def assert_same_model(got, ref, tag, well_conditioned=None):
    """`got` (from the batch) against `ref` (from mrbf_fit): (status, model) pairs"""
    (gs, gm), (rs, rm_) = got, ref
    assert gs == rs, (tag, gs, rs)
    if rs != 0:
        return
    assert np.array_equal(gm.weights, rm_.weights), tag
    assert np.array_equal(gm.poly, rm_.poly), tag
    X = _queries(gm.d)
    gV, gJ = gm.eval_sites(X, want_values=True, want_jac=True)
    rV, rJ = rm_.eval_sites(X, want_values=True, want_jac=True)
    assert np.array_equal(gV, rV) and np.array_equal(gJ, rJ), tag
    for f in INFO_EQUAL:
        assert gm.info[f] == rm_.info[f], (tag, f, gm.info, rm_.info)
    print(tag, "rel_residual batch %.3e single %.3e  max_pitw batch %.3e single %.3e" %
          (gm.info["rel_residual"], rm_.info["rel_residual"], gm.info["max_pitw"], rm_.info["max_pitw"]))
    if well_conditioned is None:
        well_conditioned = rm_.info["rel_residual"] < 1e-11        # judged by the single call's own residual
    if well_conditioned and rm_.info["path"] != _lib.PATH_LU:
        assert gm.info["rel_residual"] < 1e-11, (tag, gm.info)
        if gm.q:
            assert gm.info["max_pitw"] < 1e-11 * max(1.0, np.abs(gm.weights).max()), (tag, gm.info)


def _free(pairs):
    for _, m in pairs:
        if m is not None:
            m.free()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("kernel,deg", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_bit_identity_with_mrbf_fit(ctx, n, d, kernel, deg, k):
    specs = [_spec(kernel, deg, n, d, k, seed=1000 * n + 10 * d + p) for p in range(9)]
    refs = [single(ctx, s) for s in specs]
    assert all(rc == 0 for rc, _ in refs)
    wc = None if kernel == "gaussian" else True
    for members in (range(9), range(5), [3]):
        got = batch(ctx, [specs[p] for p in members])
        for g, p in zip(got, members):
            assert_same_model(g, refs[p], (n, d, kernel, k, len(got), p), well_conditioned=wc)
        _free(got)
    _free(refs)


def _mixed_specs():
    d = 3
    return [_spec("cubic", 1, 40, d, 2, 1), _spec("multiquadric", 1, 57, d, 2, 2), _spec("multiquadric", 1, 40, d, 2, 3, shape_parameter=2.5),
            _spec("cubic", 1, 600, d, 2, 4),                           # beyond the one-launch range: the single call inside the batch
            _spec("gaussian", -1, 129, d, 1, 5), _spec("inv_multiquadric", 0, 300, d, 2, 6), _spec("cubic", 1, 90, 65, 1, 7)]


def test_mixed_batch(ctx):
    specs = _mixed_specs()
    refs = [single(ctx, s) for s in specs]
    got = batch(ctx, specs)
    for p, (g, r) in enumerate(zip(got, refs)):
        assert_same_model(g, r, ("mixed", p))
    assert refs[3][0] == 0 and got[3][1].info["path"] == refs[3][1].info["path"] and got[3][1].n == 600
    _free(got), _free(refs)


def test_position_independence(ctx):
    specs = _mixed_specs()
    a = batch(ctx, specs)
    perm = [4, 0, 6, 2, 5, 1, 3]
    b = batch(ctx, [specs[i] for i in perm])
    for j, i in enumerate(perm):
        assert_same_model(b[j], a[i], ("permuted", j, i), well_conditioned=False)
    _free(a), _free(b)


def test_golden_cases_in_one_batch(ctx, golden):
    """every committed fixture case as one batch: mixed kernels (general exponents among them), tails, dimensions, n < q (minimum
    norm), and the ill-conditioned ones -- any start that the single fit sends to a fallback is flagged in the batch as well, takes
    mrbf_fit inside the call and must match, without disturbing its neighbours"""
    specs = [dict(C=np.ascontiguousarray(c["C"], dtype=np.float64), Y=np.ascontiguousarray(c["Y"], dtype=np.float64).reshape(c["C"].shape[0], -1),
                  kid=c["kid"], a=c["a"], b=c["b"], deg=c["deg"]) for c in golden]
    refs = [single(ctx, s) for s in specs]
    got = batch(ctx, specs)
    flagged = [c["name"] for c, (rc, m) in zip(golden, refs) if rc == 0 and m.info["fallbacks"] != 0 and m.n <= 512]
    print("fixture cases whose single fit reports a fallback at n <= 512:", flagged)
    for c, g, r in zip(golden, got, refs):
        assert_same_model(g, r, ("golden", c["name"]), well_conditioned=False)
    # DESIGN.md section 12 says that no existing input sends a fit with n <= 512 to its fallback path, i.e. that the flagged-start route
    # (slab share skipped, mrbf_fit inside the call) has no case of its own: if a fixture case ever does, it has just been compared
    # above, and that sentence and this assertion are to be replaced by a test that names the case
    assert flagged == [], flagged
    _free(got), _free(refs)


@pytest.mark.parametrize("d", [3, 65])
def test_models_hand_on_to_the_batched_descent(ctx, d):
    ns, n = 5, max(40, 2 * d + 20)
    specs = [_spec("multiquadric", 1, n + 3 * p, d, 2, seed=300 + 7 * d + p) for p in range(ns)]
    refs = [single(ctx, s) for s in specs]
    got = batch(ctx, specs)
    rng = np.random.default_rng(55 + d)
    X = rng.uniform(-1.0, 1.0, (ns, d))
    X_n = X + rng.uniform(-0.02, 0.02, (ns, d))
    deltas = np.array([0.3, 0.25, 0.4, 0.35, 0.3])
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    cfg = descent.SteepestDescentConfig()
    out = []
    for pairs in (refs, got):
        plans = [sg.container_plan(sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])])) for _, m in pairs]
        rc, D, XP, MXP, recs, ms = descent.sd_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, None)
        assert rc == 0 and all(r["sd_status"] == _lib.SD_OK for r in recs), (rc, recs)
        out.append((D, XP, MXP, recs))
    for u, v in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(u, v)
    for p, (ra, rb) in enumerate(zip(out[0][3], out[1][3])):
        assert ra.keys() == rb.keys()
        for f in ra:
            assert ra[f] == rb[f] or (isinstance(ra[f], float) and np.isnan(ra[f]) and np.isnan(rb[f])), (p, f, ra[f], rb[f])
    _free(got), _free(refs)


def test_device_pointers_and_allocation(ctx):
    n, d, k, ns = 140, 65, 2, 6
    specs = [_spec("cubic", 1, n, d, k, seed=900 + p) for p in range(ns)]
    # nine single models released first: the context's pool of released blocks is full (eight entries) of blocks smaller than a slab
    _free([single(ctx, _spec("cubic", 1, 20, 3, 1, seed=950 + p)) for p in range(9)])
    host = batch(ctx, specs)
    X = _queries(d)
    evals = [m.eval_sites(X, want_values=True, want_jac=True) for _, m in host]
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    Cs, Ys = [dev(s["C"]) for s in specs], [dev(s["Y"]) for s in specs]
    # (one start's centres on an odd double: the copy kernel's 8-byte path)
    odd = torch.empty(n * d + 1, dtype=torch.float64, device="cuda")
    odd[1:] = Cs[2].reshape(-1)
    Cs[2] = odd[1:]
    Ws = [torch.full((n, k), float("nan"), dtype=torch.float64, device="cuda") for _ in range(ns)]
    Ls = [torch.full((d + 1, k), float("nan"), dtype=torch.float64, device="cuda") for _ in range(ns)]
    torch.cuda.synchronize()

    def call():
        jobs = (_lib.FitJob * ns)()
        for p, s in enumerate(specs):
            J = jobs[p]
            J.n, J.d, J.k, J.kernel_id, J.poly_deg, J.a, J.b = n, d, k, s["kid"], s["deg"], s["a"], s["b"]
            J.centres, J.values, J.weights_out, J.poly_out = _lib.as_ptr(Cs[p]), _lib.as_ptr(Ys[p]), _lib.as_ptr(Ws[p]), _lib.as_ptr(Ls[p])
        assert ctx.lib.mrbf_fit_batch(ctx.h, ns, jobs, None) == 0
        torch.cuda.synchronize()
        assert all(J.status == 0 and J.model for J in jobs)
        return [pkg.RbfModel(ctx, _lib.c_vp(J.model), n, d, k, d + 1, False, None, None, J.info.asdict()) for J in jobs]

    def check(mods):
        for p, m in enumerate(mods):
            assert np.array_equal(Ws[p].cpu().numpy(), host[p][1].weights) and np.array_equal(Ls[p].cpu().numpy(), host[p][1].poly), p
            V, J = m.eval_sites(X, want_values=True, want_jac=True)
            assert np.array_equal(V, evals[p][0]) and np.array_equal(J, evals[p][1]), p

    _free(host)
    live0 = ctx.get_option(_lib.OPT_LIVE_HANDLES)
    mods = call()
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live0 + ns
    check(mods)
    for p in (3, 0, 5, 1, 4, 2):                       # released in a shuffled order
        mods[p].free()
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live0
    arena = ctx.get_option(_lib.OPT_ARENA_BYTES)
    free_before = torch.cuda.mem_get_info()[0]
    for W in Ws:
        W.fill_(float("nan"))
    mods = call()
    assert torch.cuda.mem_get_info()[0] >= free_before    # the second identical call takes no device memory ...
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) <= arena  # ... (the slab came out of the pool of released blocks)
    check(mods)
    # all but one model of the slab released: the one left is still whole
    for p in (0, 1, 2, 3, 5):
        mods[p].free()
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live0 + 1
    V, J = mods[4].eval_sites(X, want_values=True, want_jac=True)
    assert np.array_equal(V, evals[4][0]) and np.array_equal(J, evals[4][1])
    mods[4].free()
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live0


def test_binding_takes_the_batch(ctx):
    d, ns = 3, 5
    cfgm = pkg.RbfConfig(kernel="multiquadric", polynomial_degree=1)
    data = [_data(40 + p, d, 2, seed=70 + p) for p in range(ns)]
    stats = {}
    mods = pkg.update_models_many(cfgm, [C for C, _ in data], [Y for _, Y in data], 1.0, ctx=ctx, stats=stats)
    assert stats["path"] == "batch" and stats["status"] == [0] * ns and stats["ms_total"] > 0
    for m, (C, Y) in zip(mods, data):
        ref = pkg.update_model(cfgm, C, Y, ctx=ctx)
        assert np.array_equal(m.weights, ref.weights) and np.array_equal(m.poly, ref.poly)
        assert all(m.info[f] == ref.info[f] for f in INFO_EQUAL)
        ref.free()
    scs = [sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])]) for m in mods]
    rng = np.random.default_rng(8)
    X = rng.uniform(-1.0, 1.0, (ns, d))
    sd_stats = {}
    res = descent.sd_iterate_many(descent.SteepestDescentConfig(), scs, None, X, X + 0.01, np.full(ns, 0.3), np.full(d, -2.0),
                                  np.full(d, 2.0), stats=sd_stats)
    assert sd_stats["path"] == "batch" and len(res) == ns
    # the shard solver keeps its models
    from morbit.jl_amd import manystart

    problems = [dict(id=p, cfg=cfgm, sites=C, values=Y, X=_queries(d)[:8]) for p, (C, Y) in enumerate(data)]
    st = {}
    table, kept = manystart.run_local_keep_models(problems, 0, 1, ctx=ctx, stats=st)
    assert st["path"] == "batch" and table.shape == (ns, manystart.RECORD_LEN) and all(table[:, 1] == 0)
    for p, m in enumerate(kept):
        assert np.array_equal(m.weights, mods[p].weights) and table[p, 4] == float(np.sum(m.weights))
        m.free()
    for m in mods:
        m.free()
