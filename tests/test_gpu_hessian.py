"""Model Hessians on the device (mrbf_eval_hessian; run with -m gpu) against the extended-precision difference-form reference and the
derived bound of tests/hessian_util.py (checked on the CPU by tests/test_hessian_reference.py):

    |H_ij - H_ref,ij| <= 2 (n + 8 d + 32) 2^-52 S_ij

Models come from model_from_coeffs with random centres in the unit box and normal weights (no solve); output buffers start as NaN.
The module writes hessian_report.json -- the worst error / bound per radial function and per shape -- into the directory that
MRBF_REPORT_DIR names (default: test_reports/ in the repository root, kept out of git)."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import hessian_util as hu
from tests import near_centre_util as ncu
from tests.conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, rbf_model as rm, surrogates as sg

REPORT = {}
ALL_KERNELS = sorted(ncu.KERNELS) + sorted(hu.EXTRA_KERNELS)
DELTAS = (0.0, 1e-12, 1e-9, 3e-8, 1e-6, 1e-4, 1e-2)


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()
    out = os.environ.get("MRBF_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "hessian_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def make_model(ctx, C, W, kid, a, b, deg=-1, Lam=None):
    """mrbf_model_from_coeffs with the kernel parameters as given (the pow paths of the multiquadrics have no RbfConfig)"""
    n, d = C.shape
    k = W.shape[1]
    q = 0 if deg < 0 else (1 if deg == 0 else d + 1)
    h = _lib.c_vp()
    ctx.check(ctx.lib.mrbf_model_from_coeffs(ctx.h, n, d, k, _lib.as_ptr(C), _lib.as_ptr(W), _lib.as_ptr(Lam), kid, a, b, deg, ctypes.byref(h)))
    return rm.RbfModel(ctx, h, n, d, k, q, False, W, Lam, None)


def nan_out(m, r, d):
    return np.full((m, r, d, d), np.nan)


def check(tag, H, H_ref, S, n, d):
    ratio = hu.errors_over_bound(H, H_ref, S, n, d)
    worst = float(ratio.max())
    print(tag, "worst error / bound %.3e" % worst)
    assert np.isfinite(H).all(), tag
    assert worst < 1.0, (tag, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst


def note(group, key, worst):
    REPORT.setdefault(group, {})[key] = max(worst, REPORT.get(group, {}).get(key, 0.0))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. every variant of the kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(hu.VARIANTS))
def test_shapes_against_the_bound(ctx, variant):
    case = hu.variant_case(variant)
    mod = make_model(ctx, case.C, case.W, case.kid, case.a, case.b)
    try:
        info = {}
        r = case.k if case.rows is None else len(case.rows)
        H = mod.hessian_sites(case.X, rows=case.rows, out=nan_out(case.m, r, case.d), info=info)
    finally:
        mod.free()
    print(variant, info)
    note("shapes", variant, check(variant, H, case.H_ref, case.S, case.n, case.d))
    assert same_bits(H, np.swapaxes(H, 2, 3))
    assert info["chunks"] == 1 and info["nsplit"] >= 1


def test_the_variants_split_as_their_table_says(ctx):
    """the split counts the VARIANTS table names, as the library reports them"""
    want = {"one": 1, "d3_n3": 1, "d15_n4": 1, "d16_n5": 1, "d17_n63": 2, "d64_n257": 9, "d65_n65": 3, "d65_unsplit": 1, "d140_n64": 2,
            "d300_n300": 10, "d300_n5": 1}
    assert sorted(want) == sorted(hu.VARIANTS)
    for variant, ns in want.items():
        d, n, m, k, kind, _ = hu.VARIANTS[variant]
        rng = np.random.default_rng(1)
        mod = make_model(ctx, rng.random((n, d)), rng.standard_normal((n, k)), 2, 1.0, 0.5)
        try:
            info = {}
            mod.hessian_sites(rng.random((m, d)), rows=hu.variant_rows(k, kind), info=info)
        finally:
            mod.free()
        assert info["nsplit"] == ns, (variant, info)


# ---- 2. every radial function, fast and pow paths, split and unsplit ---------------------------------------------------------------
@pytest.mark.parametrize("variant", ["d16_n5", "d17_n63"])
@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_radial_functions(ctx, kernel, variant):
    case = hu.variant_case(variant, kernel)
    mod = make_model(ctx, case.C, case.W, case.kid, case.a, case.b)
    try:
        r = case.k if case.rows is None else len(case.rows)
        H = mod.hessian_sites(case.X, rows=case.rows, out=nan_out(case.m, r, case.d))
    finally:
        mod.free()
    note("radial", kernel, check("%s %s" % (kernel, variant), H, case.H_ref, case.S, case.n, case.d))


# ---- 3. near centres --------------------------------------------------------------------------------------------------------------
_NEAR = {}


def near_case(kernel):
    """d = 17, n = 70, k = 2: queries at the seven distances from the centres at the edges of a 4-centre step (3, 4), of a round of 32
    (31, 32) and of the range (0, n - 1); m = 42 splits the centre range in 3"""
    if kernel not in _NEAR:
        d, n, k = 17, 70, 2
        kid, a, b = hu.kernel_ids(kernel, d)
        C, W, rng = hu.random_model(d, n, k, 777)
        targets = (0, 3, 4, 31, 32, n - 1)
        X = hu.near_queries(C, targets, DELTAS, rng)
        H_ref, S = hu.reference_hessian(C, W, kid, a, b, X)
        _NEAR[kernel] = (C, W, kid, a, b, X, H_ref, S)
    return _NEAR[kernel]


@pytest.mark.parametrize("kernel", sorted(ncu.KERNELS))
def test_near_centres(ctx, kernel):
    C, W, kid, a, b, X, H_ref, S = near_case(kernel)
    mod = make_model(ctx, C, W, kid, a, b)
    try:
        info = {}
        H = mod.hessian_sites(X, out=nan_out(X.shape[0], 2, 17), info=info)
    finally:
        mod.free()
    assert info["nsplit"] == 3
    ratio = hu.errors_over_bound(H, H_ref, S, 70, 17).reshape(6, len(DELTAS), -1).max(axis=(0, 2))
    rec = {"%g" % dl: float(v) for dl, v in zip(DELTAS, ratio)}
    REPORT.setdefault("near", {})[kernel] = rec
    print(kernel, json.dumps(rec))
    assert np.isfinite(H).all()            # at distance 0 too: the centre under the query contributes w psi(0) I alone
    assert ratio.max() < 1.0, (kernel, rec)
    note("radial", kernel, float(ratio.max()))


# ---- 4. exact properties ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """d = 17, n = 63, k = 3, m = 6 (split) -- and the same model asked at m = 600 (unsplit)"""
    C, W, rng = hu.random_model(17, 63, 3, 99)
    mod = make_model(ctx, C, W, 2, 1.0, 0.5)
    X = np.ascontiguousarray(rng.random((6, 17)))
    yield mod, X, rng
    mod.free()


def test_symmetry_repeats_and_determinism_are_exact(small):
    mod, X, rng = small
    for Xq in (X, np.ascontiguousarray(np.tile(X, (100, 1)))):        # split in 2; the centre range in one piece
        info = {}
        H = mod.hessian_sites(Xq, rows=[1, 0, 1, 2, 2], out=nan_out(Xq.shape[0], 5, 17), info=info)
        assert info["nsplit"] == (2 if Xq.shape[0] == 6 else 1)
        assert same_bits(H, np.swapaxes(H, 2, 3))
        assert same_bits(H[:, 0], H[:, 2]) and same_bits(H[:, 3], H[:, 4])
        again = mod.hessian_sites(Xq, rows=[1, 0, 1, 2, 2], out=nan_out(Xq.shape[0], 5, 17))
        assert same_bits(H, again)
        # a selected row is the block of the full call: the passes do not leak into each other
        full = mod.hessian_sites(Xq, out=nan_out(Xq.shape[0], 3, 17))
        assert same_bits(full[:, [1, 0, 1, 2, 2]], H)
        perm = rng.permutation(Xq.shape[0])
        Hp = mod.hessian_sites(np.ascontiguousarray(Xq[perm]), rows=[1, 0, 1, 2, 2], out=nan_out(Xq.shape[0], 5, 17))
        assert same_bits(Hp, H[perm])
        if Xq.shape[0] == 600:                                        # identical queries give identical blocks
            assert same_bits(H[:6], H[6:12])


def test_host_and_device_buffers_agree(small):
    mod, X, _ = small
    m, d, r = X.shape[0], 17, 3
    host = mod.hessian_sites(X, out=nan_out(m, r, d))
    xbuf = torch.full((m * d + 1,), float("nan"), dtype=torch.float64, device="cuda")
    xdev = xbuf[1:].view(m, d)                                       # a device buffer on an odd double
    xdev.copy_(torch.from_numpy(X))
    for x_dev in (False, True):
        for out_dev in (False, True):
            if out_dev:
                obuf = torch.full((m * r * d * d + 1,), float("nan"), dtype=torch.float64, device="cuda")
                out = obuf[1:].view(m, r, d, d)
                assert out.data_ptr() % 16 == 8
            else:
                out = nan_out(m, r, d)
            got = mod.hessian_sites(xdev if x_dev else X, out=out)
            got = got.cpu().numpy() if out_dev else got
            assert same_bits(got, host), (x_dev, out_dev)
            if out_dev:
                assert np.isnan(obuf[:1].cpu().numpy()).all()        # nothing in front of the buffer was touched


def test_stage_limit_does_not_change_the_bits_and_nothing_grows(ctx, small):
    mod, X, _ = small
    m, d, r = X.shape[0], 17, 3
    info = {}
    host = mod.hessian_sites(X, out=nan_out(m, r, d), info=info)
    assert info["chunks"] == 1
    for limit, chunks in ((1, m), (2 * r * d * d * 8, 3)):
        info = {}
        got = mod.hessian_sites(X, out=nan_out(m, r, d), info=info, stage_bytes=limit)
        assert info["chunks"] == chunks and same_bits(got, host), (limit, info)
    # 1 MiB: a result of 3 MiB goes in chunks of whole points
    Xw = np.ascontiguousarray(np.tile(X, (60, 1)))                   # 360 points of 6936 bytes each
    info = {}
    wide = mod.hessian_sites(Xw, out=nan_out(360, r, d), info=info)
    assert info["chunks"] == 1
    info = {}
    got = mod.hessian_sites(Xw, out=nan_out(360, r, d), info=info, stage_bytes=1 << 20)
    assert info["chunks"] == -(-360 // ((1 << 20) // (r * d * d * 8))) and same_bits(got, wide)
    arena = ctx.get_option(_lib.OPT_ARENA_BYTES)
    again = mod.hessian_sites(Xw, out=nan_out(360, r, d))
    assert same_bits(again, wide) and ctx.get_option(_lib.OPT_ARENA_BYTES) == arena


# ---- 5. against central differences of the device Jacobian ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["gaussian", "multiquadric", "cubic5"])
def test_against_the_device_jacobian(ctx, kernel):
    d, n, k, m, h = 17, 40, 2, 3, 1e-4
    kid, a, b = hu.kernel_ids(kernel, d)
    C, W, rng = hu.random_model(d, n, k, 31)
    X = np.ascontiguousarray(0.25 + 0.5 * rng.random((m, d)))
    Lam = np.zeros((d + 1, k))
    mod = make_model(ctx, C, W, kid, a, b, 1, Lam)
    try:
        H = mod.hessian_sites(X, out=nan_out(m, k, d))
        Xpm = np.ascontiguousarray(np.concatenate([X[:, None, :] + s * h * np.eye(d)[None] for s in (1.0, -1.0)], axis=1).reshape(-1, d))
        _, J = mod.eval_sites(Xpm, want_values=False, want_jac=True)
    finally:
        mod.free()
    J = np.asarray(J).reshape(m, 2, d, k, d)                            # point, sign, displaced coordinate j, output, coordinate i
    step = (Xpm.reshape(m, 2, d, d)[:, 0] - Xpm.reshape(m, 2, d, d)[:, 1])[:, np.arange(d), np.arange(d)]   # the 2h actually taken
    fd = np.transpose((J[:, 0] - J[:, 1]) / step[:, :, None, None], (0, 2, 3, 1))   # [p, l, i, j] = d J_li / d x_j
    # the three allowances
    H_ref, S = hu.reference_hessian(C, W, kid, a, b, X)
    J_ref = hu.reference_jacobian_ld(C, W, kid, a, b, Xpm).reshape(m, 2, d, k, d)
    fd_ref = np.transpose((J_ref[:, 0] - J_ref[:, 1]) / step.astype(hu.LD)[:, :, None, None], (0, 2, 3, 1))
    trunc = 2.0 * np.abs(fd_ref - H_ref).astype(np.float64)
    V_dummy = np.zeros((1, k))
    _, bj = ncu.bounds(W, n, V_dummy, J_ref.reshape(-1, k, d))
    allowed = trunc + (2.0 * bj / h)[None, :, None, None] + hu.factor(n, d) * S.astype(np.float64)
    diff = np.abs(H - fd)
    print(kernel, "worst difference / allowance %.3e" % float((diff / allowed).max()))
    assert (diff <= allowed).all(), (kernel, float((diff / allowed).max()))


# ---- 6. models of every origin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [-1, 0, 1])
def test_models_of_every_origin(ctx, deg):
    d, n, k, m = 5, 40, 2, 4
    a = hu.gaussian_shape(d)
    cfg = pkg.RbfConfig(kernel="gaussian", shape_parameter=a, polynomial_degree=deg)
    C, _, rng = hu.random_model(d, n, k, 5 + deg)
    Y = np.stack([np.sin(C.sum(axis=1)), np.cos(C @ np.arange(1.0, d + 1.0) / d)], axis=1)
    X = np.ascontiguousarray(rng.random((m, d)))
    fitted = pkg.update_model(cfg, C, Y, ctx=ctx)
    batch = pkg.update_models_many([cfg, cfg], [C, C], [Y, Y], 1.0, ctx=ctx)
    coeffs = pkg.model_from_coeffs(cfg, C, fitted.weights, fitted.poly if deg >= 0 else None, ctx=ctx)
    mods = [fitted, batch[0], batch[1], coeffs]
    try:
        for mod in mods:
            assert mod is not None
            H = mod.hessian_sites(X, out=nan_out(m, k, d))
            H_ref, S = hu.reference_hessian(C, mod.weights, 4, a, 0.0, X)     # the tail has no second derivative
            check("origin deg %d" % deg, H, H_ref, S, n, d)
    finally:
        for mod in mods:
            mod.free()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, small):
    mod, X, _ = small
    lib = ctx.lib
    m, d, k = X.shape[0], 17, 3
    out = nan_out(m, k, d)
    rows_bad = np.array([0, 3], dtype=np.int32)
    rows_neg = np.array([-1], dtype=np.int32)
    rows_ok = np.array([2, 0], dtype=np.int32)
    info = _lib.HessInfo()
    P = _lib.as_ptr
    other = pkg.Context()
    try:
        cases = [
            (-1, (None, mod.model, m, P(X), 0, None, P(out), None)),
            (-2, (ctx.h, None, m, P(X), 0, None, P(out), None)),
            (-4, (other.h, mod.model, m, P(X), 0, None, P(out), None)),       # a model of another context: mrbf_eval_batch's code
            (-3, (ctx.h, mod.model, -1, P(X), 0, None, P(out), None)),
            (-5, (ctx.h, mod.model, m, P(X), -1, None, P(out), None)),
            (-5, (ctx.h, mod.model, m, P(X), 2, None, P(out), None)),
            (-6, (ctx.h, mod.model, m, P(X), 2, P(rows_bad), P(out), None)),
            (-6, (ctx.h, mod.model, m, P(X), 1, P(rows_neg), P(out), None)),
            (-6, (ctx.h, mod.model, 0, None, 2, P(rows_bad), None, None)),      # the rows are looked at whatever m is
            (-4, (ctx.h, mod.model, m, None, 0, None, P(out), None)),
            (-7, (ctx.h, mod.model, m, P(X), 0, None, None, None)),
        ]
        for want, args in cases:
            assert lib.mrbf_eval_hessian(*args) == want, (want, args)
            assert lib.mrbf_eval_hessian_limited(*args, 1) == want, (want, args)
            assert np.isnan(out).all()
    finally:
        other.close()
    # m = 0: nothing to do, whatever the pointers; the info is cleared
    info.nsplit = 77
    assert lib.mrbf_eval_hessian(ctx.h, mod.model, 0, None, 2, P(rows_ok), None, ctypes.byref(info)) == 0
    assert info.nsplit == 0 and info.chunks == 0
    assert lib.mrbf_eval_hessian(ctx.h, mod.model, 0, P(X), 0, None, P(out), None) == 0
    assert np.isnan(out).all()
    assert mod.hessian_sites(np.empty((0, d))).shape == (0, k, d, d)


# ---- 8. bindings ------------------------------------------------------------------------------------------------------------------------
def test_bindings(small):
    mod, X, _ = small
    full = mod.hessian_sites(X)
    assert full.shape == (6, 3, 17, 17)
    assert same_bits(rm.get_hessian(mod, None, X[2], 1), full[2, 1])
    assert same_bits(pkg.get_hessian(mod, None, X[0], 2), full[0, 2])
    assert same_bits(rm.get_hessians_at_sites(mod, None, X), full)
    assert same_bits(pkg.get_hessians_at_sites(mod, None, X, rows=[2, 2, 0]), full[:, [2, 2, 0]])
    assert same_bits(sg.get_hessian(mod, None, X[1], 0), full[1, 0])
    ref = sg.RefSurrogate(mod, [2, 0])
    assert same_bits(sg.get_hessian(ref, None, X[3], 0), full[3, 2]) and same_bits(sg.get_hessian(ref, None, X[3], 1), full[3, 0])
    comp = sg.CompositeSurrogate(mod, None, [0, 1], num_outputs=1)
    with pytest.raises(NotImplementedError):
        sg.get_hessian(comp, None, X[0], 0)
