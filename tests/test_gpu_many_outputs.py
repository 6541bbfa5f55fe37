"""Fits and evaluations with more than 16 outputs (run with -m gpu): k = 17 .. 1024.

mrbf_fit, mrbf_model_from_coeffs, mrbf_batch_run and mrbf_fit_batch accept 1 <= k <= 1024, and every fast path of the fit (the one-launch
small fit, the three-launch tail basis, the three-launch tail finish) is gated on k <= 16: a fit with k >= 17 is made of other code --
the launch chain at n <= 512, the twelve-launch front end, the old tail finish (apply_linv_t / trsm_lt_small / rocBLAS dtrsm with many
columns), right-hand sides as a full extra block row (65 <= k <= 128) or as several (k > 128) of the persistent factorisation, 5 .. 256
passes of the persistent backward substitution, k / 2 (or k) passes of the evaluation over reused partial buffers.  CASES names one
problem per branch.  The reference is the oracle's LAPACK LU of the saddle system; all bounds are the ones the suite already uses
(tests/test_gpu_parity.py), applied PER OUTPUT COLUMN (column error over that column's own maximum): one bad output among 130 disappears
in a global maximum.  A bounded wait that times out in a later pass makes the fit redo the solve with the blocked kernels -- the numbers
are then right and only info.fallbacks / info.giveup_code show it -- so every fit here also asserts that no fallback happened.

The module writes many_outputs_report.json -- per case the path, fallbacks, cond and every measured error -- into the directory that
MRBF_REPORT_DIR names (default: test_reports/ in the repository root, kept out of git)."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests.conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib
from oracle import rbf_oracle as orc

EPS = np.finfo(np.float64).eps
W_TOL = 1e-10          # BASELINE.json north_star: interpolation weights, relative
REPORT = {}

# name: kernel, polynomial degree, n, d, k    -- what the case reaches
CASES = {
    "a": ("cubic", 1, 100, 6, 17),              # chain at one block column, twelve-launch front end, apply_linv_t_kernel, backsolve_blocked
    "b": ("gaussian", -1, 130, 12, 40),         # chain at two block columns, q = 0, path 1
    "c": ("multiquadric", 1, 300, 100, 18),     # dpad 128, LxInv + apply_linv_t_kernel, persistent back-substitution 5 passes (last KB = 2)
    "d": ("multiquadric", 1, 640, 140, 19),     # trsm_lt_small_kernel with 19 columns, last KB = 3
    "e": ("multiquadric", 1, 520, 300, 17),     # d > 256: rocBLAS dtrsm, eval.hip chunks of 4, last KB = 1
    "f": ("gaussian", -1, 700, 12, 65),         # full extra block row (xreal = 65 > 64: no xhalf), 17 passes
    "g": ("multiquadric", 1, 1536, 64, 66),     # the same with the tail, n >= 512 persistent factorisation
    "h": ("multiquadric", 1, 1029, 128, 20),    # q = 129 (the three-launch tail finish's own limit) but k > 16
    "i": ("multiquadric", 1, 900, 24, 130),     # xt = 256: MT = NT + 2, 33 passes
    "j": ("inv_multiquadric", 0, 1300, 20, 129),  # q = 1, xt = 256, last KB = 1
    "k": ("gaussian", 1, 513, 32, 257),         # xt = 384: MT = NT + 3, ragged n
    "l": ("gaussian", -1, 384, 10, 1024),       # the limit: xt = 1024, MT = NT + 8, 256 passes
    "m": ("cubic", 1, 384, 5, 1024),            # the limit with a tail
    "n": ("cubic", -1, 257, 9, 33),             # LU path (getrs with 33 columns, scatter_solution_kernel from ldB = N)
    "o": ("thin_plate_spline", 0, 200, 5, 21),  # LU path with q = 1
}
LU_CASES = ("n", "o")


@pytest.fixture(scope="module")
def ctx():
    if not has_gpu():
        pytest.skip("needs a GPU (run with -m gpu on the MI355X box)")
    c = pkg.Context()
    yield c
    c.close()
    out = os.environ.get("MRBF_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "many_outputs_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def many_output_data(n, d, k, seed):
    """smooth, and every column different: an output written to the wrong column or a pass skipped cannot cancel"""
    rng = np.random.Generator(np.random.PCG64(seed))
    C = rng.random((n, d))
    s = C.sum(axis=1) / d
    Y = np.stack([np.sin((1 + 3 * j / k) * s * np.pi + 0.37 * j) + 0.1 * (j % 7) for j in range(k)], axis=1)
    return C, Y


_REF = {}


def reference(name):
    """the case's data, the oracle's fit and the oracle's saddle system: computed once, shared by every test, read-only"""
    if name not in _REF:
        kernel, deg, n, d, k = CASES[name]
        C, Y = many_output_data(n, d, k, 1000 + n + d + k)
        cfg = pkg.RbfConfig(kernel=kernel, polynomial_degree=deg)
        kid, a, b = pkg.rbf_model._get_kernel_params(1.0, cfg)
        ref = orc.fit(C, Y, kid, a, b, deg)
        Phi, Pi = orc.gram(C, kid, a, b, deg)
        S = orc.saddle_matrix(Phi, Pi)
        X = np.random.Generator(np.random.PCG64(5)).random((33, d))       # off-site query points
        r = SimpleNamespace(name=name, kernel=kernel, deg=deg, n=n, d=d, k=k, q=Pi.shape[1], cfg=cfg, kid=kid, a=a, b=b, C=C, Y=Y, X=X,
                            ref=ref, S=S, normS=float(np.linalg.norm(S)), cond=float(np.linalg.cond(S)),
                            pi_max=float(np.abs(Pi).max()) if Pi.size else 1.0, V=ref.values(X), J=ref.jacs(X))
        for arr in (C, Y, X, S, ref.w, ref.lam, r.V, r.J):
            arr.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def raw_fit(ctx, r):
    """mrbf_fit through the C ABI: (rc, RbfModel or None)"""
    W = np.full((r.n, r.k), np.nan)
    L = np.full((max(r.q, 1), r.k), np.nan)
    h = _lib.c_vp()
    info = _lib.FitInfo()
    rc = ctx.lib.mrbf_fit(ctx.h, r.n, r.d, r.k, _lib.as_ptr(r.C), _lib.as_ptr(r.Y), r.kid, r.a, r.b, r.deg, ctypes.byref(h),
                          _lib.as_ptr(W), _lib.as_ptr(L), ctypes.byref(info))
    return rc, (pkg.RbfModel(ctx, h, r.n, r.d, r.k, r.q, False, W, L[:r.q], info.asdict()) if rc == 0 else None)


def col_err(A, B, floor=0.0):
    """per output column (axis 1 of (rows, k) arrays and of (m, k, d) Jacobians): max |A - B| over the column / max(floor, max |B| of it)"""
    A, B = np.asarray(A), np.asarray(B)
    if A.ndim == 3:
        A, B = np.transpose(A, (0, 2, 1)).reshape(-1, A.shape[1]), np.transpose(B, (0, 2, 1)).reshape(-1, B.shape[1])
    return np.abs(A - B).max(axis=0) / np.maximum(np.abs(B).max(axis=0), max(floor, 1e-300))


def backward_errors(r, W, Lam):
    """normwise backward error of [W; Lam] in the ORACLE's saddle system (Rigal-Gaches, Frobenius norms), whole and per column"""
    x = np.vstack([W, np.asarray(Lam).reshape(r.q, r.k)])
    b = np.vstack([r.Y, np.zeros((r.q, r.k))])
    R = r.S @ x - b
    whole = float(np.linalg.norm(R) / (r.normS * np.linalg.norm(x) + np.linalg.norm(b)))
    cols = np.linalg.norm(R, axis=0) / (r.normS * np.linalg.norm(x, axis=0) + np.linalg.norm(b, axis=0))
    return whole, cols


def expected_path(r, forced=0):
    if forced:
        return forced
    if r.name in LU_CASES:
        return _lib.PATH_LU
    return _lib.PATH_CHOL if r.q == 0 else _lib.PATH_PROJ_CHOL


def isolated_eval_errors(r, W, Lam, X, V, J):
    """values / Jacobians against the oracle's formulas on the SAME coefficients, per column, over the isolated-evaluation bounds of
    test_eval_from_golden_coeffs_isolated_from_solve (1e-12 sw n for values, 1e-11 sw n for Jacobians, sw = max(1, max |w|) of the
    column): each returned figure is error / bound, < 1 passes"""
    om = orc.OracleModel(r.C, np.asarray(W), np.asarray(Lam).reshape(r.q, r.k), r.kid, r.a, r.b, r.deg)
    sw = np.maximum(1.0, np.abs(W).max(axis=0))
    ev = col_err(V, om.values(X), 1.0) / (1e-12 * sw * r.n) if V is not None else np.zeros(r.k)
    ej = col_err(J, om.jacs(X), 1.0) / (1e-11 * sw * r.n) if J is not None else np.zeros(r.k)
    return ev, ej


def check_fit(r, rc, mod, rec, forced_path=0):
    """every assert of part 1 on one fitted model; rec receives the measured figures (worst column each)"""
    assert rc == 0, (r.name, rc)
    info = mod.info
    rec.update(path=info["path"], fallbacks=info["fallbacks"], giveup_code=info["giveup_code"], cond=r.cond, n=r.n, d=r.d, k=r.k,
               rel_residual=info["rel_residual"], max_pitw=info["max_pitw"])
    ref = r.ref
    ew = col_err(mod.weights, ref.w)
    be, be_cols = backward_errors(r, mod.weights, mod.poly)
    el = col_err(mod.poly, ref.lam, 1.0) if r.q else np.zeros(r.k)
    V, J = mod.eval_sites(r.X, want_values=True, want_jac=True)
    ev, ej = col_err(V, r.V, 1.0), col_err(J, r.J, 1.0)
    iv, ij = isolated_eval_errors(r, mod.weights, mod.poly, r.X, V, J)
    idx = np.arange(0, r.n, max(1, r.n // 97))
    Vs = pkg.eval_models_at_sites(mod, None, r.C[idx])
    ei = np.abs(Vs - r.Y[idx]).max(axis=0) / max(1.0, np.abs(r.Y).max())
    rec.update(w=float(ew.max()), w_worst_column=int(ew.argmax()), backward_error=be, backward_error_worst_column=float(be_cols.max()),
               lam=float(el.max()), v=float(ev.max()), j=float(ej.max()), v_isolated_over_bound=float(iv.max()),
               j_isolated_over_bound=float(ij.max()), interpolation=float(ei.max()))
    print(r.name, json.dumps(rec))
    # path, and no silent fallback
    assert info["path"] == expected_path(r, forced_path), (r.name, info)
    assert info["fallbacks"] == 0 and info["giveup_code"] == 0, (r.name, info)
    # weights: per column against the oracle, and the conditioning-free backward error of the whole solution and of every column
    assert np.isfinite(mod.weights).all() and np.isfinite(mod.poly).all(), r.name
    assert ew.max() < W_TOL, (r.name, int(ew.argmax()), ew.max(), r.cond)      # observed <= 1.1e-12; case m (cond 3.1e5): 3.8e-12
    assert be <= 50 * EPS, (r.name, be)                                         # observed <= 5.9e-17 (0.3 eps)
    assert be_cols.max() <= 50 * EPS, (r.name, int(be_cols.argmax()), be_cols.max())   # observed <= 2.9e-16 (1.3 eps, case k)
    # tail coefficients, as test_solve_paths_agree has them
    assert el.max() < 1e-9, (r.name, int(el.argmax()), el.max())                # observed <= 6.9e-14; case m: 7.8e-13
    # residual and projection
    assert info["rel_residual"] < 1e-10, (r.name, info)                         # observed <= 2.8e-14
    if r.q:
        assert info["max_pitw"] < 1e3 * EPS * max(1.0, np.abs(ref.w).max()) * max(1.0, r.pi_max) * r.n, (r.name, info["max_pitw"])
    # values and Jacobians at 33 off-site points: against the oracle's model, and against the oracle's formulas on the GPU's coefficients
    assert ev.max() < 1e-8 and ej.max() < 1e-8, (r.name, ev.max(), ej.max())    # observed <= 4.9e-13 / 4.2e-13 (case m; else <= 1e-13)
    assert iv.max() < 1.0, (r.name, int(iv.argmax()), iv.max())                 # observed <= 4.7e-5 of the bound
    assert ij.max() < 1.0, (r.name, int(ij.argmax()), ij.max())                 # observed <= 5.2e-6 of the bound
    # interpolation at a strided subset of the training sites
    assert ei.max() < 1e-8, (r.name, int(ei.argmax()), ei.max())                # observed <= 1.1e-13


# ---- 1. fits against the oracle, one case per branch ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_against_oracle(ctx, name):
    r = reference(name)
    rc, mod = raw_fit(ctx, r)
    try:
        check_fit(r, rc, mod, REPORT.setdefault("fit_" + name, {}))
    finally:
        if mod is not None:
            mod.free()


# ---- 2. the three Cholesky implementations and the two solve paths at many outputs ------------------------------------------
@pytest.mark.parametrize("name", ["g", "i"])
def test_cholesky_implementations_agree(ctx, name):
    # impl 1: rocSOLVER potrf / potrs with k columns; impl 2: the host-driven launches with 1 (g) resp. 2 (i) extra row tiles; impl 3:
    # the persistent factorisation
    r = reference(name)
    out = []
    for impl in (1, 2, 3):
        ctx.set_option(_lib.OPT_CHOL_IMPL, impl)
        try:
            rc, mod = raw_fit(ctx, r)
        finally:
            ctx.set_option(_lib.OPT_CHOL_IMPL, 0)
        try:
            check_fit(r, rc, mod, REPORT.setdefault("impl%d_%s" % (impl, name), {}))
            out.append(mod.weights.copy())
        finally:
            if mod is not None:
                mod.free()
    e12, e13, e23 = col_err(out[1], out[0]).max(), col_err(out[2], out[0]).max(), col_err(out[2], out[1]).max()
    REPORT["impl_pairwise_" + name] = dict(impl1_impl2=float(e12), impl1_impl3=float(e13), impl2_impl3=float(e23))
    # the bound of test_fit_same_weights_with_all_cholesky_implementations, per column
    assert e12 < 1e-11 and e13 < 1e-11 and e23 < 1e-11, (name, e12, e13, e23)   # observed <= 1.3e-14


def test_solve_paths_agree_many_outputs(ctx):
    r = reference("g")
    rc1, m1 = raw_fit(ctx, r)
    ctx.set_option(_lib.OPT_FORCE_PATH, _lib.PATH_LU)
    try:
        rc2, m2 = raw_fit(ctx, r)
    finally:
        ctx.set_option(_lib.OPT_FORCE_PATH, 0)
    try:
        assert rc1 == 0 and rc2 == 0
        assert m1.info["path"] == _lib.PATH_PROJ_CHOL and m2.info["path"] == _lib.PATH_LU
        assert m1.info["fallbacks"] == 0 and m2.info["fallbacks"] == 0
        check_fit(r, rc2, m2, REPORT.setdefault("forced_lu_g", {}), forced_path=_lib.PATH_LU)
        ew, el = col_err(m1.weights, m2.weights).max(), col_err(m1.poly, m2.poly, 1.0).max()
        REPORT["paths_g"] = dict(w=float(ew), lam=float(el))
        assert ew < 1e-9 and el < 1e-9, (ew, el)          # the bounds of test_solve_paths_agree, per column (observed 8.2e-14 / 1.3e-14)
    finally:
        for m in (m1, m2):
            if m is not None:
                m.free()


def test_minimum_norm_many_outputs(ctx):
    # fewer sites than tail terms (two sites, d = 5, degree 1: q = 6), k = 20: the twin of the k = 1 check of test_error_codes_and_edge_cases
    n, d, k = 2, 5, 20
    C, Y = many_output_data(n, d, k, 1000 + n + d + k)
    r = SimpleNamespace(name="minnorm", n=n, d=d, k=k, q=d + 1, C=C, Y=Y, kid=4, a=1.0, b=0.0, deg=1)
    rc, mm = raw_fit(ctx, r)
    assert rc == 0 and mm.info["path"] == _lib.PATH_MINNORM, (rc, mm and mm.info)
    ref = orc.fit(C, Y, 4, 1.0, 0.0, 1)          # minimum-norm least squares in the oracle too
    REPORT["minnorm"] = dict(path=mm.info["path"], fallbacks=mm.info["fallbacks"], w=float(np.abs(mm.weights - ref.w).max()),
                             lam=float(np.abs(mm.poly - ref.lam).max()))
    assert np.allclose(mm.weights, ref.w, rtol=0, atol=1e-12) and np.allclose(mm.poly, ref.lam, rtol=0, atol=1e-12)   # observed 4.3e-16 / 3.3e-16
    assert np.allclose(pkg.eval_models_at_sites(mm, None, C), Y, rtol=0, atol=1e-12)  # still interpolates
    mm.free()


# ---- 3. evaluation alone -----------------------------------------------------------------------------------------------------
M_SMALL, M_LARGE = 9, 200
SMALL_ROWS = np.arange(3, M_LARGE, 23)[:M_SMALL]


def _queries(d):
    return np.random.Generator(np.random.PCG64(7)).random((M_LARGE, d))


def _eval_model(name, ncut):
    """the case with the oracle's coefficients; ncut: only its first ncut centres and their weights -- no interpolant any more, but the
    evaluation of given coefficients is what is under test"""
    r = reference(name)
    if ncut is None:
        return r, r.ref.w, r.ref.lam
    rc = SimpleNamespace(**vars(r))
    rc.C, rc.n = np.ascontiguousarray(r.C[:ncut]), ncut
    return rc, np.ascontiguousarray(r.ref.w[:ncut]), r.ref.lam


@pytest.mark.parametrize("name,ncut", [("a", None), ("c", None), ("c", 150), ("d", None), ("d", 150), ("e", None), ("i", None), ("i", 150),
                                       ("l", None), ("l", 150)])
def test_eval_alone_launch_shapes(ctx, name, ncut):
    """model_from_coeffs from the ORACLE's coefficients: the evaluation kernels alone, k / 2 (or k) passes each.  m = 9 and m = 200 query
    points, values only and values + Jacobians (dpad 256, case d: two outputs per pass without Jacobians, one with; k = 19 leaves a single
    last output in both; d = 300, case e: eval.hip's chunks of four outputs).  Which launch splits the centre range (eval_nsplit): a model
    of four centre tiles or more (n > 192) does for BOTH query counts on a device with 256 compute units -- a query batch stays "small"
    up to an eighth of the workgroup slots, 4096 points -- and the combine kernels then run behind every pass over the same partial
    buffers; a model of up to three tiles (case a, and the models cut to 150 centres: dpad 128 and 256, k = 130 and k = 1024) never
    does and finishes every pass inside the evaluation kernel."""
    r, W, Lam = _eval_model(name, ncut)
    mod = pkg.model_from_coeffs(r.cfg, r.C, W, Lam, ctx=ctx)
    X = _queries(r.d)
    Xs = np.ascontiguousarray(X[SMALL_ROWS])
    rec = REPORT.setdefault("eval_%s%s" % (name, "" if ncut is None else "_first%d" % ncut), dict(n=r.n, d=r.d, k=r.k))
    try:
        got = {}
        for m, Xq in ((M_SMALL, Xs), (M_LARGE, X)):
            for jac in (False, True):
                V, J = mod.eval_sites(Xq, want_values=True, want_jac=jac)
                assert np.isfinite(V).all() and (J is None or np.isfinite(J).all()), (name, m, jac)
                iv, ij = isolated_eval_errors(r, W, Lam, Xq, V, J)
                rec["m%d_jac%d" % (m, jac)] = dict(v_over_bound=float(iv.max()), j_over_bound=float(ij.max()))
                assert iv.max() < 1.0, (name, m, jac, int(iv.argmax()), iv.max())     # observed <= 4.9e-5 of the bound
                assert ij.max() < 1.0, (name, m, jac, int(ij.argmax()), ij.max())     # observed <= 5.4e-6 of the bound
                got[m, jac] = (V, J)
        # the same numbers across launch shapes, as test_c3_bench_workload_eval_against_oracle asserts for its two shapes (per column)
        for jac in (False, True):
            (V9, J9), (V200, J200) = got[M_SMALL, jac], got[M_LARGE, jac]
            dv = (np.abs(V9 - V200[SMALL_ROWS]).max(axis=0) / np.maximum(1.0, np.abs(V200).max(axis=0))).max()
            rec["shapes_v_jac%d" % jac] = float(dv)
            assert dv < 1e-12, (name, jac, dv)            # observed 0 (the same bits) at d <= 256; case e (eval.hip): 6.2e-16
            if jac:
                dj = (np.abs(J9 - J200[SMALL_ROWS]).max(axis=(0, 2)) / np.maximum(1.0, np.abs(J200).max(axis=(0, 2)))).max()
                rec["shapes_j"] = float(dj)
                assert dj < 1e-11, (name, dj)             # observed 0 at d <= 256; case e: 1.7e-17
    finally:
        mod.free()


@pytest.mark.parametrize("name", ["a", "i"])
def test_eval_device_pointers(ctx, name):
    # torch tensors in and out: bit for bit the host-staged result, the device Jacobian laid out (m, d, k)
    import torch

    r = reference(name)
    mod = pkg.model_from_coeffs(r.cfg, r.C, r.ref.w, r.ref.lam, ctx=ctx)
    X = _queries(r.d)
    try:
        for Xh in (np.ascontiguousarray(X[SMALL_ROWS]), X):
            m = Xh.shape[0]
            Vh, Jh = mod.eval_sites(Xh, want_values=True, want_jac=True)
            Xd = torch.from_numpy(Xh).cuda()
            Vd = torch.full((m, r.k), float("nan"), dtype=torch.float64, device="cuda")
            Jd = torch.full((m, r.d, r.k), float("nan"), dtype=torch.float64, device="cuda")
            mod.eval_sites(Xd, want_values=True, want_jac=True, out_vals=Vd, out_jac=Jd)
            torch.cuda.synchronize()
            assert np.array_equal(Vd.cpu().numpy(), Vh), (name, m)
            assert np.array_equal(np.transpose(Jd.cpu().numpy(), (0, 2, 1)), Jh), (name, m)
    finally:
        mod.free()


# ---- 4. batched entry points -------------------------------------------------------------------------------------------------
def _synthetic(n, d, k, seed):
    # the small k = 2 problems of test_batch_run_mixed_shapes_matches_single_calls
    rng = np.random.Generator(np.random.PCG64(seed))
    C = rng.random((n, d))
    Y = np.stack([((C - 1.0) ** 2).sum(axis=1), ((C + 1.0) ** 2).sum(axis=1), np.sin(C.sum(axis=1))][:k], axis=1) / d
    return C, Y


def test_batch_run_many_outputs_matches_single_calls(ctx):
    """one mrbf_batch_run over the k = 17, k = 18 and k = 130 problems mixed with three small k = 2 problems: every weight, value and
    Jacobian bit for bit the single call's"""
    specs = []   # cfg, C, Y, m, want_jac
    small = [("cubic", 1, 150, 6, 2, 20, True), ("multiquadric", 1, 257, 100, 2, 70, True), ("cubic", 1, 500, 6, 2, 12, True)]
    for p, (kernel, deg, n, d, k, m, wj) in enumerate(small):
        C, Y = _synthetic(n, d, k, seed=500 + p)
        specs.append((pkg.RbfConfig(kernel=kernel, polynomial_degree=deg), C, Y, m, wj))
    for name, m, wj in (("a", 33, True), ("c", 40, False), ("i", 30, True)):
        r = reference(name)
        specs.append((r.cfg, r.C, r.Y, m, wj))
    specs = [specs[i] for i in (0, 3, 1, 4, 5, 2)]            # mixed: the evaluation groups are not contiguous in the descriptor array
    P = len(specs)
    arr = (_lib.Problem * P)()
    res = (_lib.Result * P)()
    keep = []
    dp = lambda a: a.ctypes.data_as(_lib.c_dp) if a is not None else None
    for p, (cfg, C, Y, m, wj) in enumerate(specs):
        n, d = C.shape
        k = Y.shape[1]
        X = np.random.Generator(np.random.PCG64(600 + p)).random((m, d))
        kid, a, b = pkg.rbf_model._get_kernel_params(1.0, cfg)
        W = np.full((n, k), np.nan)
        V = np.full((m, k), np.nan)
        J = np.full((m, d, k), np.nan) if wj else None
        keep.append((X, W, V, J))
        arr[p] = _lib.Problem(n, m, d, k, kid, cfg.polynomial_degree, a, b, dp(C), dp(Y), dp(X), dp(W), None, dp(V), dp(J))
    assert ctx.lib.mrbf_batch_run(1, None, P, arr, res) == 0
    for p, (cfg, C, Y, m, wj) in enumerate(specs):
        X, W, V, J = keep[p]
        assert res[p].status == 0, (p, res[p].status)
        mod = pkg.update_model(cfg, C, Y, ctx=ctx)
        try:
            assert res[p].fit.path == mod.info["path"] and res[p].fit.fallbacks == 0 and mod.info["fallbacks"] == 0, (p, mod.info)
            assert np.array_equal(mod.weights, W), p
            Vs, Js = mod.eval_sites(X, want_values=True, want_jac=wj)
            assert np.array_equal(Vs, V), p
            if wj:
                assert np.array_equal(Js, np.transpose(J, (0, 2, 1))), p
        finally:
            mod.free()


def test_fit_batch_many_outputs_matches_mrbf_fit(ctx):
    """one mrbf_fit_batch with jobs of k = 2, 17 and 66: each kept model's weights and tail coefficients (and its evaluation) bit for
    bit mrbf_fit's, asserted the way tests/test_gpu_fit_batch.py does for k <= 2"""
    from tests import test_gpu_fit_batch as fb

    specs = [fb._spec("cubic", 1, 40, 3, 2, seed=1)]
    for name in ("a", "g"):
        r = reference(name)
        specs.append(dict(C=r.C, Y=r.Y, kid=r.kid, a=r.a, b=r.b, deg=r.deg))
    refs = [fb.single(ctx, s) for s in specs]
    got = fb.batch(ctx, specs)
    try:
        assert [m.k for _, m in got] == [2, 17, 66]
        for p, (g, s) in enumerate(zip(got, refs)):
            assert s[0] == 0 and s[1].info["fallbacks"] == 0 and g[1].info["fallbacks"] == 0, (p, s[1].info, g[1].info)
            fb.assert_same_model(g, s, ("many_outputs", p))
    finally:
        fb._free(got), fb._free(refs)


# ---- 5. the argument range itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1025])
def test_output_count_out_of_range(ctx, k):
    # (k = 1024 is accepted: cases l and m)
    n, d = 40, 3
    C = np.random.Generator(np.random.PCG64(3)).random((n, d))
    Y = np.zeros((n, max(k, 1)))
    L = np.zeros((d + 1, max(k, 1)))
    live0 = ctx.get_option(_lib.OPT_LIVE_HANDLES)
    h = _lib.c_vp()
    info = _lib.FitInfo()
    assert ctx.lib.mrbf_fit(ctx.h, n, d, k, _lib.as_ptr(C), _lib.as_ptr(Y), 4, 1.0, 0.0, 1, ctypes.byref(h), None, None, ctypes.byref(info)) == -4
    assert h.value is None and b"k = %d" % k in ctx.lib.mrbf_last_error(ctx.h)
    h = _lib.c_vp()
    assert ctx.lib.mrbf_model_from_coeffs(ctx.h, n, d, k, _lib.as_ptr(C), _lib.as_ptr(Y), _lib.as_ptr(L), 4, 1.0, 0.0, 1, ctypes.byref(h)) == -4
    assert h.value is None
    # mrbf_fit_batch refuses the call as it refuses its other range errors (-3, nothing written), a valid job beside the bad one included
    jobs = (_lib.FitJob * 2)()
    Wn = np.full((n, 1), np.nan)
    for p, kk in enumerate((1, k)):
        J = jobs[p]
        J.n, J.d, J.k, J.kernel_id, J.poly_deg, J.a, J.b = n, d, kk, 4, 1, 1.0, 0.0
        J.centres, J.values = _lib.as_ptr(C), _lib.as_ptr(Y)
        J.weights_out = _lib.as_ptr(Wn) if p == 0 else None
    assert ctx.lib.mrbf_fit_batch(ctx.h, 2, jobs, None) == -3
    assert all(J.model is None for J in jobs) and np.isnan(Wn).all()
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live0       # no model handle is left behind
