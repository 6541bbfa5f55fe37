"""The one-launch LU of the saddle system (small_lu.hip, MRBF_OPT_SMALL_LU; run with -m gpu).

Off means off (bit identity with the option at 0 before and after it was touched); with the option on: accuracy against
extended-precision truths by the rule of tests/test_gpu_parity.py (within 1e-10 of the truth, or no further from it than twice the
oracle's LAPACK LU), the Rigal-Gaches backward error on the oracle's saddle matrix at the sizes no truth covers (bar: 50 eps, as
there), pivoting, batch = single bit for bit, a singular start among healthy ones, the handles as ordinary models, the bindings.

Shapes: N = n + q in {2, 15, 16, 17, 33, 65, 129, 190} (tests/golden/make_lu_truth.py: below, at and above one 16-column panel, a
padded last panel), N = 512 (508 + 4: no padding at all), 318 and 641 (the kernel's largest system: 41 panels, k = 16)."""
import ctypes
import os

import numpy as np
import pytest

from tests.conftest import ROOT, dist_from_truth, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg
from oracle import rbf_oracle as orc

EPS = np.finfo(np.float64).eps
W_TOL = 1e-10  # tests/test_gpu_parity.py
TPS2, CUBIC3, CUBIC5, MQ, CUBIC1 = (3, 2.0, 0.0), (0, 3.0, 0.0), (0, 5.0, 0.0), (2, 1.0, 0.5), (0, 1.0, 0.0)
INFO_BITS = ("path", "factor_info", "n", "q", "rel_residual", "max_pitw", "mu", "fallbacks", "giveup_code")


@pytest.fixture()
def ctx():
    c = pkg.Context()
    yield c
    c.close()


@pytest.fixture()
def lu_ctx(ctx):
    ctx.set_option(_lib.OPT_SMALL_LU, 1)
    return ctx


def _q(d, deg):
    return 0 if deg < 0 else (1 if deg == 0 else d + 1)


def _data(n, d, k, seed):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-2.0, 2.0, (n, d))
    cols = [np.sum((C - 1.0) ** 2, axis=1), np.sum((C + 1.0) ** 2, axis=1) + C[:, 0]] + [np.sin(C[:, 0] + l) + C[:, -1] * l for l in range(2, k)]
    return C, np.ascontiguousarray(np.stack(cols, axis=1)[:, :k])


def _spec(kern, deg, n, d, k, seed):
    C, Y = _data(n, d, k, seed)
    return dict(C=C, Y=Y, kid=kern[0], a=kern[1], b=kern[2], deg=deg)


def single(ctx, s):
    n, d = s["C"].shape
    k, q = s["Y"].shape[1], _q(d, s["deg"])
    W, L = np.full((n, k), np.nan), np.full((max(q, 1), k), np.nan)
    h, info = _lib.c_vp(), _lib.FitInfo()
    rc = ctx.lib.mrbf_fit(ctx.h, n, d, k, _lib.as_ptr(s["C"]), _lib.as_ptr(s["Y"]), s["kid"], s["a"], s["b"], s["deg"], ctypes.byref(h),
                          _lib.as_ptr(W), _lib.as_ptr(L), ctypes.byref(info))
    return rc, (pkg.RbfModel(ctx, h, n, d, k, q, False, W, L[:q], info.asdict()) if rc == 0 else None)


def batch(ctx, specs):
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
    rc = ctx.lib.mrbf_fit_batch(ctx.h, ns, jobs, None)
    assert rc == 0, (rc, ctx.lib.mrbf_last_error(ctx.h))
    res = []
    for p, (n, d, k, q, W, L) in enumerate(outs):
        J = jobs[p]
        assert (J.model is None) == (J.status != 0), (p, J.status, J.model)
        res.append((int(J.status), pkg.RbfModel(ctx, _lib.c_vp(J.model), n, d, k, q, False, W, L[:q], J.info.asdict()) if J.status == 0 else None))
    return res


def _free(pairs):
    for _, m in pairs:
        if m is not None:
            m.free()


def _took_the_one_launch_lu(info):
    # fit_lu times its Gram kernel and its getrs; the one launch has neither phase
    return info["path"] == _lib.PATH_LU and info["ms_gram"] == 0.0 and info["ms_solve"] == 0.0 and info["ms_factor"] > 0.0


def assert_same(got, ref, tag, lu=None):
    (gs, gm), (rs, rm_) = got, ref
    assert gs == rs, (tag, gs, rs)
    if rs != 0:
        return
    assert np.array_equal(gm.weights, rm_.weights) and np.array_equal(gm.poly, rm_.poly), tag
    X = np.random.default_rng(77 + gm.d).uniform(-2.0, 2.0, (37, gm.d))
    gV, gJ = gm.eval_sites(X, want_values=True, want_jac=True)
    rV, rJ = rm_.eval_sites(X, want_values=True, want_jac=True)
    assert np.array_equal(gV, rV) and np.array_equal(gJ, rJ), tag
    for f in ("path", "fallbacks", "n", "q", "factor_info"):
        assert gm.info[f] == rm_.info[f], (tag, f, gm.info, rm_.info)
    if lu is not None:
        assert (gm.info["path"] == _lib.PATH_LU) == lu, (tag, gm.info)


def test_off_means_off():
    s = _spec(TPS2, 1, 40, 3, 2, seed=1)
    c = pkg.Context()
    try:
        assert c.get_option(_lib.OPT_SMALL_LU) == 0
        rc0, m0 = single(c, s)
        assert rc0 == 0 and m0.info["path"] == _lib.PATH_LU and not _took_the_one_launch_lu(m0.info)
        c.set_option(_lib.OPT_SMALL_LU, 1)
        assert c.get_option(_lib.OPT_SMALL_LU) == 1
        for bad in (2.0, -1.0):
            assert c.lib.mrbf_set_option(c.h, _lib.OPT_SMALL_LU, bad) == -2 and c.get_option(_lib.OPT_SMALL_LU) == 1
        rc_on, m_on = single(c, s)
        assert rc_on == 0 and _took_the_one_launch_lu(m_on.info), m_on.info
        c.set_option(_lib.OPT_SMALL_LU, 0)
        rc1, m1 = single(c, s)
        assert rc1 == 0
        assert np.array_equal(m0.weights, m1.weights) and np.array_equal(m0.poly, m1.poly)
        for f in INFO_BITS:
            assert m0.info[f] == m1.info[f], (f, m0.info, m1.info)
        _free([(0, m0), (0, m_on), (0, m1)])
    finally:
        c.close()


def _on_lu_path(c):
    n, d = c["C"].shape
    q = orc.poly_dim(d, c["deg"])
    return n >= q and not (orc.cpd_order(c["kid"], c["a"], c["b"]) <= c["deg"] + 1 and n > q)


def test_accuracy_fixture_cases(lu_ctx, golden):
    cases = [c for c in golden if _on_lu_path(c)]
    assert len(cases) == 21
    for c in cases:
        s = dict(C=np.ascontiguousarray(c["C"]), Y=np.ascontiguousarray(c["Y"]).reshape(c["C"].shape[0], -1), kid=c["kid"], a=c["a"], b=c["b"],
                 deg=c["deg"])
        rc, m = single(lu_ctx, s)
        assert rc == 0 and _took_the_one_launch_lu(m.info), (c["name"], rc, m and m.info)
        tw_gpu, tw_orc = dist_from_truth(m.weights, c["truth"]["W"]), dist_from_truth(c["W"], c["truth"]["W"])
        print("%-44s cond %.1e  GPU %.2e  oracle LU %.2e from the truth" % (c["name"], c["cond"], tw_gpu, tw_orc))
        assert tw_gpu <= max(W_TOL, 2.0 * tw_orc), (c["name"], tw_gpu, tw_orc)
        assert m.info["rel_residual"] < 1e-10, (c["name"], m.info)
        m.free()


@pytest.fixture(scope="module")
def lu_truth():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lu_truth.npz"))
    out = []
    for idx in range(int(z["count"][0])):
        pre = "c%03d_" % idx
        kid, a, b, deg = z[pre + "kernel"]
        out.append(dict(C=np.ascontiguousarray(z[pre + "C"]), Y=np.ascontiguousarray(z[pre + "Y"]), kid=int(kid), a=float(a), b=float(b), deg=int(deg),
                        W=(z[pre + "W_hi"], z[pre + "W_lo"]), Lam=(z[pre + "Lam_hi"], z[pre + "Lam_lo"])))
    return out


def test_accuracy_new_truths(lu_ctx, lu_truth):
    seen_N, seen_d, n_eq_q = set(), set(), 0
    for t in lu_truth:
        n, d = t["C"].shape
        q = _q(d, t["deg"])
        seen_N.add(n + q), seen_d.add(d)
        n_eq_q += n == q
        rc, m = single(lu_ctx, t)
        assert rc == 0 and _took_the_one_launch_lu(m.info), (n, d, q, rc)
        ref = orc.fit(t["C"], t["Y"], t["kid"], t["a"], t["b"], t["deg"])
        tw_gpu, tw_orc = dist_from_truth(m.weights, t["W"]), dist_from_truth(ref.w, t["W"])
        print("kid %d deg %2d d %3d N %3d: GPU %.2e  oracle LU %.2e from the truth" % (t["kid"], t["deg"], d, n + q, tw_gpu, tw_orc))
        assert tw_gpu <= max(W_TOL, 2.0 * tw_orc), (t["kid"], t["deg"], d, n + q, tw_gpu, tw_orc)
        if q:
            tl_gpu, tl_orc = dist_from_truth(m.poly, t["Lam"]), dist_from_truth(ref.lam, t["Lam"])
            assert tl_gpu <= max(W_TOL, 2.0 * tl_orc), (t["kid"], t["deg"], d, n + q, tl_gpu, tl_orc)
        m.free()
    assert seen_N == {2, 15, 16, 17, 33, 65, 129, 190} and seen_d == {1, 3, 65} and n_eq_q == 1


def _backward_error(s, W, Lam):
    """Rigal-Gaches, Frobenius norms, on the ORACLE's saddle matrix (tests/test_gpu_parity.py::_backward_error)"""
    Phi, Pi = orc.gram(s["C"], s["kid"], s["a"], s["b"], s["deg"])
    S = orc.saddle_matrix(Phi, Pi)
    q = Pi.shape[1]
    x = np.vstack([W, np.asarray(Lam).reshape(q, W.shape[1])])
    b = np.vstack([s["Y"], np.zeros((q, W.shape[1]))])
    return float(np.linalg.norm(S @ x - b) / (np.linalg.norm(S) * np.linalg.norm(x) + np.linalg.norm(b)))


@pytest.mark.parametrize("n,d,k", [(508, 3, 2), (512, 128, 16), (300, 17, 1)])
def test_backward_error_without_a_truth(lu_ctx, n, d, k):
    s = _spec(TPS2, 1, n, d, k, seed=n + d)
    rc, m = single(lu_ctx, s)
    assert rc == 0 and _took_the_one_launch_lu(m.info), (rc, m and m.info)
    be = _backward_error(s, m.weights, m.poly)
    print("n %d d %d k %d: backward error %.2f eps, residual %.2e" % (n, d, k, be / EPS, m.info["rel_residual"]))
    assert be <= 50 * EPS, be / EPS
    m.free()


# (condition numbers of these systems, by the oracle: 2.0e4, 7.8e4, 9.2e5, 8.0e5)
@pytest.mark.parametrize("kern,deg,n,d", [(CUBIC3, -1, 50, 3), (CUBIC3, 0, 50, 3), (TPS2, 1, 30, 3), (CUBIC3, 0, 40, 17)])
def test_pivoting_is_exercised(lu_ctx, kern, deg, n, d):
    """cubic without a tail has a zero diagonal, every q > 0 system the zero block: no solution without row interchanges"""
    s = _spec(kern, deg, n, d, 2, seed=5 * n + d)
    Phi, Pi = orc.gram(s["C"], s["kid"], s["a"], s["b"], s["deg"])
    cond = np.linalg.cond(orc.saddle_matrix(Phi, Pi))
    assert cond < 1e6 and (Pi.shape[1] > 0 or np.all(np.diag(Phi) == 0.0))
    rc, m = single(lu_ctx, s)
    assert rc == 0 and _took_the_one_launch_lu(m.info)
    assert m.info["rel_residual"] < 1e-10, (cond, m.info)
    m.free()


@pytest.mark.parametrize("n,d", [(33, 16), (140, 65)])
def test_batch_equals_single_nine_starts(lu_ctx, n, d):
    specs = [_spec(TPS2, 1, n, d, 2, seed=1000 * n + 10 * d + p) for p in range(9)]
    refs = [single(lu_ctx, s) for s in specs]
    assert all(rc == 0 and _took_the_one_launch_lu(m.info) for rc, m in refs)
    for members in (range(9), range(5), [3]):
        got = batch(lu_ctx, [specs[p] for p in members])
        for g, p in zip(got, members):
            assert_same(g, refs[p], (n, d, len(got), p), lu=True)
        _free(got)
    # the same batch twenty times: identical bits; a second identical call (the first one's models released) leaves the arena as it was
    first = [(m.weights.copy(), m.poly.copy()) for _, m in refs]
    arena = None
    for rep in range(20):
        again = batch(lu_ctx, specs)
        for (W, L), (_, b) in zip(first, again):
            assert np.array_equal(W, b.weights) and np.array_equal(L, b.poly)
        _free(again)
        if rep == 0:
            arena = lu_ctx.get_option(_lib.OPT_ARENA_BYTES)
        assert lu_ctx.get_option(_lib.OPT_ARENA_BYTES) == arena
    _free(refs)


def test_mixed_permuted_batch(lu_ctx):
    d = 3
    specs = [_spec(TPS2, 1, 13, d, 2, 1), _spec(CUBIC3, 1, 40, d, 2, 2),            # LU (N = 17) | Cholesky
             _spec(CUBIC3, -1, 129, d, 1, 3), _spec(TPS2, 1, 600, d, 2, 4),         # LU (N = 129) | n beyond the range
             _spec(MQ, -1, 90, 65, 3, 5), _spec(TPS2, 1, 140, 129, 1, 6),           # LU, d = 65 | d beyond the range
             _spec(CUBIC3, 0, 60, d, 17, 7), _spec(CUBIC1, -1, 30, d, 1, 8),        # k beyond the range | nonsmooth kernel
             _spec(CUBIC5, 1, 66, 65, 2, 9), _spec(MQ, 1, 57, d, 2, 10)]            # LU with n == q | Cholesky
    one_launch = [True, False, True, False, True, False, False, False, True, False]
    refs = [single(lu_ctx, s) for s in specs]
    for p, ((rc, m), want) in enumerate(zip(refs, one_launch)):
        assert rc == 0 and _took_the_one_launch_lu(m.info) == want, (p, rc, m and m.info)
    perm = [4, 9, 0, 7, 2, 5, 8, 1, 6, 3]
    got = batch(lu_ctx, [specs[i] for i in perm])
    for j, i in enumerate(perm):
        assert_same(got[j], refs[i], ("mixed", j, i))
    _free(got), _free(refs)


def test_singular_start_among_three(ctx):
    """a duplicated site: two equal rows of the saddle matrix.  The unblocked getrf of the option-off path meets an exactly zero pivot;
    the blocked kernel does too because equal sites have a distance of exactly zero and lu_trailing mirrors the chain that forms U12
    (small_lu.hip)"""
    specs = [_spec(TPS2, 1, 40, 3, 2, 21), _spec(TPS2, 1, 40, 3, 2, 22), _spec(CUBIC3, 0, 33, 5, 1, 23)]
    specs[1]["C"][-1] = specs[1]["C"][-2]     # a duplicated site: two equal rows of the saddle matrix
    rc_off, m_off = single(ctx, specs[1])     # the option is still off: what fit_lu says of this start
    assert rc_off != 0 and m_off is None
    ctx.set_option(_lib.OPT_SMALL_LU, 1)
    refs = [single(ctx, s) for s in specs]
    assert refs[1][0] == rc_off and refs[0][0] == 0 and refs[2][0] == 0
    got = batch(ctx, specs)
    assert got[1][0] == rc_off and got[1][1] is None
    for p in (0, 2):
        assert _took_the_one_launch_lu(got[p][1].info)
        assert_same(got[p], refs[p], ("neighbour", p), lu=True)
    _free(got), _free(refs)


def test_exactly_singular_start_among_three(ctx):
    """all sites of the middle start in the plane x_3 = 0: a zero column of Pi, an exactly zero pivot on either path"""
    specs = [_spec(TPS2, 1, 40, 3, 2, 21), _spec(TPS2, 1, 40, 3, 2, 22), _spec(CUBIC3, 0, 33, 5, 1, 23)]
    specs[1]["C"][:, 2] = 0.0
    rc_off, m_off = single(ctx, specs[1])
    assert rc_off != 0 and m_off is None
    ctx.set_option(_lib.OPT_SMALL_LU, 1)
    refs = [single(ctx, s) for s in specs]
    assert refs[1][0] == rc_off and refs[0][0] == 0 and refs[2][0] == 0
    got = batch(ctx, specs)
    assert got[1][0] == rc_off and got[1][1] is None
    for p in (0, 2):
        assert _took_the_one_launch_lu(got[p][1].info)
        assert_same(got[p], refs[p], ("neighbour", p), lu=True)
    _free(got), _free(refs)


def test_handles_are_ordinary_models(lu_ctx):
    ns, d = 4, 3
    specs = [_spec(TPS2, 1, 40 + 3 * p, d, 2, seed=300 + p) for p in range(ns)]
    got = batch(lu_ctx, specs)
    assert all(rc == 0 and _took_the_one_launch_lu(m.info) for rc, m in got)
    for s, (_, m) in zip(specs, got):
        V, _ = m.eval_sites(s["C"])
        assert np.abs(V - s["Y"]).max() <= 1e-9 * np.abs(s["Y"]).max()      # the surrogate interpolates at its sites
    rng = np.random.default_rng(55)
    X = rng.uniform(-1.0, 1.0, (ns, d))
    plans = [sg.container_plan(sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])])) for _, m in got]
    rc, D, XP, MXP, recs, ms = descent.sd_iterate_batch_device(plans, descent.SteepestDescentConfig(), X, X + rng.uniform(-0.02, 0.02, (ns, d)),
                                                                np.full(ns, 0.3), np.full(d, -2.0), np.full(d, 2.0), None)
    assert rc == 0 and all(r["sd_status"] == _lib.SD_OK for r in recs), (rc, recs)
    assert np.all(np.isfinite(XP)) and np.all(np.isfinite(MXP))
    _free(got)


def test_bindings_raise_and_restore_the_option(ctx):
    ns, n, d = 8, 33, 16
    cfg = pkg.RbfConfig(kernel="thin_plate_spline", polynomial_degree=1)
    data = [_data(n, d, 2, seed=70 + p) for p in range(ns)]
    admitted = ctx.lib.mrbf_dispatch_fit_batch_lu(ns, n, d) == 1
    stats = {}
    mods = pkg.update_models_many(cfg, [C for C, _ in data], [Y for _, Y in data], 1.0, ctx=ctx, stats=stats)
    assert stats["path"] == "batch" and stats["status"] == [0] * ns
    assert stats["lu"] == (ns if admitted else 0)
    assert ctx.get_option(_lib.OPT_SMALL_LU) == 0
    assert all(_took_the_one_launch_lu(m.info) == admitted for m in mods)
    for m in mods:
        m.free()
    # a job fails (its sites in a hyperplane: a zero column of Pi): its status says so, the others have their models, the option is back at 0
    data[2][0][:, 3] = 0.0
    stats = {}
    mods = pkg.update_models_many(cfg, [C for C, _ in data], [Y for _, Y in data], 1.0, ctx=ctx, stats=stats)
    assert stats["status"][2] != 0 and mods[2] is None and sum(1 for m in mods if m is not None) == ns - 1
    assert ctx.get_option(_lib.OPT_SMALL_LU) == 0
    for m in mods:
        if m is not None:
            m.free()
