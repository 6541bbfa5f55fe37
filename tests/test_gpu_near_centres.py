"""Evaluation, Gram assembly and fit at queries and sites NEAR a centre (run with -m gpu): the regime of the trust-region method's late
iterations -- the iterate is a training site, trial points lie within 1e-4 .. 1e-12 of it -- while the coordinates stay O(1).

The reference is the difference form in extended precision (tests/near_centre_util.py; checked on the CPU by
tests/test_near_centre_reference.py, where a NumPy GEMM-form evaluator fails this file's checker for cubic beta = 1 by eight orders of
magnitude).  The bounds are the suite's own for the evaluation alone (test_eval_from_golden_coeffs_isolated_from_solve), per output
column; the Gram bar is test_gram_matches_golden's 2e-13; the fit's asserts are those of test_fit_and_eval_match_golden.

Part 1 runs every evaluation-kernel variant (near_centre_util.VARIANTS: D = 64 / 128 / 256, finished in the kernel or split + combine,
and d > 256) with every family of radial function, values + Jacobians and values only.  Cubic beta = 1 and thin plate spline k = 1 --
not smooth at 0 -- take the difference-form kernels (kp_nonsmooth, DESIGN.md "Distances near a centre"); the others stay in GEMM form
and are pinned here as robust.  The module writes near_centre_report.json -- error / bound per case and per delta -- into
the directory that MRBF_REPORT_DIR names (default: test_reports/ in the repository root, kept out of git), as
tests/test_gpu_many_outputs.py writes its report."""
import json
import os

import numpy as np
import pytest

from tests import near_centre_util as u
from tests.conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib
from oracle import rbf_oracle as orc

EPS = np.finfo(np.float64).eps
W_TOL = 1e-10           # BASELINE.json north_star: interpolation weights, relative
WELL_CONDITIONED = 1e6  # below this condition number the 1e-10 bar is asserted outright (tests/test_gpu_parity.py)
REPORT = {}


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()
    out = os.environ.get("MRBF_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "near_centre_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def _cfg(kernel):
    name, sp = u.KERNELS[kernel]
    return pkg.RbfConfig(kernel=name, shape_parameter=sp, polynomial_degree=u.DEG)


# ---- 1. evaluation alone: model_from_coeffs + eval_sites ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(u.KERNELS))
@pytest.mark.parametrize("variant", sorted(u.VARIANTS))
def test_eval_near_centres(ctx, variant, kernel):
    case = u.near_centre_case(variant, kernel)
    cfg = _cfg(kernel)
    assert pkg.rbf_model._get_kernel_params(1.0, cfg) == (case.kid, case.a, case.b)
    mod = pkg.model_from_coeffs(cfg, case.C, case.W, case.Lam, ctx=ctx)
    try:
        V, J = mod.eval_sites(case.X, want_values=True, want_jac=True)
        V_only, none = mod.eval_sites(case.X, want_values=True, want_jac=False)   # the pass of the backtracking and the PS populations
    finally:
        mod.free()
    assert none is None and V.shape == (43, case.k) and J.shape == (43, case.k, case.d)
    ev, ej = u.errors_over_bound(case.W, case.n, case.V_ref, case.J_ref, V, J)
    ev_only, _ = u.errors_over_bound(case.W, case.n, case.V_ref, case.J_ref, V_only, None)
    rec = dict(d=case.d, n=case.n, k=case.k, v=u.by_delta(case, ev), j=u.by_delta(case, ej), v_only=u.by_delta(case, ev_only),
               v_worst=float(ev.max()), j_worst=float(ej.max()), v_only_worst=float(ev_only.max()))
    REPORT.setdefault("eval", {}).setdefault(variant, {})[kernel] = rec
    print(variant, kernel, json.dumps(rec))
    assert np.isfinite(V).all() and np.isfinite(J).all() and np.isfinite(V_only).all(), (variant, kernel)
    # every query, every output column, both calls
    assert ev.max() < 1.0, (variant, kernel, int(ev.argmax()), float(case.delta[ev.argmax()]), ev.max())
    assert ej.max() < 1.0, (variant, kernel, int(ej.argmax()), float(case.delta[ej.argmax()]), ej.max())
    assert ev_only.max() < 1.0, (variant, kernel, int(ev_only.argmax()), float(case.delta[ev_only.argmax()]), ev_only.max())
    # the query ON a centre: the Jacobian follows the oracle's convention (beta = 1, k = 1: the coincident term contributes nothing;
    # J_ref is built that way), and the values of the two calls are the same bits wherever the suite observes that across passes
    # (d <= 256: test_gpu_configs.py, test_eval_alone_launch_shapes; d > 256: its 1e-12)
    on = case.delta == 0
    assert ej[on].max() < 1.0 and ev[on].max() < 1.0, (variant, kernel, ej[on].max(), ev[on].max())
    if case.d <= 256:
        assert np.array_equal(V, V_only), (variant, kernel)   # (all 43 queries, those on a centre among them)
    else:
        dv = (np.abs(V - V_only).max(axis=0) / np.maximum(1.0, np.abs(V).max(axis=0))).max()
        assert dv < 1e-12, (variant, kernel, dv)


# ---- 2. Gram assembly on clustered sites, both modes ------------------------------------------------------------------------------
GRAM_SITES = {"d20_n120_r1e-3": (20, 120, 1e-3), "d20_n120_r1e-4": (20, 120, 1e-4), "d6_n60_r1e-4": (6, 60, 1e-4),
              "d20_n300_r1e-3": (20, 300, 1e-3)}   # n = 300: x0 in tile 0, cluster members in tile 1 -- close pairs in an off-diagonal tile pair
GRAM_KERNELS = ("cubic1", "cubic3", "tps1", "multiquadric")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sites", sorted(GRAM_SITES))
def test_gram_on_clustered_sites(ctx, sites, mode):
    d, n, radius = GRAM_SITES[sites]
    C = u.clustered_sites(d, n, radius)
    q = d + 1
    ctx.set_option(_lib.OPT_GRAM_MODE, mode)
    try:
        for kernel in GRAM_KERNELS:
            kid, a, b = u.kernel_ids(kernel)
            ref, Pi_ref = orc.gram(C, kid, a, b, u.DEG)
            Phi = np.full((n, n), np.nan, order="F")
            Pi = np.full((n, q), np.nan, order="F")
            ctx.check(ctx.lib.mrbf_gram(ctx.h, n, d, _lib.as_ptr(C), kid, a, b, u.DEG, _lib.as_ptr(Phi), _lib.as_ptr(Pi), None))
            err = float(np.abs(Phi - ref).max() / max(1.0, np.abs(ref).max()))
            REPORT.setdefault("gram", {}).setdefault(sites, {})["%s_mode%d" % (kernel, mode)] = err
            print(sites, kernel, mode, err)
            assert np.isfinite(Phi).all(), (sites, kernel, mode)
            assert err < 2e-13, (sites, kernel, mode, err)
            assert np.array_equal(Phi, Phi.T), (sites, kernel, mode)                       # exactly symmetric
            assert np.all(np.diag(Phi) == orc.phi(kid, a, b, 0.0)), (sites, kernel, mode)  # diagonal = phi(0)
            assert np.array_equal(Pi, Pi_ref), (sites, kernel, mode)
    finally:
        ctx.set_option(_lib.OPT_GRAM_MODE, 0)


# ---- 3. fit on clustered sites, then the fitted model at x0 and at x0 + delta u ------------------------------------------------------
def _backward_error(S, Y, W, Lam):
    """normwise backward error of [W; Lam] in the ORACLE's saddle system (Rigal-Gaches, Frobenius norms), as tests/test_gpu_parity.py"""
    x = np.vstack([W, np.asarray(Lam).reshape(-1, W.shape[1])])
    b = np.vstack([Y, np.zeros((x.shape[0] - Y.shape[0], Y.shape[1]))])
    return float(np.linalg.norm(S @ x - b) / (np.linalg.norm(S) * np.linalg.norm(x) + np.linalg.norm(b)))


@pytest.mark.parametrize("n", [120, 600])
@pytest.mark.parametrize("kernel", ["cubic1", "cubic3"])
def test_fit_on_clustered_sites(ctx, kernel, n):
    d, k = 20, 2
    C = u.clustered_sites(d, n, 1e-3)
    Y = u.cluster_values(C, k)
    kid, a, b = u.kernel_ids(kernel)
    Phi, Pi = orc.gram(C, kid, a, b, u.DEG)
    S = orc.saddle_matrix(Phi, Pi)
    cond = float(np.linalg.cond(S))
    ref = orc.fit(C, Y, kid, a, b, u.DEG)
    mod = pkg.update_model(_cfg(kernel), C, Y, ctx=ctx)
    try:
        be = _backward_error(S, Y, mod.weights, mod.poly)
        ew = float(np.abs(mod.weights - ref.w).max() / np.abs(ref.w).max())
        rec = dict(n=n, cond=cond, path=mod.info["path"], fallbacks=mod.info["fallbacks"], backward_error=be, w=ew,
                   rel_residual=mod.info["rel_residual"])
        REPORT.setdefault("fit", {})["%s_n%d" % (kernel, n)] = rec
        assert np.isfinite(mod.weights).all() and np.isfinite(mod.poly).all(), (kernel, n)
        assert be <= 50 * EPS, (kernel, n, be)
        assert mod.info["rel_residual"] < 1e-11, (kernel, n, mod.info)
        if kernel == "cubic3":
            # the control: cond 7.5e10 (n = 120) / 1.1e12 (n = 600) -- backward error and residual only
            print(kernel, n, json.dumps(rec))
            return
        # cubic beta = 1 with a linear tail: cond 1.4e5 (n = 120) / 8.4e5 (n = 600), under the outright 1e-10 rule -- a condition on the
        # INPUT (tests/test_near_centre_reference.py holds the first in place on the CPU)
        assert cond < WELL_CONDITIONED, (kernel, n, cond)
        assert ew < W_TOL, (kernel, n, ew, cond)
        # the fitted model at x0 and next to it, against the extended-precision difference form on the GPU's own coefficients
        X = u.step_queries(C[0])
        V_ref, J_ref = u.reference_eval(C, mod.weights, mod.poly, kid, a, b, u.DEG, X)
        V, J = mod.eval_sites(X, want_values=True, want_jac=True)
        V_only, _ = mod.eval_sites(X, want_values=True, want_jac=False)
        ev, ej = u.errors_over_bound(mod.weights, n, V_ref, J_ref, V, J)
        ev_only, _ = u.errors_over_bound(mod.weights, n, V_ref, J_ref, V_only, None)
        rec.update(w_max=float(np.abs(mod.weights).max()), v={"%g" % dl: float(e) for dl, e in zip(u.DELTAS, ev)},
                   j={"%g" % dl: float(e) for dl, e in zip(u.DELTAS, ej)}, v_only={"%g" % dl: float(e) for dl, e in zip(u.DELTAS, ev_only)})
        print(kernel, n, json.dumps(rec))
        assert np.isfinite(V).all() and np.isfinite(J).all() and np.isfinite(V_only).all(), (kernel, n)
        assert ev.max() < 1.0 and ej.max() < 1.0 and ev_only.max() < 1.0, (kernel, n, ev.max(), ej.max(), ev_only.max())
        # x0 is a training site: the model interpolates there
        assert np.abs(V[0] - Y[0]).max() < 1e-8 * max(1.0, np.abs(Y).max()), (kernel, n, V[0], Y[0])
    finally:
        mod.free()


# ---- 4. members of a batch: the descent chain's grouped evaluations ----------------------------------------------------------------
def test_batched_evaluations_of_nonsmooth_models_match_the_single_calls():
    """mrbf_sd_iterate_batch groups the evaluations of its starts by parameterisation: the two cubic beta = 1 starts (40 and 57 centres)
    form one launch group, which eval_fused_batch hands to the difference-form kernel with the start on a grid dimension; beta = 5 and
    beta = 3 form others and stay in GEMM form.  Every start sits ON a training site with x 1e-9 away, and reproduces the chain of its
    own single calls bit for bit -- whose evaluation part 1 holds against the reference."""
    from morbit.jl_amd import descent
    from morbit.jl_amd import surrogates as sg
    from tests import test_gpu_sd_batch as sb

    d = 3
    rng = np.random.default_rng(191)

    def fit(n, beta):
        C = rng.uniform(-1.5, 1.5, (n, d))
        cfgm = pkg.RbfConfig(kernel="cubic", shape_parameter=beta, polynomial_degree=1)
        return C, pkg.update_model(cfgm, C, np.stack([sb.base.f_a(C), sb.base.f_b(C)], axis=1))

    fits = [fit(40, 1.0), fit(57, 5.0), fit(57, 1.0), fit(40, 5.0), fit(40, 3.0)]
    mods = [m for _, m in fits]
    try:
        scs = [sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])]) for m in mods]
        lb, ub = np.full(d, -2.0), np.full(d, 2.0)
        X_n = np.array([C[0] for C, _ in fits])
        X = X_n + 1e-9 * rng.standard_normal(X_n.shape)
        deltas = np.full(len(mods), 0.3)
        cfg = descent.SteepestDescentConfig()
        ref = sb.chain(cfg, scs, X, X_n, deltas, lb, ub, None)
        sb.assert_identical(sb.batch(cfg, scs, X, X_n, deltas, lb, ub, None), ref)
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.isfinite(ref[2]).all()
    finally:
        for m in mods:
            m.free()
