"""CPU tests of the reference and the checker behind tests/test_gpu_hessian.py (tests/hessian_util.py): the long-double difference-form
Hessian against a 50-digit mpmath evaluation whose phi' and phi'' come from phi by mpmath.diff; that the checker bites (an fp64
GEMM-form evaluator fails it near a centre for the radial functions whose curvature term is unbounded at 0, and passes where it
should); the trace identity; and the h^2 convergence of central differences of the reference Jacobian.  No GPU."""
import numpy as np
import pytest

from tests import hessian_util as hu
from tests.near_centre_util import KERNELS

DELTAS = (0.0, 1e-12, 1e-8, 1e-4, 0.3)


def _case(kernel, d, n, seed=0):
    kid, a, b = hu.kernel_ids(kernel, d)
    C, W, rng = hu.random_model(d, n, 2, 100 + d + seed)
    X = hu.near_queries(C, [n // 2], DELTAS, rng)
    return kid, a, b, C, W, X


def _ld_to_mp(x):
    import mpmath as mp

    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - hu.LD(hi)))


@pytest.mark.parametrize("d, n", [(5, 30), (17, 40)])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_long_double_reference_against_mpmath(kernel, d, n):
    import mpmath as mp

    kid, a, b, C, W, X = _case(kernel, d, n)
    H, S = hu.reference_hessian(C, W, kid, a, b, X)       # long double where that is the x87 format: what the GPU tests compare with
    Hm, Sm = hu.reference_hessian_mp(C, W, kid, a, b, X)
    worst = mp.mpf(0)
    with mp.workdps(50):
        f = mp.mpf(hu.factor(n, d))
        for h, s, hm, sm in zip(H.ravel(), S.ravel(), Hm.ravel(), Sm.ravel()):
            if sm == 0:
                assert h == 0 and hm == 0
                continue
            worst = max(worst, abs(_ld_to_mp(h) - hm) / (f * sm))
            assert abs(_ld_to_mp(s) - sm) <= mp.mpf(1e-15) * sm        # the bound's own sum is the same sum
    print(kernel, d, "long double against mpmath: %.2e of the bound" % float(worst))
    assert worst < 1e-3
    assert np.isfinite(H.astype(np.float64)).all()


@pytest.mark.parametrize("kernel, delta, passes", [("cubic1", 1e-8, False), ("tps1", 1e-8, False), ("cubic3", 1e-8, False), ("cubic5", 0.3, True)])
def test_the_checker_bites(kernel, delta, passes):
    d, n = 17, 40
    kid, a, b, C, W, X = _case(kernel, d, n)
    X = X[[DELTAS.index(delta)]]
    H_ref, S = hu.reference_hessian(C, W, kid, a, b, X)
    worst = float(hu.errors_over_bound(hu.gemm_form_hessian(C, W, kid, a, b, X), H_ref, S, n, d).max())
    print(kernel, delta, "GEMM form in fp64: %.2e of the bound" % worst)
    assert (worst < 1.0) == passes
    # the reference itself, rounded to fp64, passes; a NaN or an entry one bound off does not
    H64 = H_ref.astype(np.float64)
    assert hu.errors_over_bound(H64, H_ref, S, n, d).max() < 1.0
    bad = H64.copy()
    bad[0, 1, 3, 4] += 1.5 * hu.factor(n, d) * float(S[0, 1, 3, 4])
    assert hu.errors_over_bound(bad, H_ref, S, n, d).max() > 1.0
    bad = H64.copy()
    bad[0, 0, 0, 0] = np.nan
    assert np.isinf(hu.errors_over_bound(bad, H_ref, S, n, d).max())


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_trace_identity(kernel):
    """tr H_l = sum_c w_cl (d psi_c + s_c chi_c)"""
    d, n = 17, 40
    kid, a, b, C, W, X = _case(kernel, d, n, seed=1)
    H, S = hu.reference_hessian(C, W, kid, a, b, X)
    for p in range(X.shape[0]):
        diff = X[p].astype(hu.LD)[None, :] - C.astype(hu.LD)
        s = (diff * diff).sum(axis=1)
        psi, chi = hu.psi_chi_ld(kid, a, b, s)
        want = ((d * psi + s * chi)[:, None] * W.astype(hu.LD)).sum(axis=0)
        got = np.trace(H[p], axis1=1, axis2=2)
        scale = np.trace(S[p], axis1=1, axis2=2)
        assert (np.abs(got - want) <= 64 * n * np.finfo(hu.LD).eps * scale).all(), (kernel, p)


def test_central_differences_of_the_reference_jacobian_converge_as_h_squared():
    d, n = 5, 30
    kid, a, b = hu.kernel_ids("gaussian", d)
    C, W, rng = hu.random_model(d, n, 2, 3)
    x = 0.25 + 0.5 * rng.random((1, d))
    H, _ = hu.reference_hessian_ld(C, W, kid, a, b, x)
    errs = []
    for h in (1e-2, 5e-3, 2.5e-3):
        Xpm = np.concatenate([x + h * np.eye(d), x - h * np.eye(d)])
        step = (Xpm[:d] - Xpm[d:])[np.arange(d), np.arange(d)].astype(hu.LD)
        J = hu.reference_jacobian_ld(C, W, kid, a, b, Xpm)                # (2 d, k, d)
        fd = np.transpose((J[:d] - J[d:]) / step[:, None, None], (1, 2, 0))   # [l, i, j]
        errs.append(float(np.abs(fd - H[0]).max()))
    print(errs)
    assert 3.8 < errs[0] / errs[1] < 4.2 and 3.8 < errs[1] / errs[2] < 4.2


def test_variants_table_is_well_formed():
    for name, (d, n, m, k, kind, why) in hu.VARIANTS.items():
        assert d >= 1 and n >= 1 and m in (1, 2, 63, 64, 65) and k in (1, 2, 3, 17) and kind in ("all", "last", "rep") and why
        assert not (d >= 140 and m > 5)
        rows = hu.variant_rows(k, kind)
        assert rows is None or all(0 <= l < k for l in rows)
    assert {v[0] for v in hu.VARIANTS.values()} == {1, 3, 15, 16, 17, 64, 65, 140, 300}
    assert {v[1] for v in hu.VARIANTS.values()} >= {1, 3, 4, 5, 63, 64, 65, 257, 300}
