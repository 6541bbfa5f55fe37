"""CPU checks of tests/near_centre_util.py (no GPU): the extended-precision reference against mpmath, the fp64 oracle inside the bounds
on its own, the checker's teeth (a NumPy GEMM-form evaluator must fail where the formula says it fails), and the conditioning of the
clustered sites that tests/test_gpu_near_centres.py fits."""
import numpy as np
import pytest

from oracle import rbf_oracle as orc
from tests import near_centre_util as u


def _mp_minus_ld(A_mp, A_ld):
    """|A_mp - A_ld| as float64, the longdouble taken exactly (as the sum of two doubles)"""
    import mpmath as mp

    hi = A_ld.astype(np.float64)
    lo = (A_ld - hi.astype(u.LD)).astype(np.float64)
    with mp.workdps(50):
        f = np.frompyfunc(lambda t, h, l: float(abs(t - (mp.mpf(float(h)) + mp.mpf(float(l))))), 3, 1)
        return f(A_mp, hi, lo).astype(np.float64)


@pytest.mark.parametrize("kernel", sorted(u.KERNELS))
def test_reference_matches_mpmath(kernel):
    case = u.near_centre_case("d64_final", kernel)
    V_mp, J_mp = u.reference_eval_mp(case.C, case.W, case.Lam, case.kid, case.a, case.b, case.deg, case.X, 50)
    bv, bj = u.bounds(case.W, case.n, case.V_ref, case.J_ref)
    ev = (_mp_minus_ld(V_mp, case.V_ref) / bv[None, :]).max()
    ej = (_mp_minus_ld(J_mp, case.J_ref) / bj[None, :, None]).max()
    print(kernel, "reference vs mpmath, error / bound:", ev, ej)
    assert np.isfinite(case.V_ref.astype(np.float64)).all() and np.isfinite(case.J_ref.astype(np.float64)).all()
    assert ev <= 0.01 and ej <= 0.01, (kernel, ev, ej)


@pytest.mark.parametrize("variant", sorted(u.VARIANTS))
def test_fp64_oracle_stays_inside_the_bounds(variant):
    # the difference form needs no extended precision to meet the bounds: what is asked of the device code is attainable in fp64
    for kernel in sorted(u.KERNELS):
        case = u.near_centre_case(variant, kernel)
        om = orc.OracleModel(case.C, case.W, case.Lam, case.kid, case.a, case.b, case.deg)
        V = np.array([om.value(x) for x in case.X])
        J = np.array([om.jac(x) for x in case.X])
        ev, ej = u.errors_over_bound(case.W, case.n, case.V_ref, case.J_ref, V, J)
        print(variant, kernel, "fp64 oracle, error / bound:", ev.max(), ej.max())
        assert ev.max() <= 0.01 and ej.max() <= 0.01, (variant, kernel, ev.max(), int(ev.argmax()), ej.max(), int(ej.argmax()))


@pytest.mark.parametrize("variant", sorted(u.VARIANTS))
def test_checker_rejects_the_gemm_form_where_it_is_wrong(variant):
    for kernel, must_fail in (("cubic1", True), ("cubic3", False), ("gaussian", False)):
        case = u.near_centre_case(variant, kernel)
        V, J = u.gemm_form_eval(case)
        ev, ej = u.errors_over_bound(case.W, case.n, case.V_ref, case.J_ref, V, J)
        print(variant, kernel, "GEMM form, error / bound:", ev.max(), ej.max())
        if must_fail:
            assert max(ev.max(), ej.max()) > 1.0, (variant, kernel, ev.max(), ej.max())
            far = case.target < 0
            assert ev[far].max() < 1.0 and ej[far].max() < 1.0, (variant, kernel)   # ... and only near the centres
        else:
            assert ev.max() < 1.0 and ej.max() < 1.0, (variant, kernel, ev.max(), ej.max())


def test_case_layout():
    case = u.near_centre_case("d64_split", "gaussian")
    assert case.X.shape == (43, 64) and case.targets == (0, 63, 64, 299)
    assert (case.delta == 0).sum() == 5 and (case.target < 0).sum() == u.N_FAR
    for i in np.flatnonzero(case.delta == 0):
        assert np.array_equal(case.X[i], case.C[case.target[i]])
    # the axis-direction queries differ from centre 0 in the first coordinate only
    ax = case.X[28:35]
    assert np.array_equal(ax[:, 1:], np.broadcast_to(case.C[0, 1:], ax[:, 1:].shape)) and np.all(case.target[28:35] == 0)
    assert np.abs(case.W).max() == 1.0 and np.all(np.abs(case.W[list(case.targets)]) == 1.0)


def test_clustered_sites_are_well_conditioned_for_cubic1():
    # cubic beta = 1 with a linear tail on the late-iteration geometry: below the 1e6 under which the suite asserts the weights outright
    C = u.clustered_sites(20, 120, 1e-3)
    assert C.shape == (120, 20) and np.abs(C[1:60] - C[0]).max() <= 1e-3 and np.abs(C[60:] - C[0]).max() > 0.1
    Phi, Pi = orc.gram(C, 0, 1.0, 0.0, 1)
    cond = float(np.linalg.cond(orc.saddle_matrix(Phi, Pi)))
    print("cond of the saddle system, clustered_sites(20, 120, 1e-3), cubic beta = 1:", cond)
    assert cond < 1e6, cond
