"""CPU tests of directed search (descent.jl:583-664): the host method of the direction QP (morbit.jl_amd/descent.py, the NumPy form of
the active-set method that ds_qp.hip runs) against SciPy's SLSQP on seeded QPs, its statuses, the unconstrained branch, the decision
table's rows, the struct mirrors, and the host logic of the device call (tools/ds_host_check.cpp, a stand-alone program under
AddressSanitizer and UBSan, run as a child process).  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import ds_util
from tests.conftest import ROOT

SHAPES = [(d, k) for d in (1, 2, 3, 7, 30, 64, 65, 130) for k in (1, 2, 3, 5)]   # the shapes of the issue's prototype


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


@pytest.mark.parametrize("d,k", SHAPES)
def test_host_method_against_slsqp(d, k):
    """f <= f_SLSQP + 1e-9 (1 + f): SLSQP's own stopping slack is the margin.  Measured on these QPs: the host method's value is
    within 2e-13 (relative, 1 + f) of SLSQP's, or below it; at most 2.0 (d + k) iterations."""
    from morbit.jl_amd import _lib, descent

    G, r, X, lb, ub = ds_util.make_batch(d, k, n_qp=10)
    worst, most = -np.inf, 0.0
    for p in range(10):
        lo, hi = descent._sd_box(X[p], lb, ub)
        st = {}
        dd, z, om, mu, status = descent._directed_search_direction(X[p], G[p], r[p], lb, ub, stats=st)
        assert status == _lib.DS_OK and st["method"] == "active_set", (d, k, p, status, st)
        ds_util.check_solution(G[p], r[p], lo, hi, dd, z, om, mu, (d, k, p))
        f = ds_util.value(G[p], r[p], dd)
        _, fs = ds_util.slsqp(G[p], r[p], lo, hi)
        worst, most = max(worst, (f - fs) / (1 + f)), max(most, st["iterations"] / (d + k))
        assert f <= fs + 1e-9 * (1 + f), (d, k, p, f, fs)
        assert st["iterations"] <= 8 * (d + k) + 16
    print("d = %d, k = %d: (f - f_SLSQP) / (1 + f) <= %.1e, iterations <= %.2f (d + k)" % (d, k, worst, most))


def test_more_rows_than_variables_is_no_cycle():
    """16 rows through the origin of 7 variables: the cone G d <= 0 is the origin alone, every step has length zero.  The most
    violating multiplier cycles there; the least-index rule after a step of length zero ends it."""
    from morbit.jl_amd import _lib, descent

    G, r, X, lb, ub = ds_util.make_batch(7, 16)
    for p in range(ds_util.N_QP):
        lo, hi = descent._sd_box(X[p], lb, ub)
        st = {}
        dd, z, om, mu, status = descent._ds_active_set(G[p], r[p], lo, hi, st)
        assert status == _lib.DS_OK, (p, st)
        ds_util.check_solution(G[p], r[p], lo, hi, dd, z, om, mu, (7, 16, p))


def test_critical_infeasible_and_gave_up():
    from morbit.jl_amd import _lib, descent

    rng = np.random.default_rng(3)
    G = rng.standard_normal((3, 5))
    x, lb, ub = np.full(5, 0.5), np.zeros(5), np.ones(5)
    for bad in (0.0, 0.3, np.nan):
        r = np.array([-1.0, bad, -0.5])
        dd, z, om, mu, status = descent._directed_search_direction(x, G, r, lb, ub)
        assert status == _lib.DS_CRITICAL and not dd.any() and not z.any() and om == 0.0 and not mu.any()
    r = np.array([-1.0, -0.2, -0.5])
    for xo in (np.array([0.5, 0.5, -1.5, 0.5, 0.5]), np.array([0.5, 2.5, 0.5, 0.5, 0.5])):   # l_j > u_j: more than one outside
        dd, z, om, mu, status = descent._directed_search_direction(xo, G, r, lb, ub)
        assert status == _lib.DS_INFEASIBLE and not dd.any() and om == -np.inf
    # CRITICAL is decided before the box is looked at, as the reference returns before it forms the problem (descent.jl:615-617)
    assert descent._directed_search_direction(np.full(5, 3.0), G, np.array([1.0, -1.0, -1.0]), lb, ub)[4] == _lib.DS_CRITICAL
    # x outside [lb, ub] by less than one: d = 0 is no start for the active-set method (GAVE_UP), the routed host method takes SLSQP
    xs = np.array([0.5, 0.5, -0.25, 0.5, 0.5])
    lo, hi = descent._sd_box(xs, lb, ub)
    st = {}
    assert descent._ds_active_set(G, r, lo, hi, st)[4] == _lib.DS_GAVE_UP and st["gave_up"] == "start"
    st = {}
    dd, z, om, mu, status = descent._directed_search_direction(xs, G, r, lb, ub, stats=st)
    assert st["method"] == "slsqp"
    if status == _lib.DS_OK:
        assert np.all(dd >= lo) and np.all(dd <= hi) and dd[2] >= 0.25


@pytest.mark.parametrize("d,k,cond", [(3, 2, 10.0), (7, 3, 1e3), (30, 5, 1e3), (130, 5, 1e2)])
def test_interior_case_is_the_pseudo_inverse(d, k, cond):
    """box and rows inactive, G of full row rank with cond_2 <= 1e3, ||G^+ r||_inf < 1: d = G^+ r within 1e-10 relative
    (cond^2 2^-52 with room) -- the unconstrained branch of descent.jl:623-626"""
    from morbit.jl_amd import _lib, descent

    rng = np.random.default_rng(d * 100 + k)
    U, _ = np.linalg.qr(rng.standard_normal((k, k)))
    V, _ = np.linalg.qr(rng.standard_normal((d, k)))
    sv = np.geomspace(1.0, 1.0 / cond, k)
    G = (U * sv) @ V.T
    assert np.linalg.cond(G) <= 1e3 * (1 + 1e-9)
    r = -rng.uniform(0.2, 1.0, k)
    ref = np.linalg.pinv(G) @ r
    r *= 0.4 / np.max(np.abs(ref))
    ref = np.linalg.pinv(G) @ r
    assert np.max(np.abs(ref)) < 1 and np.all(r < 0)
    x, lb, ub = np.zeros(d), np.full(d, -5.0), np.full(d, 5.0)
    dd, z, om, mu, status = descent._directed_search_direction(x, G, r, lb, ub)
    assert status == _lib.DS_OK
    err = np.linalg.norm(dd - ref) / np.linalg.norm(ref)
    print("d = %d, k = %d, cond %.0e: |d - G^+ r| / |G^+ r| = %.1e" % (d, k, cond, err))
    assert err <= 1e-10
    assert not mu.any() and om == max(0.0, -float(np.max(z)))


def test_constraint_rows_take_slsqp():
    from morbit.jl_amd import _lib, descent

    rng = np.random.default_rng(8)
    d, k = 6, 2
    G = rng.standard_normal((k, d))
    r = -rng.uniform(0.2, 1.0, k)
    x, lb, ub = np.full(d, 0.5), np.zeros(d), np.ones(d)
    A_in, b_in = rng.standard_normal((2, d)), np.array([0.05, 0.1])
    A_eq, b_eq = np.ones((1, d)), np.zeros(1)
    st = {}
    dd, z, om, mu, status = descent._directed_search_direction(x, G, r, lb, ub, A_eq, b_eq, A_in, b_in, stats=st)
    assert status == _lib.DS_OK and st["method"] == "slsqp"
    lo, hi = descent._sd_box(x, lb, ub)
    assert np.all(dd >= lo) and np.all(dd <= hi) and np.all(G @ dd <= 1e-9)
    assert abs(float((A_eq @ dd)[0])) <= 1e-9 and np.all(A_in @ dd <= b_in + 1e-9)
    free, _, _, _, s0 = descent._directed_search_direction(x, G, r, lb, ub)
    assert s0 == _lib.DS_OK and ds_util.value(G, r, free) <= ds_util.value(G, r, dd) + 1e-12   # rows can only cost


def test_config_mirrors_the_reference_fields():
    from morbit.jl_amd import descent

    cfg = descent.DirectedSearchConfig()
    sd = descent.SteepestDescentConfig()
    for f in ("strict_backtracking", "armijo_const_rhs", "armijo_const_shrink", "min_stepsize", "max_loops"):
        assert getattr(cfg, f) == getattr(sd, f), f
    assert list(cfg.reference_point) == [] and list(cfg.reference_direction) == [] and cfg.max_ideal_point_problem_evals == -1
    assert cfg.reference_algo == "GN_ISRES"
    with pytest.raises(AssertionError):
        descent.DirectedSearchConfig(reference_direction=[1.0, -1.0])
    # r is minus the direction of _get_global_dir (descent.jl:599-611)
    r = descent._ds_image_direction(descent.DirectedSearchConfig(reference_direction=[1.0, 2.0]), None, None, None, np.zeros(3), [5.0, 5.0], 1.0,
                                    None, None, None, None)
    assert np.array_equal(r, [-1.0, -2.0])
    r = descent._ds_image_direction(descent.DirectedSearchConfig(reference_point=[1.0, 2.0]), None, None, None, np.zeros(3), [5.0, 5.0], 1.0,
                                    None, None, None, None)
    assert np.array_equal(r, [-4.0, -3.0])


def test_decision_table_rows(lib):
    from morbit.jl_amd import _lib

    D, R = _lib.DISPATCH_DEVICE, _lib.DISPATCH_REFERENCE
    f = lib.mrbf_dispatch_ds   # (d, k, n_models, n_nl, n_lin, n_foreign)
    assert f(7, 2, 1, 0, 0, 0) == D and f(1, 1, 1, 0, 0, 0) == D and f(4096, 16, 8, 0, 0, 0) == D
    assert f(7, 2, 1, 0, 0, 1) == R            # a foreign surrogate
    assert f(7, 2, 0, 0, 0, 0) == R            # no device model
    assert f(0, 2, 1, 0, 0, 0) == R and f(4097, 2, 1, 0, 0, 0) == R
    assert f(7, 0, 1, 0, 0, 0) == R and f(7, 17, 1, 0, 0, 0) == R
    assert f(7, 2, 1, 1, 0, 0) == R and f(7, 2, 1, 0, 1, 0) == R      # modelled / linear constraints: the host method
    assert f(7, 2, 1, -1, 0, 0) == R and f(7, 2, 1, 0, -1, 0) == R
    assert _lib.ENTRY_DS == 22
    assert lib.mrbf_dispatch_after(_lib.ENTRY_DS, -2) == 1
    for rc in (0, -1, -3, -4, -8, _lib.MRBF_EHIP, _lib.MRBF_ENOMEM):
        assert lib.mrbf_dispatch_after(_lib.ENTRY_DS, rc) == 0


def test_refusals_that_need_no_device(lib):
    assert lib.mrbf_ds_direction(None, 1, 2, 2, *([None] * 11)) == -1
    assert lib.mrbf_ds_criticality(None, None, None, None, None, None, None, None, None) == -1


def test_struct_mirrors_and_declarations():
    from morbit.jl_amd import _lib
    from tests.test_julia_binding import JL, _jl_struct_layout

    assert ctypes.sizeof(_lib.DsInfo) == 24 and _lib.DsInfo.omega.offset == 16 and _lib.DsInfo.ms_total.offset == 12
    assert (_lib.DS_OK, _lib.DS_CRITICAL, _lib.DS_INFEASIBLE, _lib.DS_GAVE_UP) == (0, 1, 2, 3)
    src = open(JL, encoding="utf-8").read()
    layout, total = _jl_struct_layout(src, "MrbfDsInfo")
    assert total == 24 and list(layout) == [f for f, _ in _lib.DsInfo._fields_]
    for f, _ in _lib.DsInfo._fields_:
        assert layout[f] == getattr(_lib.DsInfo, f).offset, f
    for call in ("mrbf_ds_direction", "mrbf_ds_criticality", "mrbf_dispatch_ds"):
        assert re.search(r"ccall\(\(:%s, libmrbf\)" % call, src), call
    assert "struct HipDirectedSearchConfig" in src
    hdr = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert "MRBF_DS_OK = 0, MRBF_DS_CRITICAL = 1, MRBF_DS_INFEASIBLE = 2, MRBF_DS_GAVE_UP = 3" in hdr and "MRBF_ENTRY_DS = 22" in hdr
    # each entry cites the reference's lines
    for name in ("mrbf_ds_direction", "mrbf_ds_criticality"):
        before = hdr[:hdr.index("int32_t %s(" % name)]
        assert "descent.jl:583-664" in before[before.rindex("\n/* "):], name      # the block comment in front of the entry (and its struct)
    # the constants of the method are the same on both sides
    from morbit.jl_amd import descent

    host = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ds_host.hpp")).read()
    for name in ("RANK_TOL", "VANISH_TOL", "DUAL_TOL", "FEAS_TOL"):
        m = re.search(r"constexpr double %s = ([0-9.e+-]+);" % name, host)
        assert m and float(m.group(1)) == getattr(descent, "DS_" + name), name


def test_ds_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "ds_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "ds_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "ds_host_check: ok" in res.stdout


def test_host_header_includes_no_hip():
    text = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ds_host.hpp")).read()
    assert not re.search(r"#include\s*[<\"](hip|rocblas|common\.hpp)", text)


def test_golden_host_results_cover_the_gpu_shapes():
    g = ds_util.load_golden()
    for d, k in ds_util.GPU_SHAPES:
        key = "d%d_k%d" % (d, k)
        assert g[key + "_z"].shape == (ds_util.N_QP, k) and g[key + "_omega"].shape == (ds_util.N_QP,)
        assert np.all(g[key + "_iters"] <= 8 * (d + k) + 16)
    # the stored results are those of the host method on the seeded batch: spot-checked on one small shape, within the device test's
    # bound (another machine's BLAS may add in another order)
    from morbit.jl_amd import descent

    G, r, X, lb, ub = ds_util.make_batch(7, 3)
    for p in (0, 5, 36):
        lo, hi = descent._sd_box(X[p], lb, ub)
        _, z, om, _, _ = descent._ds_active_set(G[p], r[p], lo, hi)
        assert np.all(np.abs(z - g["d7_k3_z"][p]) <= ds_util.z_bound(G[p], r[p])), p
    assert 8 * float(g["worst_ratio"]) <= ds_util.MARGIN
