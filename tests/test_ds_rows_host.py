"""CPU tests of directed search with constraint rows (descent.jl:196-236, :598-645): the host mirror of the extended direction QP
(morbit.jl_amd/descent.py: _ds_active_set_rows, the NumPy form of the method ds_qp_rows.hip runs) on seeded QPs with the certificate
of every solution and against SciPy's SLSQP, its statuses and start rule, the identity with _ds_active_set where there are no rows,
the decision table's rows, the mirrors of the header, and the host logic of the device call (tools/ds_rows_host_check.cpp, a
stand-alone program under AddressSanitizer and UBSan, run as a child process).  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import ds_rows_util as ru
from tests import ds_util
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


@pytest.mark.parametrize("d,k,m_eq,m_in", ru.CPU_SHAPES)
def test_host_mirror_certificate_and_slsqp(d, k, m_eq, m_in):
    """Every status OK, the box exactly, rows within FEAS_TOL (sum |W| + |h|), the KKT certificate within ds_util.KKT_TOL, and
    f <= f_SLSQP + SLSQP_TAU (1 + f).  Measured (tests/golden/make_ds_rows_host.py): certificate residual at most 8.7e-13, excess over
    SLSQP at most 5.21e-10 (SLSQP accepts rows within 1e-9), SLSQP failing on at most 1 of a shape's 10 QPs, iterations at most
    3.37 (d + K)."""
    from morbit.jl_amd import _lib, descent

    K = k + m_eq + m_in
    G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(d, k, m_eq, m_in, n_qp=10)
    worst, most, kkt, skipped = -np.inf, 0.0, 0.0, 0
    for p in range(10):
        lo, hi = descent._sd_box(X[p], lb, ub)
        st = {}
        dd, c, om, mu, status = descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p], st)
        assert status == _lib.DS_OK, (d, k, m_eq, m_in, p, status, st)
        kkt = max(kkt, ru.check_solution(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p], dd, c, om, mu, (d, k, m_eq, m_in, p)))
        assert st["iterations"] <= 8 * (d + K) + 16
        most = max(most, st["iterations"] / (d + K))
        ds = descent._ds_slsqp(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p])
        if ds is None:
            skipped += 1
            continue
        f, fs = ru.value(G[p], r[p], dd), ru.value(G[p], r[p], ds)
        worst = max(worst, (f - fs) / (1 + f))
        print("QP %d: (f - f_SLSQP) / (1 + f) = %.3g" % (p, (f - fs) / (1 + f)))
        assert f <= fs + ru.SLSQP_TAU * (1 + f), (d, k, m_eq, m_in, p, f, fs)
    assert 4 * skipped <= 10, skipped      # at most a quarter of a shape's QPs without SLSQP's answer
    print("%s: certificate <= %.1e, f - f_SLSQP <= %.1e (1 + f), SLSQP failed on %d, iterations <= %.2f (d + K)"
          % (ru.key(d, k, m_eq, m_in), kkt, worst, skipped, most))


@pytest.mark.parametrize("d,k", [(1, 1), (2, 3), (7, 5), (7, 16), (30, 2), (65, 3)])
def test_without_rows_it_is_the_active_set_method_bit_for_bit(d, k):
    from morbit.jl_amd import descent

    G, r, X, lb, ub = ds_util.make_batch(d, k, n_qp=12)
    for p in range(12):
        lo, hi = descent._sd_box(X[p], lb, ub)
        s1, s2 = {}, {}
        a = descent._ds_active_set(G[p], r[p], lo, hi, s1)
        b = descent._ds_active_set_rows(G[p], r[p], lo, hi, None, None, None, None, s2)
        assert a[4] == b[4] and s1 == s2, (p, s1, s2)
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True) and np.all(np.signbit(u) == np.signbit(v)), p


def _small(seed=3, d=6, k=2):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((k, d))
    r = -rng.uniform(0.2, 1.0, k)
    lo, hi = np.full(d, -0.5), np.full(d, 0.5)
    A_eq, A_in = rng.standard_normal((1, d)), rng.standard_normal((2, d))
    return G, r, lo, hi, A_eq, np.zeros(1), A_in, np.array([0.0, 0.2])


def test_start_rule_no_start_and_clamp():
    from morbit.jl_amd import _lib, descent

    G, r, lo, hi, A_eq, b_eq, A_in, b_in = _small()
    assert descent.DS_START_TOL == 1e-10 and _lib.DS_NO_START == 4
    se, si = np.abs(A_eq).sum(axis=1), np.abs(A_in).sum(axis=1)
    for be, bi in ((2e-10 * se, b_in), (-2e-10 * se, b_in), (b_eq, np.array([-2e-10 * si[0], 0.2])), (np.array([np.nan]), b_in)):
        dd, c, om, mu, status = descent._ds_active_set_rows(G, r, lo, hi, A_eq, be, A_in, bi)
        assert status == _lib.DS_NO_START and np.all(np.isnan(dd)) and np.all(np.isnan(c)) and np.isnan(om) and np.all(np.isnan(mu))
    # a residual below START_TOL times the row's scale is clamped: the QP is solved for h = 0 on those rows, to the bit
    ref = descent._ds_active_set_rows(G, r, lo, hi, A_eq, b_eq, A_in, b_in)
    assert ref[4] == _lib.DS_OK
    for be, bi in ((0.5e-10 * se, b_in), (-0.5e-10 * se, np.array([-0.5e-10 * si[0], 0.2]))):
        out = descent._ds_active_set_rows(G, r, lo, hi, A_eq, be, A_in, bi)
        assert out[4] == _lib.DS_OK and all(np.array_equal(u, v) for u, v in zip(out[:4], ref[:4]))
        ru.check_solution(G, r, lo, hi, A_eq, be, A_in, bi, *out[:4], "clamped", h=np.array([0.0, 0.0, 0.0, 0.0, 0.2]))


def test_critical_and_infeasible_as_the_active_set_method():
    from morbit.jl_amd import _lib, descent

    G, r, lo, hi, A_eq, b_eq, A_in, b_in = _small()
    for bad in (0.0, 0.3, np.nan):
        rr = np.array([r[0], bad])
        a = descent._ds_active_set(G, rr, lo, hi)
        b = descent._ds_active_set_rows(G, rr, lo, hi, A_eq, b_eq, A_in, b_in)
        assert a[4] == b[4] == _lib.DS_CRITICAL and not b[0].any() and not b[1].any() and b[1].shape == (5,) and b[2] == a[2] == 0.0
        assert not b[3].any()
    lo2 = lo.copy()
    lo2[2] = 0.75
    a = descent._ds_active_set(G, r, lo2, hi)
    b = descent._ds_active_set_rows(G, r, lo2, hi, A_eq, b_eq, A_in, b_in)
    assert a[4] == b[4] == _lib.DS_INFEASIBLE and not b[0].any() and b[2] == a[2] == -np.inf
    # CRITICAL is decided before the box and the rows are looked at; a start outside the box is GAVE_UP as before
    assert descent._ds_active_set_rows(G, np.array([1.0, -1.0]), lo2, hi, A_eq, np.ones(1), A_in, b_in)[4] == _lib.DS_CRITICAL
    lo3 = lo.copy()
    lo3[1] = 0.25
    st = {}
    assert descent._ds_active_set_rows(G, r, lo3, hi, A_eq, b_eq, A_in, b_in, st)[4] == _lib.DS_GAVE_UP and st["gave_up"] == "start"


def test_a_far_inequality_changes_nothing():
    """an inequality row with b = 1e6 never blocks: z moves by no more than the device test's bound (MARGIN (d + K) 2^-52 scale)"""
    from morbit.jl_amd import _lib, descent

    margin = 8.0 * float(ru.load_golden()["worst_ratio"])
    for d, k, m_eq, m_in in ((7, 2, 1, 1), (30, 3, 0, 2), (65, 2, 2, 3)):
        G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(d, k, m_eq, m_in, n_qp=8)
        for p in range(8):
            lo, hi = descent._sd_box(X[p], lb, ub)
            far = np.random.default_rng(p).standard_normal((1, d))
            a = descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p])
            b = descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], np.vstack([Ai[p], far]), np.append(bi[p], 1e6))
            assert a[4] == b[4] == _lib.DS_OK
            assert np.all(np.abs(a[1][:k] - b[1][:k]) <= ru.z_bound(G[p], r[p], k + m_eq + m_in + 1, margin)), (d, p)
            assert b[3][-1] == 0.0


def test_rank_cap_ends_the_stall_of_a_full_vertex():
    """(d; k, m_eq, m_in) = (7; 5, 3, 8), QP 4 of seed 0 (row 1 = 2 row 0): seven rows of S pin all seven variables, and rounding left an
    eighth pivot on a residual diagonal above RANK_TOL -- the step then moved the equalities and one row blocked until the cap.  With
    at most |N| pivots it ends with status OK."""
    from morbit.jl_amd import _lib, descent

    G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(7, 5, 3, 8)
    for p in range(ru.N_QP):
        lo, hi = descent._sd_box(X[p], lb, ub)
        st = {}
        out = descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p], st)
        assert out[4] == _lib.DS_OK and st["iterations"] <= 3 * (7 + 16), (p, st)


def test_decision_table_rows(lib):
    from morbit.jl_amd import _lib

    D, R = _lib.DISPATCH_DEVICE, _lib.DISPATCH_REFERENCE
    f = lib.mrbf_dispatch_ds_rows   # (d, k, n_models, n_nl, n_lin, n_foreign)
    assert f(7, 2, 1, 1, 0, 0) == D and f(7, 2, 1, 0, 1, 0) == D and f(1, 1, 1, 0, 1, 0) == D and f(4096, 1, 8, 7, 8, 0) == D
    assert f(7, 2, 1, 0, 0, 0) == R            # no constraint row: mrbf_dispatch_ds is the table to ask
    assert f(7, 2, 1, 1, 0, 1) == R            # a foreign surrogate
    assert f(7, 2, 0, 1, 0, 0) == R            # no device model
    assert f(0, 2, 1, 1, 0, 0) == R and f(4097, 2, 1, 1, 0, 0) == R
    assert f(7, 0, 1, 1, 0, 0) == R
    assert f(7, 2, 1, 10, 4, 0) == D and f(7, 2, 1, 10, 5, 0) == R and f(7, 16, 1, 1, 0, 0) == R     # k + n_nl + n_lin <= 16
    assert f(7, 2, 1, -1, 2, 0) == R and f(7, 2, 1, 2, -1, 0) == R
    assert _lib.ENTRY_DS_ROWS == 24
    assert lib.mrbf_dispatch_after(_lib.ENTRY_DS_ROWS, -2) == 1
    for rc in (0, -1, -3, -4, -8, -21, _lib.MRBF_EHIP, _lib.MRBF_ENOMEM):
        assert lib.mrbf_dispatch_after(_lib.ENTRY_DS_ROWS, rc) == 0
    # the rows of mrbf_dispatch_ds stay: constraint rows still take the host method there
    g = lib.mrbf_dispatch_ds
    assert g(7, 2, 1, 0, 0, 0) == D and g(7, 2, 1, 1, 0, 0) == R and g(7, 2, 1, 0, 1, 0) == R


def test_refusals_that_need_no_device(lib):
    assert lib.mrbf_ds_direction_rows(None, 1, 2, 2, 0, 0, *([None] * 15)) == -1
    assert lib.mrbf_ds_criticality_rows(None, None, None, None, None, None, None, None, None, None) == -1


def test_mirrors_and_declarations():
    from morbit.jl_amd import _lib, descent
    from tests.test_julia_binding import JL

    src = open(JL, encoding="utf-8").read()
    for call in ("mrbf_ds_criticality_rows", "mrbf_dispatch_ds_rows"):
        assert re.search(r"ccall\(\(:%s, libmrbf\)" % call, src), call
    assert "constraint_rows::Symbol" in src and "constraint_rows = :host" in src
    assert descent.DirectedSearchConfig().constraint_rows == "host"
    with pytest.raises(AssertionError):
        descent.DirectedSearchConfig(constraint_rows="gpu")
    hdr = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"^enum \{ MRBF_DS_NO_START = 4 \};", hdr, re.M) and "MRBF_ENTRY_DS_ROWS = 24" in hdr
    for name in ("mrbf_ds_direction_rows", "mrbf_ds_criticality_rows"):
        before = hdr[:hdr.index("int32_t %s(" % name)]
        block = before[before.rindex("\n/* "):]
        assert "descent.jl:196-236" in block and ":598-645" in block, name
    host = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ds_rows_host.hpp")).read()
    m = re.search(r"constexpr double START_TOL = ([0-9.e+-]+);", host)
    assert m and float(m.group(1)) == descent.DS_START_TOL and 1e-13 <= descent.DS_START_TOL <= 1e-9
    assert not re.search(r"#include\s*[<\"](hip|rocblas|common\.hpp)", host)


def test_ds_rows_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "ds_rows_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "ds_rows_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "ds_rows_host_check: ok" in res.stdout


def test_golden_host_results_cover_the_gpu_shapes():
    from morbit.jl_amd import descent

    g = ru.load_golden()
    for d, k, m_eq, m_in in ru.GPU_SHAPES:
        key = ru.key(d, k, m_eq, m_in)
        assert g[key + "_z"].shape == (ru.N_QP, k) and g[key + "_omega"].shape == (ru.N_QP,) and g[key + "_value"].shape == (ru.N_QP,)
        assert np.all(g[key + "_iters"] <= 8 * (d + k + m_eq + m_in) + 16) and not g[key + "_status"].any()
    margin = 8.0 * float(g["worst_ratio"])
    G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(7, 2, 2, 3)
    for p in (0, 5, 36):      # spot-checked within the device test's bound (another machine's BLAS may add in another order)
        lo, hi = descent._sd_box(X[p], lb, ub)
        c = descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p])[1]
        assert np.all(np.abs(c[:2] - g["d7_k2_e2_i3_z"][p]) <= ru.z_bound(G[p], r[p], 7, margin)), p
