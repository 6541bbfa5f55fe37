"""CPU tests of the steepest-descent criticality (no GPU): the decision-table rows of mrbf_dispatch_sd and mrbf_dispatch_after,
the host direction LP against the HiGHS fixture and hand cases, the initial step size of compute_descent_step (descent.jl:251-303)
on its three branches, and the Julia binding's routing text."""
import json
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    return pkg._lib.load()


def test_dispatch_sd_rows(lib):
    from morbit.jl_amd import _lib

    D, R = _lib.DISPATCH_DEVICE, _lib.DISPATCH_REFERENCE
    assert lib.mrbf_dispatch_sd(2, 2, 1, 0, 0, 0) == D
    assert lib.mrbf_dispatch_sd(4096, 8, 3, 20, 36, 0) == D            # 64 rows
    assert lib.mrbf_dispatch_sd(4096, 8, 3, 20, 37, 0) == R            # 65 rows
    assert lib.mrbf_dispatch_sd(4097, 2, 1, 0, 0, 0) == R
    assert lib.mrbf_dispatch_sd(0, 2, 1, 0, 0, 0) == R
    assert lib.mrbf_dispatch_sd(12, 0, 1, 0, 0, 0) == R
    assert lib.mrbf_dispatch_sd(12, 2, 0, 0, 0, 0) == R
    assert lib.mrbf_dispatch_sd(12, 2, 1, 0, 0, 1) == R                # a foreign surrogate
    assert lib.mrbf_dispatch_sd(12, 64, 9, 0, 0, 0) == D               # no cap on the model count
    assert lib.mrbf_dispatch_sd(12, 2, 1, -1, 0, 0) == R
    assert _lib.ENTRY_SD == 6
    assert lib.mrbf_dispatch_after(_lib.ENTRY_SD, -2) == 1
    for rc in (0, -1, -3, 1, 2, 3, 5):
        assert lib.mrbf_dispatch_after(_lib.ENTRY_SD, rc) == 0
    # the existing entries are unchanged
    assert lib.mrbf_dispatch_after(_lib.ENTRY_PS_STEP, -2) == 1 and lib.mrbf_dispatch_after(_lib.ENTRY_PS_STEP, 5) == 0
    assert lib.mrbf_dispatch_after(_lib.ENTRY_ROUND4, 5) == 1 and lib.mrbf_dispatch_after(_lib.ENTRY_AFFINE, -2) == 0


def test_sd_direction_rejects_invalid_arguments(lib):
    assert lib.mrbf_sd_direction(None, 1, 2, 1, 0, 0, *([None] * 8), 1, None, None, None, None, None) == -1


def load_sd_fixture():
    """tests/golden/sd_lp.{json,npz} as dicts with fp64 arrays (the loader of tests/golden/make_sd_lp.py)"""
    import importlib.util

    g = os.path.join(ROOT, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_sd_lp", os.path.join(g, "make_sd_lp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load(os.path.join(g, "sd_lp.npz"), os.path.join(g, "sd_lp.json"))


def _fixture():
    return load_sd_fixture()


def test_fixture_covers_the_issue_families():
    cases = _fixture()
    assert 200 <= len(cases)
    tags = {c["tag"] for c in cases}
    assert {"random", "x_on_bound", "l_eq_u", "duplicate_rows", "zero_row", "all_zero", "critical", "linear", "infeasible_eq",
            "infeasible_ineq", "empty_box", "m64", "large"} <= tags
    assert {c["d"] for c in cases} >= {1, 2, 5, 12, 64, 256, 1024, 4096}
    assert {c["k"] for c in cases} >= {1, 2, 3, 5, 8}
    assert max(c["k"] + c["m_eq"] + c["m_ineq"] for c in cases) == 64
    assert any(c["m_ineq"] and np.any(c["b_ineq"] < 0) for c in cases)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sd_lp.npz")) < 300e3


def test_host_direction_against_the_fixture():
    from morbit.jl_amd import descent

    for c in _fixture():
        d, om, st = descent._steepest_descent_direction(c["x"], c["G"], c["lb"], c["ub"], c["A_eq"], c["b_eq"], c["A_ineq"],
                                                         c["b_ineq"], c["normalize"], want_status=True)
        assert st == c["status"], c["idx"]
        if c["omega"] is None:
            assert om == -np.inf and not d.any()
            continue
        lo, hi = descent._sd_box(c["x"], c["lb"], c["ub"])
        assert np.all(d >= lo) and np.all(d <= hi)
        assert abs(om - c["omega"]) <= 1e-9 * max(1.0, abs(c["omega"])), c["idx"]


def test_host_direction_hand_cases():
    from morbit.jl_amd import descent

    # one objective, box [-1, 1]^2: d = -sign(g), omega = ||g||_1 / ||g||_2
    d, om = descent._steepest_descent_direction(np.zeros(2), [[3.0, -4.0]], -np.ones(2) * 5, np.ones(2) * 5)
    assert np.array_equal(d, [-1.0, 1.0]) and abs(om - 7.0 / 5.0) < 1e-12
    # opposite gradients: critical
    d, om = descent._steepest_descent_direction(np.zeros(2), [[1.0, 1.0], [-1.0, -1.0]], -np.ones(2), np.ones(2))
    assert abs(om) < 1e-12
    # x on its upper bound: the direction cannot go up
    d, om = descent._steepest_descent_direction(np.array([1.0, 0.0]), [[-1.0, 0.0]], -np.ones(2), np.array([1.0, 1.0]))
    assert d[0] == 0.0 and abs(om) < 1e-12
    # the reference's catch branch: zero gradients under normalize, an empty box
    d, om = descent._steepest_descent_direction(np.zeros(2), np.zeros((2, 2)), -np.ones(2), np.ones(2), normalize=True)
    assert om == -np.inf and not d.any()
    d, om = descent._steepest_descent_direction(np.zeros(2), np.zeros((1, 2)), -np.ones(2), np.ones(2), normalize=False)
    assert om == 0.0
    d, om = descent._steepest_descent_direction(np.zeros(2), [[1.0, 0.0]], np.array([1.5, -1.0]), np.array([2.0, 1.0]))
    assert om == -np.inf and not d.any()


def test_initial_step_size_branches():
    from morbit.jl_amd import descent

    lb, ub = np.full(2, -10.0), np.full(2, 10.0)
    x = np.zeros(2)
    # Delta <= 1 at x == x_n: sigma = min(Delta / ||d||_inf, 1)
    assert descent._sd_stepsize(x, x, 0.5, lb, ub, np.array([-1.0, 0.25])) == (0.5, "delta")
    assert descent._sd_stepsize(x, x, 0.5, lb, ub, np.array([-0.25, 0.1])) == (1.0, "delta")
    # x ~ x_n with Julia's isapprox (rtol sqrt(eps)) counts as no normal step
    xs = np.array([1.0, 1.0])
    assert descent._sd_stepsize(xs, xs * (1 + 1e-10), 0.5, lb, ub, np.array([-1.0, 0.0]))[0] == 0.5
    # after a normal step Delta is the step to the trust region's boundary along d from x_n
    s, br = descent._sd_stepsize(x, np.array([0.2, 0.0]), 0.5, lb, ub, np.array([1.0, 0.0]))
    assert br == "delta" and abs(s - 0.3) < 1e-15
    # Delta > 1 and ||d|| != 1: sigma = 1
    assert descent._sd_stepsize(x, x, 3.0, lb, ub, np.array([0.5, -0.2])) == (1.0, "one")
    # Delta > 1 and ||d|| ~ 1: the largest sigma with x_n + sigma d inside the local box and A (x_n + sigma d) <= b
    s, br = descent._sd_stepsize(x, x, 3.0, lb, ub, np.array([1.0, 0.5]))
    assert br == "intersect" and s == 3.0
    s, br = descent._sd_stepsize(x, x, 3.0, lb, ub, np.array([1.0, 0.5]), lin=(None, None, np.array([[1.0, 0.0]]), np.array([2.0])))
    assert br == "intersect" and s == 2.0
    # with a modelled inequality constraint m(x) + Dm(x) (n + sigma d) <= 0
    s, br = descent._sd_stepsize(x, x, 3.0, lb, ub, np.array([1.0, 0.0]),
                                 constraints_at_x=lambda: (np.zeros((0, 2)), np.zeros(0), np.array([[0.5, 0.0]]), np.array([-0.25])))
    assert br == "intersect" and abs(s - 0.5) < 1e-15
    # Delta / ||d|| with d = 0: sigma = min(Inf, 1)
    assert descent._sd_stepsize(x, x, 0.5, lb, ub, np.zeros(2)) == (1.0, "delta")


def test_intersect_bounds_equality_rows():
    from morbit.jl_amd import descent

    x, d = np.zeros(2), np.array([1.0, 1.0])
    assert descent._intersect_bounds(x, d, -np.ones(2) * 5, np.ones(2) * 5, np.array([[1.0, 0.0]]), np.array([2.0])) == 2.0
    assert descent._intersect_bounds(x, d, -np.ones(2), np.ones(2), np.array([[1.0, 0.0]]), np.array([2.0])) == 0.0   # leaves the box
    assert descent._intersect_bounds(x, d, -np.ones(2) * 5, np.ones(2) * 5, np.array([[1.0, 0.0], [0.0, 1.0]]), np.array([2.0, 3.0])) == 0.0


def test_julia_binding_routes_steepest_descent():
    src = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    m = re.search(r"^function get_criticality\(desc_cfg::SteepestDescentConfig.*?^end", src, flags=re.S | re.M)
    assert m, "no get_criticality method for SteepestDescentConfig"
    body = m.group(0)
    assert re.search(r"reference\(\) = invoke\(get_criticality, Tuple\{SteepestDescentConfig,", body)
    assert "_dispatch_sd(" in body and re.search(r"_locked\(ctx\) do \w+\s+ccall\(\(:mrbf_sd_criticality, libmrbf\)", body)
    i_call, i_fb = body.index(":mrbf_sd_criticality"), body.index("_fallback_rc(6, rc)")
    assert i_fb > i_call
    assert re.search(r"ccall\(\(:mrbf_dispatch_sd, libmrbf\)", src)
    section = src[src.index("# ---- descent consumers"):src.index("# ---- site selection on the device")]
    assert "error(" not in section


def test_sd_info_layout_and_julia_mirror():
    import ctypes

    from morbit.jl_amd import _lib
    from tests.test_julia_binding import JL, _jl_struct_layout

    assert ctypes.sizeof(_lib.SdInfo) == 24 and _lib.SdInfo.omega.offset == 16
    layout, total = _jl_struct_layout(open(JL, encoding="utf-8").read(), "MrbfSdInfo")
    assert total == 24 and list(layout) == [f for f, _ in _lib.SdInfo._fields_]
    assert all(layout[f] == getattr(_lib.SdInfo, f).offset for f in layout)
