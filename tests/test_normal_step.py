"""CPU tests of the normal step (no GPU): the decision-table rows of mrbf_dispatch_normal and mrbf_dispatch_after, argument checks of
mrbf_normal_direction, the host LP (_normal_step_lp) and the dual bound of its certificate against the HiGHS fixture and the
closed form, compute_normal_step's radius / infeasibility / projection semantics and its routing, the NormalInfo layout and the
Julia binding's text."""
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    return pkg._lib.load()


def load_normal_fixture():
    """tests/golden/normal_lp.{json,npz} as dicts with fp64 arrays (the loader of tests/golden/make_normal_lp.py)"""
    import importlib.util

    g = os.path.join(ROOT, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_normal_lp", os.path.join(g, "make_normal_lp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load(os.path.join(g, "normal_lp.npz"), os.path.join(g, "normal_lp.json"))


def _scale(c):
    C = np.vstack([c["A_eq"], c["A_ineq"]])
    b = np.concatenate([c["b_eq"], c["b_ineq"]])
    a = c["alpha"] or 0.0
    return float(np.max(np.maximum(1.0, np.abs(b) + max(1.0, a) * np.abs(C).sum(axis=1)), initial=1.0))


def test_dispatch_normal_rows(lib):
    from morbit.jl_amd import _lib

    D, R = _lib.DISPATCH_DEVICE, _lib.DISPATCH_REFERENCE
    assert lib.mrbf_dispatch_normal(2, 1, 1, 0, 0) == D
    assert lib.mrbf_dispatch_normal(1, 0, 0, 1, 0) == D                  # linear rows only, no model
    assert lib.mrbf_dispatch_normal(4096, 3, 20, 44, 0) == D             # 64 rows
    assert lib.mrbf_dispatch_normal(4096, 3, 20, 45, 0) == R             # 65 rows
    assert lib.mrbf_dispatch_normal(4097, 1, 1, 0, 0) == R
    assert lib.mrbf_dispatch_normal(0, 1, 1, 0, 0) == R
    assert lib.mrbf_dispatch_normal(12, 1, 0, 0, 0) == R                 # no row
    assert lib.mrbf_dispatch_normal(12, 1, 0, 1, 0) == D                 # one row
    assert lib.mrbf_dispatch_normal(12, 1, 1, 0, 1) == R                 # a modelled row on a foreign surrogate
    assert lib.mrbf_dispatch_normal(12, 1, -1, 0, 0) == R
    assert _lib.ENTRY_NORMAL == 7
    assert lib.mrbf_dispatch_after(_lib.ENTRY_NORMAL, -2) == 1
    for rc in (0, -1, -3, 1, 2, 5):
        assert lib.mrbf_dispatch_after(_lib.ENTRY_NORMAL, rc) == 0
    assert lib.mrbf_dispatch_after(_lib.ENTRY_SD, -2) == 1 and lib.mrbf_dispatch_after(_lib.ENTRY_AFFINE, -2) == 0


def test_normal_direction_rejects_invalid_arguments(lib):
    assert lib.mrbf_normal_direction(None, 1, 2, 0, 1, *([None] * 12)) == -1
    assert lib.mrbf_normal_step(None, None, 2, None, None, None, 0.5, 1.0, 1.0, 0, None, None, None) == -1


def test_fixture_covers_the_issue_families():
    cases = load_normal_fixture()
    tags = {c["tag"] for c in cases}
    assert {"alpha0", "closed", "eq_only", "mixed", "on_bound", "outside", "inf_box", "infeasible_rows", "infeasible_eq",
            "infeasible_box", "empty_box", "duplicate_rows", "zero_row", "zero_row_infeasible", "ties"} <= tags
    assert {c["d"] for c in cases} >= {1, 2, 3, 12, 64, 128, 256, 1024, 4096}
    assert max(c["m_eq"] + c["m_ineq"] for c in cases) == 64
    assert any(np.isinf(c["lb"]).any() for c in cases) and any(np.isinf(c["ub"]).any() for c in cases)
    assert any(((c["x"] < c["lb"]) | (c["x"] > c["ub"])).any() for c in cases)
    feas = [c for c in cases if c["status"] == 0]
    assert any(c["alpha"] / c["kappa_delta"] <= c["delta_max"] for c in feas)
    assert any(c["alpha"] / c["kappa_delta"] > c["delta_max"] for c in feas)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "normal_lp.npz")) < 410e3


def test_host_lp_against_the_fixture():
    from morbit.jl_amd import descent

    for c in load_normal_fixture():
        n, alpha, st, y = descent._normal_step_lp(c["x"], c["lb"], c["ub"], c["A_eq"], c["b_eq"], c["A_ineq"], c["b_ineq"])
        assert st == c["status"], c["idx"]
        if st:
            assert np.all(np.isnan(n)) and alpha == np.inf
            continue
        assert abs(alpha - c["alpha"]) <= 1e-9 * _scale(c), c["idx"]
        assert np.all(c["x"] + n >= c["lb"]) and np.all(c["x"] + n <= c["ub"])
        if c["closed"] is not None:
            assert abs(alpha - c["closed"]) <= 1e-12 * _scale(c), (c["idx"], alpha, c["closed"])   # relative to the row scale


def test_dual_bound_certificate_and_weak_duality():
    from morbit.jl_amd import descent

    rng = np.random.default_rng(1)
    for c in load_normal_fixture():
        if c["status"]:
            continue
        args = (c["x"], c["lb"], c["ub"], c["A_eq"], c["b_eq"], c["A_ineq"], c["b_ineq"])
        phi = descent.normal_lp_dual_bound(c["y"], *args)
        assert abs(c["alpha"] - phi) <= 1e-9 * _scale(c), (c["idx"], c["alpha"], phi)
        for _ in range(3):
            y = rng.standard_normal(c["m_eq"] + c["m_ineq"]) * rng.random() * 2
            y[c["m_eq"]:] = np.abs(y[c["m_eq"]:])
            assert descent.normal_lp_dual_bound(y, *args) <= c["alpha"] + 1e-9 * _scale(c), c["idx"]


def test_dual_bound_hand_cases():
    from morbit.jl_amd import descent

    # one row c . n <= b with b < 0, no box: phi(y) = -y b for y ||c||_1 <= 1, -inf beyond
    c, b = np.array([[1.0, -2.0]]), np.array([-3.0])
    inf = np.full(2, np.inf)
    assert descent.normal_lp_dual_bound([1.0 / 3.0], np.zeros(2), -inf, inf, A_ineq=c, b_ineq=b) == 1.0
    assert descent.normal_lp_dual_bound([0.1], np.zeros(2), -inf, inf, A_ineq=c, b_ineq=b) == pytest.approx(0.3)
    assert descent.normal_lp_dual_bound([0.5], np.zeros(2), -inf, inf, A_ineq=c, b_ineq=b) == -np.inf
    # x outside the box: alpha0 = 2 is a floor even for y = 0
    assert descent.normal_lp_dual_bound([0.0], np.array([3.0, 0.0]), np.array([-1.0, -1.0]), np.array([1.0, 1.0]), A_ineq=c,
                                        b_ineq=np.array([10.0])) == 2.0


def _linear_container(d):
    """a container whose only surrogate is an objective (the normal step ignores objectives): linear rows only"""
    from morbit.jl_amd import surrogates as sg
    from oracle import rbf_oracle as orc
    from tests.test_dispatch import DeviceModelDouble

    rng = np.random.default_rng(d)
    C = rng.random((3 * d + 3, d))
    m = DeviceModelDouble(orc.fit(C, np.stack([C.sum(axis=1), -C.sum(axis=1)], axis=1), 0, 3.0, 0.0, 1))
    return sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])])


def test_compute_normal_step_reference_semantics(monkeypatch):
    from morbit.jl_amd import _lib, descent

    lib = _lib.load()
    monkeypatch.setattr(lib, "mrbf_dispatch_normal", lambda *a: _lib.DISPATCH_REFERENCE)
    sc = _linear_container(2)
    lb, ub = np.full(2, -1.0), np.full(2, 1.0)
    lin = (None, None, np.array([[1.0, 1.0]]), np.array([-1.0]))                 # n_1 + n_2 <= -1 at x = 0: alpha* = 0.5
    st = {}
    n, dl = descent.compute_normal_step(sc, None, np.zeros(2), 0.3, lb, ub, lin, stats=st)
    assert st["path"] == "reference" and dl == 0.3 and np.allclose(n, [-0.5, -0.5], atol=1e-9)
    n, dl = descent.compute_normal_step(sc, None, np.zeros(2), 0.3, lb, ub, lin, kappa_delta=0.25, delta_max=5.0, variable_radius=True)
    assert abs(dl - 2.0) <= 1e-9
    n, dl = descent.compute_normal_step(sc, None, np.zeros(2), 0.3, lb, ub, lin, kappa_delta=0.25, delta_max=1.5, variable_radius=True)
    assert dl == -np.inf and np.all(np.isnan(n))
    bad = (None, None, np.array([[1.0, 1.0], [-1.0, -1.0]]), np.array([-1.0, -1.0]))
    n, dl = descent.compute_normal_step(sc, None, np.zeros(2), 0.3, lb, ub, bad)
    assert dl == -np.inf and np.all(np.isnan(n))
    # the projection into the box: x outside [lb, ub] with rows that hold anywhere -> n moves x onto the box
    x = np.array([1.5, -3.0])
    n, dl = descent.compute_normal_step(sc, None, x, 0.3, lb, ub, (None, None, np.array([[0.0, 1.0]]), np.array([100.0])))
    assert np.all(x + n >= lb) and np.all(x + n <= ub) and abs(np.max(np.abs(n)) - 2.0) <= 1e-9


def test_compute_normal_step_routes_to_the_device(monkeypatch):
    from morbit.jl_amd import _lib, descent

    lib = _lib.load()
    calls = []
    monkeypatch.setattr(lib, "mrbf_dispatch_normal", lambda *a: calls.append(a) or _lib.DISPATCH_DEVICE)
    monkeypatch.setattr(descent, "normal_step_device",
                        lambda plan, x, lb, ub, delta, lin, kd, dm, vr: (0, np.full(np.asarray(x).size, 0.125), 0.7, {"status": 0}))
    sc = _linear_container(3)
    st = {}
    lin = (None, None, np.ones((1, 3)), np.array([-1.0]))
    n, dl = descent.compute_normal_step(sc, None, np.zeros(3), 0.7, np.full(3, -1.0), np.full(3, 1.0), lin, stats=st)
    assert st["path"] == "device" and dl == 0.7 and np.all(n == 0.125)
    assert calls == [(3, 1, 0, 1, 0)]
    # a fall-back code from the device path takes the reference method
    monkeypatch.setattr(descent, "normal_step_device", lambda *a: (-2, None, None, {"status": _lib.NS_GAVE_UP}))
    n, dl = descent.compute_normal_step(sc, None, np.zeros(3), 0.7, np.full(3, -1.0), np.full(3, 1.0), lin, stats=st)
    assert st["path"] == "reference" and dl == 0.7 and abs(np.max(np.abs(n)) - 1.0 / 3.0) <= 1e-9


def test_normal_info_layout_and_julia_mirror():
    import ctypes

    from morbit.jl_amd import _lib
    from tests.test_julia_binding import JL, _jl_struct_layout

    assert ctypes.sizeof(_lib.NormalInfo) == 32 and _lib.NormalInfo.alpha.offset == 16 and _lib.NormalInfo.delta.offset == 24
    hdr = open(os.path.join(ROOT, "include", "mrbf.h"), encoding="utf-8").read()
    m = re.search(r"typedef struct \{([^{}]*?)\} mrbf_normal_info;", hdr, flags=re.S)
    assert m and [f for f in re.findall(r"\b(\w+);", m.group(1))] == [f for f, _ in _lib.NormalInfo._fields_]
    layout, total = _jl_struct_layout(open(JL, encoding="utf-8").read(), "MrbfNormalInfo")
    assert total == 32 and list(layout) == [f for f, _ in _lib.NormalInfo._fields_]
    assert all(layout[f] == getattr(_lib.NormalInfo, f).offset for f in layout)


def test_julia_binding_routes_the_normal_step():
    src = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    m = re.search(r"^function hip_compute_normal_step\(.*?^end", src, flags=re.S | re.M)
    assert m, "no hip_compute_normal_step"
    body = m.group(0)
    assert re.search(r"reference\(\) = compute_normal_step\(", body) and "_touches_device(sc) || return reference()" in body
    assert "_dispatch_normal(" in body and re.search(r"_locked\(ctx\) do \w+\s+ccall\(\(:mrbf_normal_step, libmrbf\)", body)
    assert body.index("_fallback_rc(7, rc)") > body.index(":mrbf_normal_step")
    # linear rows only pass the table with no device model in the plan: the context must not come from plan.models[1] alone
    assert re.search(r"ctx = isempty\(plan\.models\) \? mrbf_context\(\) : plan\.models\[1\]\.ctx", body)
    assert "plan.models[1]" not in body.replace("isempty(plan.models) ? mrbf_context() : plan.models[1].ctx", "")
    assert re.search(r"ccall\(\(:mrbf_dispatch_normal, libmrbf\)", src)
