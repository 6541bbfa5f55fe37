"""CPU tests of the local-ideal-point entries (mrbf_ideal_point_problem, mrbf_ideal_point_batch): their decision-table rows against
the Pascoletti-Serafini rows they repeat, the record's struct mirror against the header and the Julia struct, the NULL-context answer,
the routing of `pascoletti_serafini.compute_local_ideal_points_many` and of `descent.ds_iterate_many` / `get_criticality_ds` with
`ideal_point="device"` (one call for the ideal points of all starts, constraints not carried, every start handed its r), the default
configuration staying clear of the new symbols, and the host logic of the device calls (tools/ideal_host_check.cpp, a stand-alone
program under AddressSanitizer and UBSan, run as a child process).  No GPU: the device calls are replaced by stubs."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


def test_decision_table_rows_are_the_ps_rows(lib):
    from morbit.jl_amd import _lib

    n = 0
    grid = itertools.product((0, 1, 3, 128, 256, 257, 356, 357), (0, 1, 2, 8, 9), (0, 1, 8, 9), (-1, 0, 32, 33), (-1, 0, 256, 257), (0, 1))
    for d, k, nm, n_nl, n_lin, n_foreign in grid:
        want = lib.mrbf_dispatch_ps(d, k, nm, n_nl, n_lin, n_foreign)
        assert lib.mrbf_dispatch_ideal(d, k, nm, n_nl, n_lin, n_foreign) == want, (d, k, nm, n_nl, n_lin, n_foreign)
        for ns in (-1, 0, 1, 2, 65535, 65536, 1 << 40):
            assert (lib.mrbf_dispatch_ideal_batch(ns, d, k, nm, n_nl, n_lin, n_foreign)
                    == lib.mrbf_dispatch_ps_batch(ns, d, k, nm, n_nl, n_lin, n_foreign)), (ns, d, k, nm, n_nl, n_lin, n_foreign)
            n += 1
    assert n > 10000
    # the corners by name: the single call reaches d = 356, the batch d = 256; eight objectives; 1 .. 65535 starts
    dev, ref = _lib.DISPATCH_DEVICE, _lib.DISPATCH_REFERENCE
    assert [lib.mrbf_dispatch_ideal(d, 2, 1, 0, 0, 0) for d in (256, 257, 356, 357)] == [dev, dev, dev, ref]
    assert [lib.mrbf_dispatch_ideal_batch(5, d, 2, 1, 0, 0, 0) for d in (256, 257, 356, 357)] == [dev, ref, ref, ref]
    assert [lib.mrbf_dispatch_ideal(3, k, 1, 0, 0, 0) for k in (8, 9)] == [dev, ref]
    assert [lib.mrbf_dispatch_ideal_batch(ns, 3, 2, 1, 0, 0, 0) for ns in (0, 1, 65535, 65536)] == [ref, dev, dev, ref]


def test_return_codes_that_mean_reference(lib):
    from morbit.jl_amd import _lib

    assert (_lib.ENTRY_IDEAL, _lib.ENTRY_IDEAL_BATCH) == (25, 26)
    for entry in (25, 26):
        assert lib.mrbf_dispatch_after(entry, -2) == 1
        assert all(lib.mrbf_dispatch_after(entry, rc) == 0 for rc in (0, -1, -3, -4, -5, -6, -10, -100, -101, 1))
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_IDEAL = 25\b", text) and re.search(r"MRBF_ENTRY_IDEAL_BATCH = 26\b", text)


def test_record_mirror_matches_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_ideal_info;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "double": 8, "float": 4, "int64_t": 8}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), sizes[ctype]) for n in names.split(",")]
    off, layout = 0, []
    for name, size in fields:       # natural alignment
        off = (off + size - 1) // size * size
        layout.append((name, off, size))
        off += size
    assert off == 20 == ctypes.sizeof(_lib.IdealInfo)           # no 8-byte member: no tail padding
    assert [f[0] for f in _lib.IdealInfo._fields_] == [n for n, _, _ in layout] == ["evals_ideal", "generations", "found", "refined", "ms_total"]
    for name, o, size in layout:
        fld = getattr(_lib.IdealInfo, name)
        assert (fld.offset, fld.size) == (o, size), name
    # the Julia mirror carries the same fields in the same order
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfIdealInfo\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = re.findall(r"(\w+)::(Int32|Float32|Float64)", jbody)
    assert [(n, {"Int32": 4, "Float32": 4, "Float64": 8}[t]) for n, t in jfields] == fields
    assert [t for _, t in jfields] == ["Int32"] * 4 + ["Float32"]
    for sym, fn in (("mrbf_ideal_point_problem", "hip_local_ideal_point"), ("mrbf_ideal_point_batch", "hip_local_ideal_points_many")):
        assert re.search(r"_locked\([^\n]*\) do \w+\s+ccall\(\(:%s, libmrbf\)" % sym, jl) and "function %s(" % fn in jl
    assert re.search(r"ideal_point::Symbol", jl) and "@assert ideal_point in (:host, :device)" in jl


def test_a_null_context_returns_minus_one(lib):
    from morbit.jl_amd import _lib

    d, k, ns = 3, 2, 2
    bufs = [np.full((ns, k), 7.0), np.full((ns, k, d), 7.0), np.full((ns, k), 7.0)]
    infos = (_lib.IdealInfo * ns)()
    ctypes.memset(infos, 0x55, ctypes.sizeof(infos))
    ms = ctypes.c_float(7.0)
    roles = (ctypes.c_int32 * k)(0, 1)
    handles = (ctypes.c_void_p * ns)()
    prob = _lib.PsProblem(n_models=1, n_objectives=k, models=handles, roles=roles, eq_tol=-1.0)
    opts = _lib.PsOptions(-1, -1, 0, 0, 0, -0.5, 1e-3)
    p = _lib.as_ptr
    X = np.zeros((ns, d))
    for with_args in (True, False):
        a = [p(X), p(X), p(X)] if with_args else [None] * 3
        pr, op = (ctypes.byref(prob), ctypes.byref(opts)) if with_args else (None, None)
        for n_starts in (ns, 0, 1 << 40):
            assert lib.mrbf_ideal_point_batch(None, n_starts, pr, handles if with_args else None, *a, op, None, p(bufs[0]), p(bufs[1]),
                                              p(bufs[2]), infos, ctypes.byref(ms)) == -1
        assert lib.mrbf_ideal_point_problem(None, pr, *a, op, p(bufs[0]), p(bufs[1]), p(bufs[2]), infos) == -1
    assert all(np.all(b == 7.0) for b in bufs) and ms.value == 7.0 and bytes(infos) == b"\x55" * ctypes.sizeof(infos)


class _FakeCtx:
    def check(self, rc):
        raise AssertionError("rc %d is an error" % rc)


class _FakeModel:
    num_outputs = 2
    ctx = _FakeCtx()


def _fake_plan(sc, objectives_only=False):
    return {"models": [_FakeModel()], "roles": [0, 1], "k": 2, "n_con": 0, "n_foreign": 0, "in_order": True}


def test_routing_of_compute_local_ideal_points_many(lib, monkeypatch):
    from morbit.jl_amd import descent
    from morbit.jl_amd import pascoletti_serafini as ps
    from morbit.jl_amd import surrogates as sg

    ns, d, k = ps.IDEAL_BATCH_MIN_STARTS, 3, 2             # the fewest starts that take the batch
    assert 2 <= ns <= 64
    containers = ["container %d" % p for p in range(ns)]
    rng = np.random.default_rng(0)
    X_n = rng.random((ns, d))
    LB, UB = X_n - 0.1, X_n + 0.1
    IDEAL = rng.standard_normal((ns, k))
    calls = {"batch": [], "single": [], "host": []}
    rc_batch = [0]

    def fake_batch(cfg, plans, X_n_, lb, ub, lin=None, seeds=None, eq_tol=-1.0, carry_constraints=True, out=None):
        calls["batch"].append((len(plans), list(seeds), carry_constraints, lin))
        return rc_batch[0], IDEAL.copy(), np.zeros((ns, k, d)), np.zeros((ns, k)), [dict(found=3)] * ns, 0.5

    def fake_single(cfg, plan, x_n, lb, ub, lin=None, seed=0, eq_tol=-1.0, carry_constraints=True):
        p = len(calls["single"])                 # the loop goes through the starts in order
        calls["single"].append((p, seed, carry_constraints, lin))
        return 0, IDEAL[p].copy(), np.zeros((k, d)), np.zeros(k), dict(found=3)

    def fake_host(x_n, lb, ub, ev, n_out, max_evals, rng_, eval_constraints=None, stats=None):
        calls["host"].append((n_out, max_evals))
        return np.full(n_out, -1.0)

    monkeypatch.setattr(sg, "container_plan", _fake_plan)
    monkeypatch.setattr(ps, "ideal_points_batch_device", fake_batch)
    monkeypatch.setattr(ps, "ideal_point_problem_device", fake_single)
    monkeypatch.setattr(ps, "compute_local_ideal_point", fake_host)
    cfg = descent.DirectedSearchConfig(ideal_point="device")
    lin = (None, None, np.ones((1, d)), np.ones(1))

    def clear():
        for v in calls.values():
            v.clear()

    # one shape, the table agrees: ONE batch call
    stats = {}
    seeds = list(range(7, 7 + ns))
    out = ps.compute_local_ideal_points_many(cfg, containers, X_n, LB, UB, seeds=seeds, stats=stats)
    assert np.array_equal(out, IDEAL) and stats["path"] == "batch" and stats["ms_total"] == 0.5 and len(stats["infos"]) == ns
    assert calls["batch"] == [(ns, seeds, True, None)] and not calls["single"] and not calls["host"]
    # seeds default to 0 per start; the linear rows and the switch travel
    clear()
    ps.compute_local_ideal_points_many(cfg, containers, X_n, LB, UB, lin=lin, carry_constraints=False)
    assert calls["batch"][0][:3] == (ns, [0] * ns, False) and calls["batch"][0][3] is lin
    # one start fewer than IDEAL_BATCH_MIN_STARTS: the loop of single calls
    clear()
    stats = {}
    m = ns - 1
    out = ps.compute_local_ideal_points_many(cfg, containers[:m], X_n[:m], LB[:m], UB[:m], seeds=seeds[:m], stats=stats)
    assert stats["path"] == "loop" and calls["single"] == [(p, seeds[p], True, None) for p in range(m)] and not calls["batch"]
    assert np.array_equal(out, IDEAL[:m])
    # the batch's row refuses (d = 257), the single call's does not: the loop
    clear()
    stats = {}
    big = np.zeros((ns, 257))
    out = ps.compute_local_ideal_points_many(cfg, containers, big, big - 0.1, big + 0.1, stats=stats)
    assert stats["path"] == "loop" and [c[0] for c in calls["single"]] == list(range(ns)) and not calls["batch"] and not calls["host"]
    # the batch call answers -2 after all: the loop likewise
    clear()
    rc_batch[0] = -2
    stats = {}
    ps.compute_local_ideal_points_many(cfg, containers, X_n, LB, UB, stats=stats)
    assert stats["path"] == "loop" and len(calls["batch"]) == 1 and len(calls["single"]) == ns
    rc_batch[0] = -3                                             # an error is an error
    with pytest.raises(AssertionError, match="rc -3"):
        ps.compute_local_ideal_points_many(cfg, containers, X_n, LB, UB)
    rc_batch[0] = 0
    # mixed plan shapes: the loop
    clear()
    shapes = iter([[0, 1], [1, 0]] + [[0, 1]] * (ns - 2))
    monkeypatch.setattr(sg, "container_plan",
                        lambda sc, objectives_only=False: dict(_fake_plan(sc), roles=next(shapes)))
    stats = {}
    ps.compute_local_ideal_points_many(cfg, containers, X_n, LB, UB, stats=stats)
    assert stats["path"] == "loop" and len(calls["single"]) == ns and not calls["batch"]
    # a shape both rows refuse (a foreign surrogate): the host search per start, with the configuration's budget
    clear()
    monkeypatch.setattr(sg, "container_plan",
                        lambda sc, objectives_only=False: dict(_fake_plan(sc), n_foreign=1))
    stats = {}
    out = ps.compute_local_ideal_points_many(cfg, containers, X_n, LB, UB, stats=stats)
    assert stats["path"] == "reference" and calls["host"] == [(k, 500 * (d + 1))] * ns and not calls["batch"] and not calls["single"]
    assert np.array_equal(out, np.full((ns, k), -1.0))
    # modelled constraints that are carried count for the table, those that are not do not
    clear()
    monkeypatch.setattr(sg, "container_plan",
                        lambda sc, objectives_only=False: dict(_fake_plan(sc), n_con=33))
    stats = {}
    ps.compute_local_ideal_points_many(cfg, containers, X_n, LB, UB, carry_constraints=False, stats=stats)
    assert stats["path"] == "batch" and calls["batch"][0][2] is False


def _ds_stubs(monkeypatch, ns, d, k, gave_up=None):
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import pascoletti_serafini as ps

    rng = np.random.default_rng(1)
    log = {"ideal": [], "device": [], "crit": [], "step": [], "host": []}
    IDEAL = rng.standard_normal((ns, k))

    def fake_many(cfg, containers, X_n, lb_effs, ub_effs, lin=None, seeds=None, carry_constraints=True, stats=None, scal=None, eq_tol=1e-8):
        log["ideal"].append(dict(n=len(containers), X_n=np.array(X_n), lb=np.array(lb_effs), ub=np.array(ub_effs), lin=lin, seeds=seeds,
                                 carry=carry_constraints))
        if stats is not None:
            stats["path"] = "batch" if len(containers) >= 2 else "loop"
        return IDEAL[:len(containers)].copy()

    def fake_device(plans, cfg, X_, X_n_, deltas_, lb_, ub_, R, out=None):
        log["device"].append(np.array(R))
        recs = [dict(ds_status=_lib.DS_GAVE_UP if p == gave_up else _lib.DS_OK, iterations=4, dropped=0, branch=0, loops=2, reserved=0,
                     omega=0.5 + p, omega_step=0.5 + p, sigma=0.1, step_norm=0.01 * (p + 1), dnorm=0.75, branch_name="delta") for p in range(ns)]
        return 0, np.ones((ns, d)), np.ones((ns, d)), np.ones((ns, k)), np.zeros((ns, k)), recs, 0.25

    def fake_crit(cfg, sc, scal, x, x_n, fx_n, delta, lb_, ub_, lin=None, stats=None, rng=None, r=None, seed=0):
        log["crit"].append((sc, None if r is None else np.array(r)))
        return 7.0, np.full(d, 0.25)

    def fake_step(cfg, sc, scal, x, x_n, delta, lb_, ub_, omega, dd, lin=None, stats=None):
        log["step"].append(sc)
        return omega, np.full(d, 1.5), np.full(k, 2.5), 0.125

    def fake_host(*a, **kw):
        log["host"].append(a)
        return np.full(k, -5.0)

    monkeypatch.setattr(descent.sg, "container_plan", _fake_plan)
    monkeypatch.setattr(ps, "compute_local_ideal_points_many", fake_many)
    monkeypatch.setattr(ps, "compute_local_ideal_point", fake_host)
    monkeypatch.setattr(descent, "ds_iterate_batch_device", fake_device)
    monkeypatch.setattr(descent, "compute_descent_step_ds", fake_step)
    return log, IDEAL, fake_crit


def test_routing_of_ds_iterate_many_with_device_ideal_points(lib, monkeypatch):
    from morbit.jl_amd import descent

    ns, d, k, gave_up = 5, 3, 2, 3
    log, IDEAL, fake_crit = _ds_stubs(monkeypatch, ns, d, k, gave_up)
    monkeypatch.setattr(descent, "get_criticality_ds", fake_crit)
    containers = ["container %d" % p for p in range(ns)]
    rng = np.random.default_rng(0)
    X, X_n, deltas = rng.uniform(0.3, 0.7, (ns, d)), rng.uniform(0.3, 0.7, (ns, d)), np.full(ns, 0.2)
    FX_n = rng.standard_normal((ns, k))
    lb, ub = np.zeros(d), np.ones(d)
    cfg = descent.DirectedSearchConfig(ideal_point="device")
    stats = {}
    res = descent.ds_iterate_many(cfg, containers, None, X, X_n, FX_n, deltas, lb, ub, stats=stats, seeds=[5, 6, 7, 8, 9])
    # ONE ideal-point call for all starts, before the one batch call: today's box per start, the box only, the seeds
    assert len(log["ideal"]) == 1 and len(log["device"]) == 1 and not log["host"]
    c = log["ideal"][0]
    assert c["n"] == ns and c["carry"] is False and c["lin"] is None and c["seeds"] == [5, 6, 7, 8, 9] and np.array_equal(c["X_n"], X_n)
    for p in range(ns):
        lo, hi = descent._local_bounds(X[p], cfg.reference_trust_region_factor * 0.2, lb, ub)
        assert np.array_equal(c["lb"][p], lo) and np.array_equal(c["ub"][p], hi)
    assert np.array_equal(log["device"][0], IDEAL - FX_n)
    assert stats["path"] == "batch" and stats["ideal_point_path"] == "device" and stats["image_direction"] == "ideal_point"
    assert stats["rerouted"] == [gave_up] and len(res) == ns
    # the start whose QP gave up goes through the single functions WITH its r
    assert [c_[0] for c_ in log["crit"]] == [containers[gave_up]] and np.array_equal(log["crit"][0][1], IDEAL[gave_up] - FX_n[gave_up])
    # linear rows: the loop of single functions, the ideal points still from one call, every start handed its r
    for v in log.values():
        v.clear()
    stats = {}
    lin = (np.ones((1, d)), np.zeros(1), None, None)
    descent.ds_iterate_many(cfg, containers, None, X, X_n, FX_n, deltas, lb, ub, lin=lin, stats=stats)
    assert stats["path"] == "loop" and stats["ideal_point_path"] == "device" and len(log["ideal"]) == 1 and not log["device"]
    assert log["ideal"][0]["carry"] is False and log["ideal"][0]["lin"] is None and log["ideal"][0]["seeds"] is None
    assert [c_[0] for c_ in log["crit"]] == containers
    assert all(np.array_equal(c_[1], IDEAL[p] - FX_n[p]) for p, c_ in enumerate(log["crit"]))
    # a reference point: arithmetic, no ideal-point call of any kind
    for v in log.values():
        v.clear()
    descent.ds_iterate_many(descent.DirectedSearchConfig(ideal_point="device", reference_point=[-3.0, -4.0]), containers, None, X, X_n, FX_n,
                            deltas, lb, ub)
    assert not log["ideal"] and not log["host"] and np.array_equal(log["device"][0], np.array([-3.0, -4.0]) - FX_n)


def test_get_criticality_ds_takes_the_single_device_call(lib, monkeypatch):
    from morbit.jl_amd import _lib, descent

    d, k = 3, 2
    log, IDEAL, _ = _ds_stubs(monkeypatch, 1, d, k)
    seen = {}

    def fake_qp(plan, x_n, lb, ub, r, want_mult=False):
        seen["r"] = np.array(r)
        return 0, 0.5, np.array([0.5, -0.25, 0.125]), dict(status=_lib.DS_OK)

    monkeypatch.setattr(descent, "ds_criticality_device", fake_qp)
    x, x_n, fx_n = np.full(d, 0.5), np.full(d, 0.45), np.array([1.0, 2.0])
    cfg = descent.DirectedSearchConfig(ideal_point="device")
    stats = {}
    om, dn = descent.get_criticality_ds(cfg, "sc", None, x, x_n, fx_n, 0.2, np.zeros(d), np.ones(d), stats=stats, seed=42)
    assert len(log["ideal"]) == 1 and not log["host"]
    c = log["ideal"][0]
    lo, hi = descent._local_bounds(x, 1.1 * 0.2, np.zeros(d), np.ones(d))
    assert c["n"] == 1 and c["carry"] is False and c["seeds"] == [42] and np.array_equal(c["lb"][0], lo) and np.array_equal(c["ub"][0], hi)
    assert np.array_equal(seen["r"], IDEAL[0] - fx_n) and stats["ideal_point_path"] == "device" and stats["path"] == "device"
    assert om == 0.5 and np.array_equal(dn, np.array([1.0, -0.5, 0.25]))
    # a given r: no search at all
    log["ideal"].clear()
    descent.get_criticality_ds(cfg, "sc", None, x, x_n, fx_n, 0.2, np.zeros(d), np.ones(d), r=[-1.0, -2.0])
    assert not log["ideal"] and not log["host"] and np.array_equal(seen["r"], [-1.0, -2.0])


def test_the_default_configuration_does_not_touch_the_new_symbols(lib, monkeypatch):
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import pascoletti_serafini as ps

    ns, d, k = 3, 3, 2
    log, IDEAL, _ = _ds_stubs(monkeypatch, ns, d, k)

    def boom(*a, **kw):
        raise AssertionError("the default configuration reached an ideal-point device path")

    for name in ("compute_local_ideal_points_many", "ideal_points_batch_device", "ideal_point_problem_device"):
        monkeypatch.setattr(ps, name, boom)
    monkeypatch.setattr(descent.sg, "eval_container_objectives_at_scaled_sites", lambda sc, scal, X: np.zeros((np.atleast_2d(X).shape[0], k)))
    monkeypatch.setattr(descent, "ds_criticality_device",
                        lambda plan, x_n, lb, ub, r, want_mult=False: (0, 0.5, np.array([0.5, -0.25, 0.125]), dict(status=_lib.DS_OK)))
    cfg = descent.DirectedSearchConfig()
    assert cfg.ideal_point == "host"
    with pytest.raises(AssertionError):
        descent.DirectedSearchConfig(ideal_point="gpu")
    rng = np.random.default_rng(0)
    X, X_n, FX_n = rng.uniform(0.3, 0.7, (ns, d)), rng.uniform(0.3, 0.7, (ns, d)), rng.standard_normal((ns, k))
    stats = {}
    descent.ds_iterate_many(cfg, ["a", "b", "c"], None, X, X_n, FX_n, np.full(ns, 0.2), np.zeros(d), np.ones(d), stats=stats)
    assert len(log["host"]) == ns and stats["path"] == "batch" and stats["ideal_point_path"] == "reference"
    assert np.array_equal(log["device"][0], np.full((ns, k), -5.0) - FX_n)              # the host search's ideal point per start
    stats = {}
    descent.get_criticality_ds(cfg, "a", None, X[0], X_n[0], FX_n[0], 0.2, np.zeros(d), np.ones(d), stats=stats)
    assert len(log["host"]) == ns + 1 and stats["ideal_point_path"] == "reference"


def test_ideal_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "ideal_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "ideal_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "ideal_host_check: ok" in res.stdout


def test_host_header_includes_no_hip_and_the_phase_exists_once():
    text = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ideal_host.hpp")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower()
    src = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ps_solver.hip")).read()
    assert '#include "ideal_host.hpp"' in src
    # one copy of the ideal-point block: one place makes the single-objective runs, one place reads their best records
    assert src.count("ps_make_run(a.runs[l], 0, l, lam_ip") == 1
    assert len(re.findall(r"^static int ps_ideal_phase\(", src, flags=re.M)) == 1
    assert src.count("MRBF_TRY(ps_ideal_phase(c))") == 1            # and one place runs it, for the step and the ideal-point calls alike
    assert "ideal_only" not in src
