"""CPU tests of the many-start directed-search entry (mrbf_ds_iterate_batch): its decision-table row, the record's struct mirror
against the header and the Julia struct, the NULL-context answer, the routing of `descent.ds_iterate_many` -- one start whose
direction QP gave up goes through the single-start functions, the others do not; refused shapes, mixed containers and linear rows
take the loop -- and the host logic of the device call (tools/ds_batch_host_check.cpp, a stand-alone program under AddressSanitizer and
UBSan, run as a child process).  No GPU: the device call is replaced by a stub."""
import ctypes
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


# (n_starts, d, k, n_models, n_nl, n_lin, n_foreign, max_loops)
C4 = (64, 128, 2, 1, 0, 0, 0, 117)


def _row(**kw):
    names = ("n_starts", "d", "k", "n_models", "n_nl", "n_lin", "n_foreign", "max_loops")
    v = dict(zip(names, C4))
    v.update(kw)
    return tuple(v[n] for n in names)


@pytest.mark.parametrize("args, device", [
    (C4, True),
    (_row(n_starts=1), True),
    (_row(n_starts=65535), True),
    (_row(n_starts=0), False),
    (_row(n_starts=65536), False),
    (_row(d=256), True),
    (_row(d=257), False),
    (_row(k=16), True),
    (_row(k=17), False),
    (_row(n_nl=1), False),
    (_row(n_lin=1), False),
    (_row(n_foreign=1), False),
    (_row(max_loops=1024), True),
    (_row(max_loops=1025), False),
])
def test_decision_table_row(lib, args, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_ds_batch(*args) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)
    if device:  # the batch never takes what one of the single calls would refuse
        assert lib.mrbf_dispatch_ds(*args[1:7]) == _lib.DISPATCH_DEVICE and lib.mrbf_dispatch_sd_step(*args[1:]) == _lib.DISPATCH_DEVICE


def test_return_codes_that_mean_reference(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_DS_BATCH == 23
    assert lib.mrbf_dispatch_after(23, -2) == 1 and lib.mrbf_dispatch_after(23, -3) == 0 and lib.mrbf_dispatch_after(23, 0) == 0
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_DS_BATCH = 23\b", text)


def test_record_mirror_matches_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_ds_batch_record;", text).group(1)
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
    total = (off + 7) // 8 * 8
    assert total == 64 == ctypes.sizeof(_lib.DsBatchRecord)
    assert [f[0] for f in _lib.DsBatchRecord._fields_] == [n for n, _, _ in layout]
    assert [n for n, _, _ in layout] == ["ds_status", "iterations", "dropped", "branch", "loops", "reserved", "omega", "omega_step", "sigma",
                                        "step_norm", "dnorm"]
    for name, o, size in layout:
        fld = getattr(_lib.DsBatchRecord, name)
        assert (fld.offset, fld.size) == (o, size), name
    # the Julia mirror carries the same fields in the same order
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfDsBatchRecord\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = re.findall(r"(\w+)::(Int32|Float64)", jbody)
    assert [(n, {"Int32": 4, "Float64": 8}[t]) for n, t in jfields] == fields
    assert re.search(r"ccall\(\(:mrbf_ds_iterate_batch, libmrbf\)", jl) and "function hip_ds_iterate_many(" in jl


def test_a_null_context_returns_minus_one(lib):
    from morbit.jl_amd import _lib

    d, k, ns = 3, 2, 2
    bufs = [np.full((ns, d), 7.0), np.full((ns, d), 7.0), np.full((ns, k), 7.0), np.full((ns, k), 7.0)]
    recs = (_lib.DsBatchRecord * ns)()
    ctypes.memset(recs, 0x55, ctypes.sizeof(recs))
    ms = ctypes.c_float(7.0)
    roles = (ctypes.c_int32 * k)(0, 1)
    handles = (ctypes.c_void_p * ns)()
    prob = _lib.PsProblem(n_models=1, n_objectives=k, models=handles, roles=roles, eq_tol=-1.0)
    opts = _lib.SdStepOptions(strict=1, max_loops=6, const_rhs=1e-6, shrink=0.75, min_stepsize=1e-15)
    p = _lib.as_ptr
    X = np.zeros((ns, d))
    args = [p(X), p(X), p(np.ones(ns)), p(np.zeros(d)), p(np.ones(d)), p(-np.ones((ns, k)))]
    for n_starts in (ns, 0, 1 << 40):
        for with_args in (True, False):
            a = args if with_args else [None] * 6
            rc = lib.mrbf_ds_iterate_batch(None, n_starts, ctypes.byref(prob) if with_args else None, handles if with_args else None, *a,
                                           ctypes.byref(opts) if with_args else None, p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), recs,
                                           ctypes.byref(ms))
            assert rc == -1
    assert all(np.all(b == 7.0) for b in bufs) and ms.value == 7.0 and bytes(recs) == b"\x55" * ctypes.sizeof(recs)


class _FakeModel:
    num_outputs = 2
    ctx = None


def test_routing_of_ds_iterate_many(lib, monkeypatch):
    from morbit.jl_amd import _lib, descent

    ns, d, k = 5, 3, 2
    gave_up = 3
    containers = ["container %d" % p for p in range(ns)]

    def fake_plan(sc, objectives_only=False):
        return {"models": [_FakeModel()], "roles": [0, 1], "k": k, "n_con": 0, "n_foreign": 0, "in_order": True}

    rng = np.random.default_rng(0)
    X, X_n, deltas = rng.standard_normal((ns, d)), rng.standard_normal((ns, d)), np.full(ns, 0.3)
    FX_n = rng.standard_normal((ns, k))
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    D, XP, MXP = rng.standard_normal((ns, d)), rng.standard_normal((ns, d)), rng.standard_normal((ns, k))
    D[gave_up], XP[gave_up], MXP[gave_up] = np.nan, np.nan, np.nan
    device_calls = []

    def fake_device(plans, cfg, X_, X_n_, deltas_, lb_, ub_, R, out=None):
        device_calls.append((len(plans), np.array(R)))
        recs = []
        for p in range(ns):
            recs.append(dict(ds_status=_lib.DS_GAVE_UP if p == gave_up else _lib.DS_OK, iterations=4, dropped=1, branch=0, loops=2,
                             reserved=0, omega=0.5 + p, omega_step=0.5 + p, sigma=0.1, step_norm=0.01 * (p + 1), dnorm=0.75,
                             branch_name="delta"))
        return 0, D.copy(), XP.copy(), MXP.copy(), np.zeros((ns, k)), recs, 0.25

    single = {"crit": [], "step": []}

    def fake_crit(cfg, sc, scal, x, x_n, fx_n, delta, lb_, ub_, lin=None, stats=None, rng=None):
        single["crit"].append(sc)
        return 7.0, np.full(d, 0.25)

    def fake_step(cfg, sc, scal, x, x_n, delta, lb_, ub_, omega, dd, lin=None, stats=None):
        single["step"].append((sc, omega, delta))
        return omega, np.full(d, 1.5), np.full(k, 2.5), 0.125

    monkeypatch.setattr(descent.sg, "container_plan", fake_plan)
    monkeypatch.setattr(descent, "ds_iterate_batch_device", fake_device)
    monkeypatch.setattr(descent, "get_criticality_ds", fake_crit)
    monkeypatch.setattr(descent, "compute_descent_step_ds", fake_step)
    ref_point = [-3.0, -4.0]
    cfg = descent.DirectedSearchConfig(reference_point=ref_point)
    stats = {}
    res = descent.ds_iterate_many(cfg, containers, None, X, X_n, FX_n, deltas, lb, ub, stats=stats)
    assert [c[0] for c in device_calls] == [ns]
    assert np.array_equal(device_calls[0][1], np.asarray(ref_point) - FX_n)          # r per start: the reference point minus f(x_n)
    assert stats["path"] == "batch" and stats["rerouted"] == [gave_up] and stats["image_direction"] == "reference_point"
    assert len(stats["records"]) == ns and stats["ms_total"] == 0.25
    assert single["crit"] == [containers[gave_up]] and single["step"] == [(containers[gave_up], 7.0, 0.3)]
    assert len(res) == ns
    for p, (om, dd, xp, mxp, nrm) in enumerate(res):
        if p == gave_up:
            assert om == 7.0 and np.array_equal(dd, np.full(d, 0.25)) and np.array_equal(xp, np.full(d, 1.5))
            assert np.array_equal(mxp, np.full(k, 2.5)) and nrm == 0.125
        else:
            assert om == 0.5 + p and nrm == 0.01 * (p + 1)
            assert np.array_equal(dd, D[p]) and np.array_equal(xp, XP[p]) and np.array_equal(mxp, MXP[p])
    # a reference direction: r = -direction for every start
    device_calls.clear(), single["crit"].clear(), single["step"].clear()
    stats = {}
    descent.ds_iterate_many(descent.DirectedSearchConfig(reference_direction=[1.0, 2.0]), containers, None, X, X_n, FX_n, deltas, lb, ub,
                            stats=stats)
    assert np.array_equal(device_calls[0][1], np.tile([-1.0, -2.0], (ns, 1))) and stats["image_direction"] == "reference_direction"

    def loop_taken(stats_):
        assert device_calls == [] and stats_["path"] == "loop" and stats_["rerouted"] == []
        assert single["crit"] == containers and [s[0] for s in single["step"]] == containers

    # a shape the decision table refuses (d = 257): the device entry is not called, every start takes the single-start functions
    single["crit"].clear(), single["step"].clear(), device_calls.clear()
    stats = {}
    res = descent.ds_iterate_many(cfg, containers, None, np.zeros((ns, 257)), np.zeros((ns, 257)), FX_n, deltas, np.zeros(257), np.ones(257),
                                  stats=stats)
    loop_taken(stats)
    assert len(res) == ns
    # linear rows present: likewise
    single["crit"].clear(), single["step"].clear()
    stats = {}
    lin = (np.ones((1, d)), np.zeros(1), None, None)
    res = descent.ds_iterate_many(cfg, containers, None, X, X_n, FX_n, deltas, lb, ub, lin=lin, stats=stats)
    loop_taken(stats)
    assert len(res) == ns
    # containers of different roles: likewise
    shapes = iter([[0, 1], [1, 0], [0, 1], [0, 1], [0, 1]])
    monkeypatch.setattr(descent.sg, "container_plan", lambda sc, objectives_only=False: dict(fake_plan(sc), roles=next(shapes)))
    single["crit"].clear(), single["step"].clear()
    stats = {}
    res = descent.ds_iterate_many(cfg, containers, None, X, X_n, FX_n, deltas, lb, ub, stats=stats)
    loop_taken(stats)
    assert len(res) == ns


def test_ds_normalise_is_the_rule_of_get_criticality_ds():
    from morbit.jl_amd import _lib, descent

    d = np.array([0.25, -0.5, 0.125])
    om, dn = descent._ds_normalise(0.75, d, _lib.DS_OK, 3)
    assert om == 0.75 and np.array_equal(dn, d / 0.5)
    for status, dd in ((_lib.DS_CRITICAL, d), (_lib.DS_INFEASIBLE, d), (_lib.DS_GAVE_UP, np.full(3, np.nan)), (_lib.DS_OK, np.zeros(3))):
        om, dn = descent._ds_normalise(0.75, dd, status, 3)
        assert om == 0.0 and np.array_equal(dn, np.zeros(3))


def test_ds_batch_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "ds_batch_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "ds_batch_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "ds_batch_host_check: ok" in res.stdout


def test_host_header_includes_no_hip():
    text = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ds_batch_host.hpp")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower()
    assert '#include "ds_batch_host.hpp"' in open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ds_batch.hip")).read()
