"""CPU tests of the many-start steepest-descent entry (mrbf_sd_iterate_batch): its decision-table row, the record's struct mirror
against the header, and the routing of `descent.sd_iterate_many` -- one start whose direction LP gave up goes through the single-start
functions, the others do not.  No GPU: the device call is replaced by a stub."""
import ctypes
import os
import re

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
    (_row(n_starts=65535, d=256), True),
    (_row(d=257), False),
    (_row(n_starts=0), False),
    (_row(n_starts=65536), False),
    (_row(n_foreign=1), False),
    (_row(n_nl=3, n_lin=60), False),          # 2 + 3 + 60 = 65 LP rows
    (_row(n_nl=2, n_lin=60), True),           # 64 rows
    (_row(max_loops=1025), False),
    (_row(max_loops=1024), True),
])
def test_decision_table_row(lib, args, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_sd_batch(*args) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)
    if device:  # the batch never takes what one of the single calls would refuse
        assert lib.mrbf_dispatch_sd(*args[1:7]) == _lib.DISPATCH_DEVICE and lib.mrbf_dispatch_sd_step(*args[1:]) == _lib.DISPATCH_DEVICE


def test_return_codes_that_mean_reference(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_SD_BATCH == 9
    assert lib.mrbf_dispatch_after(9, -2) == 1 and lib.mrbf_dispatch_after(9, -3) == 0 and lib.mrbf_dispatch_after(9, 0) == 0
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_SD_BATCH = 9\b", text)


def test_record_mirror_matches_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_sd_batch_record;", text).group(1)
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
    assert total == 56 == ctypes.sizeof(_lib.SdBatchRecord)
    assert [f[0] for f in _lib.SdBatchRecord._fields_] == [n for n, _, _ in layout]
    for name, o, size in layout:
        fld = getattr(_lib.SdBatchRecord, name)
        assert (fld.offset, fld.size) == (o, size), name
    # the Julia mirror carries the same fields in the same order
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfSdBatchRecord\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = re.findall(r"(\w+)::(Int32|Float64)", jbody)
    assert [(n, {"Int32": 4, "Float64": 8}[t]) for n, t in jfields] == fields


class _FakeModel:
    num_outputs = 2
    ctx = None


def test_a_start_that_gave_up_takes_the_single_start_functions(lib, monkeypatch):
    from morbit.jl_amd import _lib, descent

    ns, d, k = 5, 3, 2
    gave_up = 3
    containers = ["container %d" % p for p in range(ns)]
    plan_calls = []

    def fake_plan(sc, objectives_only=False):
        plan_calls.append(sc)
        return {"models": [_FakeModel()], "roles": [0, 1], "k": k, "n_con": 0, "n_foreign": 0, "in_order": True}

    rng = np.random.default_rng(0)
    X, X_n, deltas = rng.standard_normal((ns, d)), rng.standard_normal((ns, d)), np.full(ns, 0.3)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    D, XP, MXP = rng.standard_normal((ns, d)), rng.standard_normal((ns, d)), rng.standard_normal((ns, k))
    D[gave_up], XP[gave_up], MXP[gave_up] = np.nan, np.nan, np.nan
    device_calls = []

    def fake_device(plans, cfg, X_, X_n_, deltas_, lb_, ub_, lin=None, out=None):
        device_calls.append(len(plans))
        recs = []
        for p in range(ns):
            recs.append(dict(sd_status=_lib.SD_GAVE_UP if p == gave_up else _lib.SD_OK, iterations=4, bound_flips=1, branch=0, loops=2,
                             reserved=0, omega=0.5 + p, omega_step=0.5 + p, sigma=0.1, step_norm=0.01 * (p + 1), branch_name="delta"))
        return 0, D.copy(), XP.copy(), MXP.copy(), recs, 0.25

    single = {"crit": [], "step": []}

    def fake_crit(cfg, sc, scal, x, x_n, lb_, ub_, lin=None, stats=None):
        single["crit"].append(sc)
        return 7.0, np.full(d, 0.25)

    def fake_step(cfg, sc, scal, x, x_n, delta, lb_, ub_, omega, dd, lin=None, stats=None):
        single["step"].append((sc, omega, delta))
        return omega, np.full(d, 1.5), np.full(k, 2.5), 0.125

    monkeypatch.setattr(descent.sg, "container_plan", fake_plan)
    monkeypatch.setattr(descent, "sd_iterate_batch_device", fake_device)
    monkeypatch.setattr(descent, "get_criticality_sd", fake_crit)
    monkeypatch.setattr(descent, "compute_descent_step_sd_routed", fake_step)
    cfg = descent.SteepestDescentConfig()
    stats = {}
    res = descent.sd_iterate_many(cfg, containers, None, X, X_n, deltas, lb, ub, stats=stats)
    assert device_calls == [ns]
    assert stats["path"] == "batch" and stats["rerouted"] == [gave_up]
    assert single["crit"] == [containers[gave_up]] and single["step"] == [(containers[gave_up], 7.0, 0.3)]
    assert len(res) == ns
    for p, (om, dd, xp, mxp, nrm) in enumerate(res):
        if p == gave_up:
            assert om == 7.0 and np.array_equal(dd, np.full(d, 0.25)) and np.array_equal(xp, np.full(d, 1.5))
            assert np.array_equal(mxp, np.full(k, 2.5)) and nrm == 0.125
        else:
            assert om == 0.5 + p and nrm == 0.01 * (p + 1)
            assert np.array_equal(dd, D[p]) and np.array_equal(xp, XP[p]) and np.array_equal(mxp, MXP[p])
    # a shape the decision table refuses (d = 257): the device entry is not called, every start takes the single-start functions
    single["crit"].clear(), single["step"].clear(), device_calls.clear()
    stats = {}
    res = descent.sd_iterate_many(cfg, containers, None, np.zeros((ns, 257)), np.zeros((ns, 257)), deltas, np.zeros(257), np.ones(257),
                                  stats=stats)
    assert device_calls == [] and stats["path"] == "loop" and stats["rerouted"] == []
    assert single["crit"] == containers and [s[0] for s in single["step"]] == containers and len(res) == ns
    # containers of different shapes: likewise
    shapes = iter([[0, 1], [1, 0], [0, 1], [0, 1], [0, 1]])
    monkeypatch.setattr(descent.sg, "container_plan", lambda sc, objectives_only=False: dict(fake_plan(sc), roles=next(shapes)))
    single["crit"].clear(), single["step"].clear()
    stats = {}
    descent.sd_iterate_many(cfg, containers, None, X, X_n, deltas, lb, ub, stats=stats)
    assert device_calls == [] and stats["path"] == "loop" and single["crit"] == containers
