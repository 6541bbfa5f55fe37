"""CPU tests of the many-start normal-step entry (mrbf_normal_step_batch): its decision-table row, the record's struct mirror against
the header, and the routing of `descent.normal_steps_many` -- one start whose LP gave up goes through the single-start function, the
others do not.  No GPU: the device call is replaced by a stub."""
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


# (n_starts, d, n_models, n_nl, n_lin, n_foreign): the C4 shape with one modelled and two linear rows
C4 = (64, 128, 2, 1, 2, 0)


def _row(**kw):
    names = ("n_starts", "d", "n_models", "n_nl", "n_lin", "n_foreign")
    v = dict(zip(names, C4))
    v.update(kw)
    return tuple(v[n] for n in names)


@pytest.mark.parametrize("args, device", [
    (C4, True),
    (_row(n_starts=0), False),
    (_row(n_starts=1), True),
    (_row(n_starts=65535), True),
    (_row(n_starts=65536), False),
    (_row(d=256), True),                                      # modelled rows: the fused evaluation kernels' range
    (_row(d=257), False),
    (_row(d=257, n_models=0, n_nl=0), True),                  # linear rows alone need no evaluation
    (_row(d=4096, n_models=0, n_nl=0), True),
    (_row(d=4097, n_models=0, n_nl=0), False),
    (_row(d=4096, n_models=1, n_nl=0), True),                 # a model without constraint rows is not evaluated either
    (_row(n_nl=4, n_lin=60), True),                           # 64 rows
    (_row(n_nl=5, n_lin=60), False),                          # 65 rows
    (_row(n_nl=0, n_lin=64, n_models=0), True),
    (_row(n_nl=0, n_lin=65, n_models=0), False),
    (_row(n_nl=0, n_lin=0), False),                           # no row: nothing to step towards
    (_row(n_foreign=1), False),                               # a constraint row on a foreign surrogate
    (_row(d=0), False),
])
def test_decision_table_row(lib, args, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_normal_batch(*args) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)
    if device:  # the batch never takes what the single call would refuse
        assert lib.mrbf_dispatch_normal(*args[1:]) == _lib.DISPATCH_DEVICE


def test_return_codes_that_mean_reference(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_NORMAL_BATCH == 12
    assert lib.mrbf_dispatch_after(12, -2) == 1 and lib.mrbf_dispatch_after(12, -3) == 0 and lib.mrbf_dispatch_after(12, 0) == 0
    assert lib.mrbf_dispatch_after(12, -1) == 0 and lib.mrbf_dispatch_after(12, _lib.MRBF_ENOMEM) == 0
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_NORMAL_BATCH = 12\b", text)


def test_record_mirror_matches_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_normal_batch_record;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "double": 8, "float": 4, "int64_t": 8}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), sizes[ctype]) for n in names.split(",")]
    assert [n for n, _ in fields] == ["status", "iterations", "bound_flips", "reserved", "alpha", "delta"]
    off, layout = 0, []
    for name, size in fields:       # natural alignment
        off = (off + size - 1) // size * size
        layout.append((name, off, size))
        off += size
    total = (off + 7) // 8 * 8
    assert total == 32 == ctypes.sizeof(_lib.NormalBatchRecord)
    assert [f[0] for f in _lib.NormalBatchRecord._fields_] == [n for n, _, _ in layout]
    for name, o, size in layout:
        fld = getattr(_lib.NormalBatchRecord, name)
        assert (fld.offset, fld.size) == (o, size), name
    # the Julia mirror carries the same fields in the same order
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfNormalBatchRecord\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = re.findall(r"(\w+)::(Int32|Float64)", jbody)
    assert [(n, {"Int32": 4, "Float64": 8}[t]) for n, t in jfields] == fields


def test_both_bindings_declare_the_entry(lib):
    from morbit.jl_amd import _lib

    assert "mrbf_normal_step_batch" in _lib.SIGNATURES and "mrbf_dispatch_normal_batch" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mrbf_normal_step_batch"][1]) == 17
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    assert re.search(r"^function hip_normal_steps_many\(", jl, flags=re.M)
    assert re.search(r"_locked\([^\n]*\) do \w+\s+ccall\(\(:mrbf_normal_step_batch, libmrbf\)", jl)


class _FakeModel:
    num_outputs = 2
    ctx = None


def test_a_start_that_gave_up_takes_the_single_start_function(lib, monkeypatch):
    from morbit.jl_amd import _lib, descent

    ns, d = 5, 3
    gave_up = 3
    containers = ["container %d" % p for p in range(ns)]

    def fake_plan(sc, objectives_only=False):
        return {"models": [_FakeModel()], "roles": [_lib.ROLE_INEQ, _lib.ROLE_EQ], "k": 0, "n_con": 0 if objectives_only else 2,
                "n_foreign": 0, "in_order": True}

    rng = np.random.default_rng(0)
    X, deltas = rng.standard_normal((ns, d)), np.array([0.3, 0.25, 0.4, 0.35, 0.3])
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    N = rng.standard_normal((ns, d))
    N[gave_up] = np.nan
    device_calls = []

    def fake_device(plans, X_, lb_, ub_, deltas_, lin=None, kappa_delta=1.0, delta_max=np.inf, variable_radius=False, out=None,
                    want_duals=False):
        device_calls.append((len(plans), kappa_delta, delta_max, variable_radius))
        recs = [dict(status=_lib.NS_GAVE_UP if p == gave_up else _lib.NS_OK, iterations=4, bound_flips=1, reserved=0, alpha=0.1 * (p + 1),
                     delta=-np.inf if p == gave_up else float(deltas_[p])) for p in range(ns)]
        n, x_n = out if out is not None else (np.empty((ns, d)), np.empty((ns, d)))
        n[:], x_n[:] = N, X_ + N
        return 0, n, x_n, recs, 0.25

    single = []

    def fake_single(sc, scal, x, delta, lb_, ub_, lin=None, kappa_delta=1.0, delta_max=np.inf, variable_radius=False, stats=None):
        single.append((sc, delta, kappa_delta, delta_max, variable_radius))
        return np.full(d, 0.25), 0.125

    monkeypatch.setattr(descent.sg, "container_plan", fake_plan)
    monkeypatch.setattr(descent, "normal_step_batch_device", fake_device)
    monkeypatch.setattr(descent, "compute_normal_step", fake_single)
    stats = {}
    x_n = np.empty((ns, d))
    res = descent.normal_steps_many(containers, None, X, deltas, lb, ub, kappa_delta=0.5, delta_max=7.0, variable_radius=True, stats=stats,
                                    x_n_out=x_n)
    assert device_calls == [(ns, 0.5, 7.0, True)]
    assert stats["path"] == "batch" and stats["rerouted"] == [gave_up] and len(stats["records"]) == ns and stats["ms_total"] == 0.25
    assert single == [(containers[gave_up], 0.35, 0.5, 7.0, True)]
    assert len(res) == ns
    for p, (n, dl) in enumerate(res):
        if p == gave_up:
            assert np.array_equal(n, np.full(d, 0.25)) and dl == 0.125 and np.array_equal(x_n[p], X[p] + 0.25)
        else:
            assert np.array_equal(n, N[p]) and dl == deltas[p] and np.array_equal(x_n[p], X[p] + N[p])
    # a shape the decision table refuses (modelled rows at d = 257): the device entry is not called, every start takes the single call
    single.clear(), device_calls.clear()
    stats = {}
    res = descent.normal_steps_many(containers, None, np.zeros((ns, 257)), deltas, np.zeros(257), np.ones(257), stats=stats)
    assert device_calls == [] and stats["path"] == "loop" and stats["rerouted"] == []
    assert [s[0] for s in single] == containers and [s[1] for s in single] == list(deltas) and len(res) == ns
    # containers of different shapes: likewise
    shapes = iter([[-3, -2], [-2, -3], [-3, -2], [-3, -2], [-3, -2]])
    monkeypatch.setattr(descent.sg, "container_plan",
                        lambda sc, objectives_only=False: dict(fake_plan(sc, objectives_only), roles=[-3, -2] if objectives_only else next(shapes)))
    single.clear()
    stats = {}
    descent.normal_steps_many(containers, None, X, deltas, lb, ub, stats=stats)
    assert device_calls == [] and stats["path"] == "loop" and [s[0] for s in single] == containers
