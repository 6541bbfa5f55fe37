"""CPU tests of the many-start Pascoletti-Serafini entry (mrbf_ps_step_batch): its decision-table row, the return codes that mean
"take the single call", the ctypes signature against the header, the size of mrbf_ps_info, and the routing of
`pascoletti_serafini.get_criticality_many` -- every start's status is mapped as `get_criticality_container` maps it, and a shape the
table refuses takes the loop of single calls.  No GPU: the device call is replaced by a stub."""
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


# (n_starts, d, k, n_models, n_nl, n_lin, n_foreign)
C4 = (64, 128, 2, 1, 0, 0, 0)


def _row(**kw):
    names = ("n_starts", "d", "k", "n_models", "n_nl", "n_lin", "n_foreign")
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
    # whatever mrbf_dispatch_ps refuses
    (_row(d=0), False),
    (_row(k=0), False),
    (_row(k=8), True),
    (_row(k=9), False),
    (_row(n_models=0), False),
    (_row(n_models=8, k=8), True),
    (_row(n_models=9), False),
    (_row(n_nl=32), True),
    (_row(n_nl=33), False),
    (_row(n_nl=-1), False),
    (_row(n_lin=256), True),
    (_row(n_lin=257), False),
])
def test_decision_table_row(lib, args, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_ps_batch(*args) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)
    if device:  # the batch never takes what the single call would refuse
        assert lib.mrbf_dispatch_ps(*args[1:]) == _lib.DISPATCH_DEVICE
    if args[0] == 64 and args[1] <= 256:  # inside the batch's own limits the single call's table decides
        assert lib.mrbf_dispatch_ps_batch(*args) == lib.mrbf_dispatch_ps(*args[1:])


def test_return_codes_that_mean_reference(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_PS_BATCH == 14
    assert lib.mrbf_dispatch_after(14, -2) == 1
    for rc in (0, -1, -3, -4, -5, _lib.MRBF_EHIP, _lib.MRBF_ENOMEM):
        assert lib.mrbf_dispatch_after(14, rc) == 0, rc
    assert lib.mrbf_dispatch_after(14, -2) == lib.mrbf_dispatch_after(_lib.ENTRY_PS_STEP, -2)
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_PS_BATCH = 14\b", text)


_CTYPE = {"mrbf_ctx *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "const double *": ctypes.c_void_p,
          "double *": ctypes.c_void_p, "const mrbf_model *const *": "handles", "const mrbf_ps_problem *": "problem",
          "const mrbf_ps_options *": "options", "const uint64_t *": "seeds", "mrbf_ps_info *": "infos", "float *": "float"}


def test_signature_matches_the_header(lib):
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    decl = re.search(r"int32_t mrbf_ps_step_batch\((.*?)\);", text, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    kinds = []
    for p in params:
        m = re.match(r"(.*?)(\w+)$", p)
        kinds.append(_CTYPE[m.group(1).strip()])
    res, args = _lib.SIGNATURES["mrbf_ps_step_batch"]
    assert res is ctypes.c_int32 and len(args) == len(kinds) == 16
    special = {"handles": ctypes.POINTER(ctypes.c_void_p), "problem": ctypes.POINTER(_lib.PsProblem), "options": ctypes.POINTER(_lib.PsOptions),
               "seeds": ctypes.POINTER(ctypes.c_uint64), "infos": ctypes.POINTER(_lib.PsInfo), "float": ctypes.POINTER(ctypes.c_float)}
    for i, (a, kd) in enumerate(zip(args, kinds)):
        assert a is special.get(kd, kd), (i, params[i])
    assert lib.mrbf_ps_step_batch.argtypes == args
    dres, dargs = _lib.SIGNATURES["mrbf_dispatch_ps_batch"]
    assert dres is ctypes.c_int32 and dargs == [ctypes.c_int64] + [ctypes.c_int32] * 6
    ddecl = re.search(r"int32_t mrbf_dispatch_ps_batch\((.*?)\);", text, flags=re.S).group(1)
    assert [" ".join(p.split()).split()[0] for p in ddecl.split(",")] == ["int64_t"] + ["int32_t"] * 6
    # the Julia binding calls the same symbol with as many arguments
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jm = re.search(r"ccall\(\(:mrbf_ps_step_batch, libmrbf\), Int32,\s*\((.*?)\),\s*hctx", jl, flags=re.S)
    assert jm and len([t for t in jm.group(1).split(",") if t.strip()]) == 16
    assert "function hip_ps_criticality_many" in jl


def test_info_size_and_layout():
    """mrbf_ps_info is an existing struct; what is new is that mrbf_ps_step_batch fills an ARRAY of them, so the mirror's size is the
    array's stride: the batch's `infos` argument is a pointer to the mirror, and the Julia binding passes a vector of its own mirror"""
    from morbit.jl_amd import _lib

    assert _lib.SIGNATURES["mrbf_ps_step_batch"][1][14] is ctypes.POINTER(_lib.PsInfo)
    arr = (_lib.PsInfo * 3)()
    assert ctypes.addressof(arr[1]) - ctypes.addressof(arr[0]) == 32 and ctypes.sizeof(arr) == 96
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    assert "infos = Vector{MrbfPsInfo}(undef, ns)" in jl and re.search(r"^struct MrbfPsInfo\b[^\n]*32 bytes", jl, flags=re.M)

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_ps_info;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "double": 8, "float": 4}
    off, names = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for n in rest.split(","):
            size = sizes[ctype]
            off = (off + size - 1) // size * size
            fld = getattr(_lib.PsInfo, n.strip())
            assert (fld.offset, fld.size) == (off, size), n
            names.append(n.strip())
            off += size
    assert (off + 7) // 8 * 8 == 32 == ctypes.sizeof(_lib.PsInfo)      # an array of them is what the batch fills
    assert names == [f for f, _ in _lib.PsInfo._fields_]


class _FakeModel:
    num_outputs = 2
    ctx = None


def test_routing_of_get_criticality_many(lib, monkeypatch):
    from morbit.jl_amd import _lib
    from morbit.jl_amd import pascoletti_serafini as ps

    ns, d, k = 4, 3, 2
    containers = ["container %d" % p for p in range(ns)]

    def fake_plan(sc, objectives_only=False):
        return {"models": [_FakeModel()], "roles": [0, 1], "k": k, "n_con": 0, "n_foreign": 0, "in_order": True}

    rng = np.random.default_rng(1)
    X, X_n, FX = rng.standard_normal((ns, d)), rng.standard_normal((ns, d)), rng.standard_normal((ns, k))
    lbs, ubs = X - 0.5, X + 0.5
    XT, MT, RO = rng.standard_normal((ns, d)), rng.standard_normal((ns, k)), rng.standard_normal((ns, k))
    status = [_lib.PS_OK, _lib.PS_CRITICAL, _lib.PS_FAILURE, _lib.PS_OK]
    calls = {"device": [], "single": []}

    def fake_device(desc_cfg, plans, X_n_, FX_, lb_, ub_, R=None, lin=None, seeds=None, eq_tol=-1.0, out=None):
        calls["device"].append((len(plans), R, list(seeds)))
        infos = [dict(status=status[p], generations=3, evals_ideal=10, evals_ps=20, evals_polish=0, ms_total=1.5, tau=-0.25 * (p + 1))
                 for p in range(ns)]
        return 0, XT.copy(), MT.copy(), RO.copy(), infos, 1.5

    def fake_single(desc_cfg, sc, scal, x, x_n, fx_n, lb_eff, ub_eff, lin=None, seed=0, rng=None, stats=None, eq_tol=1e-8):
        calls["single"].append((sc, seed))
        return "single", sc

    from morbit.jl_amd import surrogates as sg
    monkeypatch.setattr(sg, "container_plan", fake_plan)
    monkeypatch.setattr(ps, "ps_step_batch_device", fake_device)
    monkeypatch.setattr(ps, "get_criticality_container", fake_single)
    cfg = ps.PascolettiSerafiniConfig()
    stats = {}
    res = ps.get_criticality_many(cfg, containers, None, X, X_n, FX, lbs, ubs, seeds=[5, 6, 7, 8], stats=stats)
    assert calls["device"] == [(ns, None, [5, 6, 7, 8])] and calls["single"] == [] and stats["path"] == "batch"
    assert np.array_equal(stats["r"], RO) and stats["ms_total"] == 1.5
    om, (xt, mt, nrm) = res[0]
    assert om == 0.25 and np.array_equal(xt, XT[0]) and np.array_equal(mt, MT[0]) and nrm == np.linalg.norm(X[0] - XT[0], ord=np.inf)
    assert res[1][0] == 0 and np.array_equal(res[1][1], X_n[1]) and np.array_equal(res[1][2], MT[1]) and res[1][3] == 0   # critical: x_n
    assert res[2][0] == 0 and np.array_equal(res[2][1], X[2]) and np.array_equal(res[2][2], MT[2]) and res[2][3] == 0     # failure: x
    assert res[3][0] == 1.0
    # a given direction is passed on, one row per start
    calls["device"].clear()
    cfg_r = ps.PascolettiSerafiniConfig(reference_direction=[1.0, 2.0])
    ps.get_criticality_many(cfg_r, containers, None, X, X_n, FX, lbs, ubs)
    assert np.array_equal(calls["device"][0][1], np.tile([1.0, 2.0], (ns, 1))) and calls["device"][0][2] == [0] * ns
    # a shape the decision table refuses (d = 257), a batch below the rule, containers of different shapes: the loop of single calls
    for min_starts, Xs in ((ps.PS_BATCH_MIN_STARTS, np.zeros((ns, 257))), (ns + 1, X)):
        calls["device"].clear(), calls["single"].clear()
        stats = {}
        monkeypatch.setattr(ps, "PS_BATCH_MIN_STARTS", min_starts)
        res = ps.get_criticality_many(cfg, containers, None, Xs, Xs, FX, Xs, Xs, seeds=[1, 2, 3, 4], stats=stats)
        assert calls["device"] == [] and stats["path"] == "loop" and calls["single"] == list(zip(containers, [1, 2, 3, 4]))
        assert res == [("single", c) for c in containers]
    monkeypatch.setattr(ps, "PS_BATCH_MIN_STARTS", 2)
    shapes = iter([[0, 1], [1, 0], [0, 1], [0, 1]])
    monkeypatch.setattr(sg, "container_plan", lambda sc, objectives_only=False: dict(fake_plan(sc), roles=next(shapes)))
    calls["single"].clear()
    ps.get_criticality_many(cfg, containers, None, X, X_n, FX, lbs, ubs)
    assert calls["device"] == [] and [c for c, _ in calls["single"]] == containers
    assert ps.ps_batch_pays(2) and not ps.ps_batch_pays(1)
