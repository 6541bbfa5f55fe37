"""CPU tests of the many-start model update (mrbf_fit_batch): the job's struct mirror against the header and the Julia file, its
decision-table row, the return codes that mean "take the loop", the routing of `rbf_model.update_models_many`, and the no-device
error.  No GPU: the device call is replaced by a stub."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT, has_gpu


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


def test_job_mirror_matches_the_header():
    from morbit.jl_amd import _lib

    assert ctypes.sizeof(_lib.FitJob) == 168 and _lib.FitJob.info.offset == 88
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_fit_job;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "double": 8, "int64_t": 8, "mrbf_fit_info": ctypes.sizeof(_lib.FitInfo)}
    fields = []
    for decl in body.split(";"):
        decl = re.sub(r"\bconst\b", " ", decl).strip()
        if decl:
            ctype, names = decl.split(None, 1)
            for n in names.split(","):
                n = n.strip()
                fields.append((n.lstrip("*"), 8 if n.startswith("*") or ctype == "mrbf_model" else sizes[ctype]))
    off, layout = 0, []
    for name, size in fields:       # natural alignment (mrbf_fit_info holds doubles: 8)
        al = min(size, 8)
        off = (off + al - 1) // al * al
        layout.append((name, off, size))
        off += size
    assert (off + 7) // 8 * 8 == 168
    assert [f[0] for f in _lib.FitJob._fields_] == [n for n, _, _ in layout]
    for name, o, size in layout:
        fld = getattr(_lib.FitJob, name)
        assert (fld.offset, fld.size) == (o, size), name
    # the Julia mirror carries the same fields in the same order
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfFitJob\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jsizes = {"Int32": 4, "Int64": 8, "Float64": 8, "Ptr{Float64}": 8, "Ptr{Cvoid}": 8, "MrbfFitInfo": ctypes.sizeof(_lib.FitInfo)}
    jfields = [(n, jsizes[t]) for n, t in re.findall(r"(\w+)::([\w{}]+)", "\n".join(ln.split("#")[0] for ln in jbody.split("\n")))]
    assert jfields == fields
    assert re.search(r"_locked\(ctx\) do hctx\s+ccall\(\(:mrbf_fit_batch, libmrbf\)", jl)


def test_decision_table_row(lib):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_fit_batch(0) == _lib.DISPATCH_REFERENCE and lib.mrbf_dispatch_fit_batch(65536) == _lib.DISPATCH_REFERENCE
    assert lib.mrbf_dispatch_fit_batch(1) == _lib.DISPATCH_DEVICE and lib.mrbf_dispatch_fit_batch(65535) == _lib.DISPATCH_DEVICE
    assert lib.mrbf_dispatch_fit_batch(-1) == _lib.DISPATCH_REFERENCE


def test_return_codes_that_mean_the_loop(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_FIT_BATCH == 11
    assert lib.mrbf_dispatch_after(_lib.ENTRY_FIT_BATCH, -2) == 1
    assert lib.mrbf_dispatch_after(_lib.ENTRY_FIT_BATCH, _lib.MRBF_EHIP) == 0 and lib.mrbf_dispatch_after(_lib.ENTRY_FIT_BATCH, 0) == 0
    assert re.search(r"MRBF_ENTRY_FIT_BATCH = 11\b", open(os.path.join(ROOT, "include", "mrbf.h")).read())


class _StubLib:
    """the real decision table around a stubbed device call"""

    def __init__(self, lib, rc, dispatch_as=None):
        self.real, self.rc, self.dispatch_as, self.calls = lib, rc, dispatch_as, []

    def mrbf_dispatch_fit_batch(self, ns):
        return self.real.mrbf_dispatch_fit_batch(ns if self.dispatch_as is None else self.dispatch_as)

    def mrbf_dispatch_after(self, entry, rc):
        return self.real.mrbf_dispatch_after(entry, rc)

    def mrbf_last_error(self, h):
        return b"stub"

    def mrbf_fit_batch(self, h, ns, jobs, ms):
        self.calls.append(ns)
        for p in range(ns):
            jobs[p].status = 0 if p != 1 else 2
            jobs[p].model = 1000 + p
            jobs[p].info.path = 2
        return self.rc


class _StubCtx:
    def __init__(self, lib):
        self.lib, self.h = lib, None

    def check(self, rc):
        from morbit.jl_amd import _lib

        if rc != 0:
            raise _lib.MrbfError(rc, "stub")


def test_update_models_many_routing(lib, monkeypatch):
    from morbit.jl_amd import _lib, rbf_model as rm

    ns, n, d, k = 3, 9, 2, 2
    rng = np.random.default_rng(0)
    sites = [rng.standard_normal((n, d)) for _ in range(ns)]
    vals = [rng.standard_normal((n, k)) for _ in range(ns)]
    cfg = rm.RbfConfig()
    looped = []

    def fake_update(cfg_, C, Y, delta=1.0, fully_linear=False, ctx=None):
        looped.append((C, delta))
        if len(looped) % ns == 2:
            raise _lib.MrbfError(2, "stub")
        return rm.RbfModel(ctx, None, n, d, k, d + 1, fully_linear, None, None, {"ms_total": 0.5})

    monkeypatch.setattr(rm, "update_model", fake_update)
    # the table refuses (as it does 65536 starts): the loop, the device entry is not called
    stub = _StubLib(lib, 0, dispatch_as=65536)
    stats = {}
    mods = rm.update_models_many(cfg, sites, vals, [0.5, 0.6, 0.7], ctx=_StubCtx(stub), stats=stats)
    assert stub.calls == [] and stats["path"] == "loop" and stats["status"] == [0, 2, 0]
    assert [m is None for m in mods] == [False, True, False] and [lp[1] for lp in looped] == [0.5, 0.6, 0.7]
    assert all(lp[0] is s for lp, s in zip(looped, sites))
    # the library refuses (-2): the loop after one device call
    looped.clear()
    stub = _StubLib(lib, -2)
    stats = {}
    mods = rm.update_models_many(cfg, sites, vals, 1.0, ctx=_StubCtx(stub), stats=stats)
    assert stub.calls == [ns] and stats["path"] == "loop" and len(looped) == ns and len(mods) == ns
    # the call goes through: no loop, a failed start is None with its status
    looped.clear()
    stub = _StubLib(lib, 0)
    stats = {}
    mods = rm.update_models_many(cfg, sites, vals, 1.0, fully_linear=[True, False, True], ctx=_StubCtx(stub), stats=stats)
    assert stub.calls == [ns] and looped == [] and stats["path"] == "batch" and stats["status"] == [0, 2, 0]
    assert mods[1] is None and mods[0].model.value == 1000 and mods[2].model.value == 1002
    assert (mods[0].n, mods[0].d, mods[0].k, mods[0].q, mods[0].fully_linear, mods[2].fully_linear) == (n, d, k, d + 1, True, True)
    assert mods[0].info["path"] == 2
    for m in mods:
        if m is not None:
            m.model = None          # (stub handles: nothing to release)
    # any other return code is an error, not a reason to loop
    stub = _StubLib(lib, _lib.MRBF_EHIP)
    with pytest.raises(_lib.MrbfError):
        rm.update_models_many(cfg, sites, vals, 1.0, ctx=_StubCtx(stub))
    assert looped == []


def test_no_device_no_fit(lib):
    from morbit.jl_amd import _lib

    jobs = (_lib.FitJob * 1)()
    assert lib.mrbf_fit_batch(None, 1, jobs, None) == -1
    if has_gpu():
        return
    import morbit.jl_amd as pkg

    with pytest.raises(pkg.MrbfError) as ei:
        pkg.update_models_many(pkg.RbfConfig(), [np.zeros((4, 2))], [np.zeros((4, 1))], 1.0)
    assert ei.value.code == _lib.MRBF_ENODEVICE
