"""CPU tests of the model-Hessian entry (mrbf_eval_hessian): the host logic of the call (tools/hess_host_check.cpp, a stand-alone
program under AddressSanitizer and UBSan, run as a child process), the struct mirrors (ctypes, Julia) against the header, the Julia
ccall, the refusals that need no device, and the routing of the three Python layers with a recording fake library.  No GPU."""
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


def test_hess_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "hess_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "hess_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "hess_host_check: ok" in res.stdout


def test_host_header_includes_no_hip():
    text = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "hess_host.hpp")).read()
    assert not re.search(r"#include\s*[<\"](hip|rocblas|common\.hpp)", text)


def test_symbols_are_exported_and_declared(lib):
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    for name in ("mrbf_eval_hessian", "mrbf_eval_hessian_limited"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"int32_t %s\(mrbf_ctx \*ctx, const mrbf_model \*model, int64_t m, const double \*X," % name, text)
    assert len(_lib.SIGNATURES["mrbf_eval_hessian_limited"][1]) == len(_lib.SIGNATURES["mrbf_eval_hessian"][1]) + 1 == 9


def test_info_mirrors_match_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_hess_info;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("ms_total", "float"), ("nsplit", "int32_t"), ("chunks", "int32_t"), ("reserved", "int32_t")]
    cmap = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    assert [(n, cmap[t]) for n, t in fields] == list(_lib.HessInfo._fields_)
    assert ctypes.sizeof(_lib.HessInfo) == 16
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfHessInfo\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jmap = {"float": "Float32", "int32_t": "Int32"}
    assert re.findall(r"(\w+)::(\w+)", jbody) == [(n, jmap[t]) for n, t in fields]


def test_julia_call_is_locked_preserved_and_matches_the_header():
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    fn = re.search(r"^function hip_get_hessians_at_sites\(.*?^end", jl, flags=re.S | re.M).group(0)
    call = re.search(r"GC\.@preserve X rows0 H begin\s+_locked\(mod\.ctx\) do hctx\s+ccall\(\(:mrbf_eval_hessian, libmrbf\), Int32,\s+\(([^)]*)\),", fn)
    assert call, fn
    assert [t.strip() for t in call.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{Cvoid}", "Int64", "Ptr{Float64}", "Int32", "Ptr{Int32}", "Ptr{Float64}",
                                                             "Ref{MrbfHessInfo}"]
    assert "Int32(ℓ - 1)" in fn                       # 1-based outputs in Julia, 0-based rows in the library
    assert re.search(r"^hip_get_hessian\(mod::HipRbfModel, scal, x̂::Vec, ℓ::Integer\) =", jl, flags=re.M)


def test_refusals_that_need_no_device(lib):
    out = np.full(4, np.nan)
    X = np.zeros(2)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.mrbf_eval_hessian(None, None, 1, P(X), 0, None, P(out), None) == -1
    assert lib.mrbf_eval_hessian_limited(None, None, 1, P(X), 0, None, P(out), None, 1) == -1
    assert np.isnan(out).all()


# ---- routing with a recording fake library -----------------------------------------------------------------------------------------
def _surface(tag, X, rows, d):
    """what the fake "model" `tag` gives: per point and selected output a symmetric d x d block"""
    X = np.asarray(X, dtype=np.float64)
    base = np.cos(X)[:, None, :, None] * np.cos(X)[:, None, None, :]
    return tag + base * (1.0 + np.asarray(rows, dtype=np.float64))[None, :, None, None] + np.zeros((1, 1, d, d))


class _FakeLib:
    def __init__(self, k):
        self.k, self.calls, self.rc = k, [], 0

    def _run(self, h, model, m, X, n_rows, rows, out, info, limit):
        d = _FakeLib.dims[model.value]
        rows_l = list(range(self.k)) if n_rows == 0 else list(np.ctypeslib.as_array((ctypes.c_int32 * n_rows).from_address(rows.value)))
        self.calls.append((model.value, m, n_rows, None if rows is None else rows_l, limit))
        if self.rc != 0:
            return self.rc
        Xa = np.ctypeslib.as_array((ctypes.c_double * (m * d)).from_address(X.value)).reshape(m, d)
        H = _surface(model.value, Xa, rows_l, d)
        np.ctypeslib.as_array((ctypes.c_double * H.size).from_address(out.value))[:] = H.ravel()
        info._obj.nsplit, info._obj.chunks = 3, 1
        return 0

    def mrbf_eval_hessian(self, h, model, m, X, n_rows, rows, out, info):
        return self._run(h, model, m, X, n_rows, rows, out, info, None)

    def mrbf_eval_hessian_limited(self, h, model, m, X, n_rows, rows, out, info, limit):
        return self._run(h, model, m, X, n_rows, rows, out, info, limit)

    def mrbf_free_model(self, h, model):
        return 0

    dims = {}


class _FakeCtx:
    h = None

    def __init__(self, lib):
        self.lib = lib

    def check(self, rc):
        from morbit.jl_amd import _lib

        if rc != 0:
            raise _lib.MrbfError(rc, "fake")


def test_python_layers_route_to_the_one_call():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, rbf_model as rm, surrogates as sg

    d, k = 4, 3
    fake = _FakeLib(k)
    handle = ctypes.c_void_p(5)
    _FakeLib.dims[5] = d
    mod = rm.RbfModel(_FakeCtx(fake), handle, 10, d, k, 0)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((6, d))
    # RbfModel.hessian_sites: all outputs -> NULL rows with n_rows = 0; a row list goes through as int32, in order, repeats kept
    info = {}
    H = mod.hessian_sites(X, info=info)
    assert fake.calls[-1] == (5, 6, 0, None, None) and H.shape == (6, k, d, d) and info["nsplit"] == 3 and info["chunks"] == 1
    assert np.array_equal(H, _surface(5, X, [0, 1, 2], d))
    Hr = mod.hessian_sites(X, rows=[2, 0, 2])
    assert fake.calls[-1] == (5, 6, 3, [2, 0, 2], None) and np.array_equal(Hr, H[:, [2, 0, 2]])
    out = np.full((6, 1, d, d), np.nan)
    assert mod.hessian_sites(X, rows=[1], out=out) is out and np.array_equal(out[:, 0], H[:, 1])
    mod.hessian_sites(X, stage_bytes=4096)
    assert fake.calls[-1] == (5, 6, 0, None, 4096)               # the limited twin, only when a limit is given
    n_calls = len(fake.calls)
    assert mod.hessian_sites(X, rows=[]).shape == (6, 0, d, d) and len(fake.calls) == n_calls   # an empty selection is not "all"
    # rbf_model / package level
    assert np.array_equal(rm.get_hessian(mod, None, X[2], 1), H[2, 1]) and fake.calls[-1] == (5, 1, 1, [1], None)
    assert np.array_equal(pkg.get_hessians_at_sites(mod, None, X, rows=[1, 1]), H[:, [1, 1]])
    assert np.array_equal(rm.get_hessians_at_sites(mod, None, X), H) and fake.calls[-1] == (5, 6, 0, None, None)
    # surrogates: the model itself, a RefSurrogate (selects the row of the grouped model), a CompositeSurrogate (refused, no call)
    assert np.array_equal(sg.get_hessian(mod, None, X[0], 2), H[0, 2])
    ref = sg.RefSurrogate(mod, [2, 0])
    assert np.array_equal(sg.get_hessian(ref, None, X[3], 0), H[3, 2]) and fake.calls[-1] == (5, 1, 1, [2], None)
    assert np.array_equal(sg.get_hessian(ref, None, X[3], 1), H[3, 0]) and fake.calls[-1] == (5, 1, 1, [0], None)
    n_calls = len(fake.calls)
    with pytest.raises(NotImplementedError):
        sg.get_hessian(sg.CompositeSurrogate(mod, None, [0, 1], num_outputs=1), None, X[0], 0)
    assert len(fake.calls) == n_calls
    # an error code of the library is raised
    fake.rc = -6
    with pytest.raises(_lib.MrbfError):
        mod.hessian_sites(X, rows=[7])
    mod.model = None
