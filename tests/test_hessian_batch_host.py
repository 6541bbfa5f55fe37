"""CPU tests of the many-start Hessian entry (mrbf_eval_hessian_batch): the host logic of the call (tools/hess_batch_host_check.cpp, a
stand-alone program under AddressSanitizer and UBSan, run as a child process), the struct mirrors (ctypes, Julia) against the header,
the Julia ccall, the refusal that needs no device, the three rows of the decision table, and the routing of get_hessians_many and of
the container functions with a recording fake library.  No GPU."""
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


def test_hess_batch_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "hess_batch_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "hess_batch_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "hess_batch_host_check: ok" in res.stdout


def test_host_header_includes_no_hip():
    text = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "hess_batch_host.hpp")).read()
    assert not re.search(r"#include\s*[<\"](hip|rocblas|common\.hpp)", text)
    assert '#include "hess_host.hpp"' in text


def test_symbols_are_exported_and_declared(lib):
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    for name in ("mrbf_eval_hessian_batch", "mrbf_eval_hessian_batch_limited"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"int32_t %s\(mrbf_ctx \*ctx, int64_t n_jobs, mrbf_hess_job \*jobs, mrbf_hess_batch_info \*info" % name, text)
    for name in ("mrbf_dispatch_hessian_batch", "mrbf_dispatch_hessian_batch_min_jobs"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mrbf_eval_hessian_batch_limited"][1]) == len(_lib.SIGNATURES["mrbf_eval_hessian_batch"][1]) + 1 == 5
    assert _lib.ENTRY_HESSIAN_BATCH == 21 and re.search(r"MRBF_ENTRY_HESSIAN_BATCH = 21\b", text)


def _header_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.rsplit(None, 1) if "*" in decl else decl.split(None, 1)
        for n in names.split(","):
            n = n.strip()
            fields.append((n.lstrip("*"), "pointer" if "*" in decl else ctype))
    return fields


def test_struct_mirrors_match_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    cmap = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "pointer": ctypes.c_void_p}
    jmap = {"float": ("Float32",), "int32_t": ("Int32",), "int64_t": ("Int64",), "pointer": ("Ptr{Cvoid}", "Ptr{Float64}", "Ptr{Int32}")}
    want = {"mrbf_hess_job": [("model", "pointer"), ("m", "int64_t"), ("X", "pointer"), ("rows", "pointer"), ("hess_out", "pointer"),
                              ("n_rows", "int32_t"), ("status", "int32_t"), ("nsplit", "int32_t"), ("reserved", "int32_t")],
            "mrbf_hess_batch_info": [("ms_total", "float"), ("chunks", "int32_t"), ("groups", "int32_t"), ("single_inside", "int32_t")]}
    for cname, ct, jname, size in (("mrbf_hess_job", _lib.HessJob, "MrbfHessJob", 56),
                                   ("mrbf_hess_batch_info", _lib.HessBatchInfo, "MrbfHessBatchInfo", 16)):
        fields = _header_fields(text, cname)
        assert fields == want[cname]
        assert [(n, cmap[t]) for n, t in fields] == list(ct._fields_)
        assert ctypes.sizeof(ct) == size
        # natural alignment: every field at the offset the C struct gives it
        off = 0
        for n, t in fields:
            sz = ctypes.sizeof(cmap[t])
            off = (off + sz - 1) // sz * sz
            assert getattr(ct, n).offset == off, (cname, n)
            off += sz
        jbody = re.search(r"^struct %s\b[^\n]*\n(.*?)^end" % jname, jl, flags=re.S | re.M).group(1)
        jfields = re.findall(r"(\w+)::([\w{}]+)", jbody)
        assert [n for n, _ in jfields] == [n for n, _ in fields]
        for (n, jt), (_, t) in zip(jfields, fields):
            assert jt in jmap[t], (jname, n, jt)
    assert re.search(r"^struct MrbfHessJob\s+# mirrors mrbf_hess_job, 56 bytes", jl, flags=re.M)


def test_julia_call_is_locked_preserved_and_matches_the_header():
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    fn = re.search(r"^function hip_get_hessians_many\(.*?^end", jl, flags=re.S | re.M).group(0)
    assert re.search(r"hip_get_hessians_many\(mods::AbstractVector\{HipRbfModel\}, Xs::AbstractVector\{Matrix\{Float64\}\}, rows = nothing;\s+"
                     r"min_jobs::Union\{Nothing,Int\} = nothing\)", fn)
    call = re.search(r"GC\.@preserve Xs rows0 Hs jobs begin.*?_locked\(ctx\) do hctx\s+ccall\(\(:mrbf_eval_hessian_batch, libmrbf\), Int32, \(([^)]*)\),"
                     r" hctx, nj, jobs, info\)", fn, flags=re.S)
    assert call, fn
    assert [t.strip() for t in call.group(1).split(",")] == ["Ptr{Cvoid}", "Int64", "Ptr{MrbfHessJob}", "Ref{MrbfHessBatchInfo}"]
    assert "_fallback_rc(21, rc) && return loop()" in fn     # the loop of single calls on -2
    assert "Int32(ℓ - 1)" in fn                              # 1-based outputs in Julia, 0-based rows in the library
    assert "_dispatch_hessian_batch(nj) && pays" in fn and "_hessian_batch_pays(nj)" in fn


def test_refusal_that_needs_no_device(lib):
    from morbit.jl_amd import _lib

    jobs = (_lib.HessJob * 2)()
    info = _lib.HessBatchInfo()
    assert lib.mrbf_eval_hessian_batch(None, 2, jobs, ctypes.byref(info)) == -1
    assert lib.mrbf_eval_hessian_batch_limited(None, 2, jobs, None, 1) == -1
    assert lib.mrbf_eval_hessian_batch(None, 0, None, None) == -1


def test_decision_table_rows(lib):
    from morbit.jl_amd import _lib

    for n, want in ((-1, 0), (0, 0), (1, 1), (2, 1), (64, 1), (65535, 1), (65536, 0), (1 << 40, 0)):
        assert lib.mrbf_dispatch_hessian_batch(n) == (_lib.DISPATCH_DEVICE if want else _lib.DISPATCH_REFERENCE), n
    for rc in range(-12, 3):
        assert lib.mrbf_dispatch_after(_lib.ENTRY_HESSIAN_BATCH, rc) == (1 if rc == -2 else 0), rc
    floor = lib.mrbf_dispatch_hessian_batch_min_jobs()
    # a measured job count, or 65536: the bindings keep the loop; the source, DESIGN.md and the profile agree on it
    assert floor == 65536 or 2 <= floor <= 64
    src = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "dispatch.hip")).read()
    assert int(re.search(r"constexpr int64_t HESSIAN_BATCH_MIN_JOBS = (\d+);", src).group(1)) == floor
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"`mrbf_dispatch_hessian_batch_min_jobs\(\)` (is|stays) %d\b" % floor, design)


# ---- routing with a recording fake library -----------------------------------------------------------------------------------------
def _surface(tag, X, rows, d):
    """what the fake "model" `tag` gives: per point and selected output a symmetric d x d block"""
    X = np.asarray(X, dtype=np.float64)
    base = np.cos(X)[:, None, :, None] * np.cos(X)[:, None, None, :]
    return tag + base * (1.0 + np.asarray(rows, dtype=np.float64))[None, :, None, None] + np.zeros((1, 1, d, d))


class _FakeLib:
    """records every call; models are integer handles with dims[handle] = (d, k)"""

    def __init__(self):
        self.calls, self.rc, self.floor, self.dims = [], 0, 4, {}

    def mrbf_dispatch_hessian_batch(self, n):
        return 1 if 1 <= n <= 65535 else 0

    def mrbf_dispatch_hessian_batch_min_jobs(self):
        return self.floor

    def mrbf_dispatch_after(self, entry, rc):
        self.calls.append(("after", entry, rc))
        return 1 if (entry == 21 and rc == -2) else 0

    def _rows(self, h, n_rows, rows):
        addr = rows.value if hasattr(rows, "value") else rows
        return list(range(self.dims[h][1])) if n_rows == 0 else list(np.ctypeslib.as_array((ctypes.c_int32 * n_rows).from_address(addr)))

    def _fill(self, h, m, X, rows_l, out):
        d = self.dims[h][0]
        Xa = np.ctypeslib.as_array((ctypes.c_double * (m * d)).from_address(X)).reshape(m, d)
        H = _surface(h, Xa, rows_l, d)
        np.ctypeslib.as_array((ctypes.c_double * H.size).from_address(out))[:] = H.ravel()

    def mrbf_eval_hessian(self, h, model, m, X, n_rows, rows, out, info):
        rows_l = self._rows(model.value, n_rows, rows)
        self.calls.append(("single", model.value, m, n_rows, rows_l))
        self._fill(model.value, m, X.value, rows_l, out.value)
        info._obj.nsplit, info._obj.chunks = 3, 1
        return 0

    def _batch(self, n, jobs, info, limit):
        rec = []
        for i in range(n):
            J = jobs[i]
            rec.append((J.model, J.m, J.n_rows, None if not J.rows else self._rows(J.model, J.n_rows, J.rows), bool(J.X), bool(J.hess_out)))
        self.calls.append(("batch", n, rec, limit))
        if self.rc != 0:
            return self.rc
        for i in range(n):
            J = jobs[i]
            J.status = 0
            if J.m > 0:
                self._fill(J.model, J.m, J.X, self._rows(J.model, J.n_rows, J.rows), J.hess_out)
                J.nsplit = 2
        info._obj.chunks, info._obj.groups, info._obj.single_inside, info._obj.ms_total = 1, 2, 0, 0.5
        return 0

    def mrbf_eval_hessian_batch(self, h, n, jobs, info):
        return self._batch(n, jobs, info, None)

    def mrbf_eval_hessian_batch_limited(self, h, n, jobs, info, limit):
        return self._batch(n, jobs, info, limit)

    def mrbf_free_model(self, h, model):
        return 0


class _FakeCtx:
    h = None

    def __init__(self, lib):
        self.lib = lib

    def check(self, rc):
        from morbit.jl_amd import _lib

        if rc != 0:
            raise _lib.MrbfError(rc, "fake")


def _fake_models(fake, ctx, shapes):
    from morbit.jl_amd import rbf_model as rm

    mods = []
    for i, (d, k) in enumerate(shapes):
        fake.dims[10 + i] = (d, k)
        mods.append(rm.RbfModel(ctx, ctypes.c_void_p(10 + i), 10, d, k, 0))
    return mods


def test_get_hessians_many_routes_by_the_table_and_the_threshold():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, rbf_model as rm

    assert pkg.get_hessians_many is rm.get_hessians_many
    fake = _FakeLib()
    ctx = _FakeCtx(fake)
    mods = _fake_models(fake, ctx, [(4, 3), (2, 5), (4, 3), (3, 1), (4, 3)])
    rng = np.random.default_rng(1)
    Xs = [rng.standard_normal((m, mod.d)) for m, mod in zip((2, 1, 3, 0, 2), mods)]
    want = [_surface(10 + i, Xs[i], range(mod.k), mod.d) for i, mod in enumerate(mods)]
    # at the threshold: ONE batch call with the job fields of every pair; all outputs -> NULL rows with n_rows = 0; m = 0 -> NULL buffers
    stats = {}
    H = rm.get_hessians_many(mods, Xs, stats=stats)
    assert [c[0] for c in fake.calls] == ["batch"]
    _, n, rec, limit = fake.calls[0]
    assert n == 5 and limit is None
    assert rec == [(10, 2, 0, None, True, True), (11, 1, 0, None, True, True), (12, 3, 0, None, True, True), (13, 0, 0, None, False, False),
                   (14, 2, 0, None, True, True)]
    assert stats == {"path": "batch", "jobs": 5, "single_inside": 0, "chunks": 1, "groups": 2, "ms_total": 0.5, "nsplit": [2, 2, 2, 0, 2]}
    assert all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(H, want)) and H[3].shape == (0, 1, 3, 3)
    # below the threshold: the loop of single calls, no batch call
    fake.calls.clear()
    stats = {}
    H = rm.get_hessians_many(mods[:3], Xs[:3], stats=stats)
    assert [c[0] for c in fake.calls] == ["single"] * 3 and stats["path"] == "loop" and stats["jobs"] == 0 and stats["nsplit"] == [3, 3, 3]
    assert all(np.array_equal(a, b) for a, b in zip(H, want[:3]))
    # min_jobs overrides the table's threshold both ways
    fake.calls.clear()
    rm.get_hessians_many(mods[:3], Xs[:3], min_jobs=3, stats=stats)
    assert [c[0] for c in fake.calls] == ["batch"] and stats["path"] == "batch"
    fake.calls.clear()
    rm.get_hessians_many(mods, Xs, min_jobs=6, stats=stats)
    assert "batch" not in [c[0] for c in fake.calls] and stats["path"] == "loop"
    # rows: one list for all pairs (int32, in order, repeats kept) or one entry per pair; an empty selection is not "all"
    fake.calls.clear()
    three = [mods[0], mods[2], mods[4]]
    X3 = [Xs[0], Xs[2], Xs[4]]
    H = rm.get_hessians_many(three, X3, rows=[2, 0, 2], min_jobs=1, limit_bytes=4096)
    _, n, rec, limit = fake.calls[0]
    assert limit == 4096 and [r[2:4] for r in rec] == [(3, [2, 0, 2])] * 3
    assert all(np.array_equal(h, _surface(t, x, [2, 0, 2], 4)) for h, t, x in zip(H, (10, 12, 14), X3))
    fake.calls.clear()
    H = rm.get_hessians_many(three, X3, rows=[[1], None, []], min_jobs=1)
    _, n, rec, limit = fake.calls[0]
    assert rec == [(10, 2, 1, [1], True, True), (12, 3, 0, None, True, True), (14, 0, 0, None, False, False)]
    assert H[0].shape == (2, 1, 4, 4) and H[1].shape == (3, 3, 4, 4) and H[2].shape == (2, 0, 4, 4)
    loop = rm.get_hessians_many(three, X3, rows=[[1], None, []], min_jobs=9)
    assert all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(H, loop))
    # outs are used in place
    outs = [np.full((2, 3, 4, 4), np.nan), None, np.full((2, 3, 4, 4), np.nan)]
    H = rm.get_hessians_many(three, X3, outs=outs, min_jobs=1)
    assert H[0] is outs[0] and H[2] is outs[2] and np.array_equal(outs[0], want[0]) and np.array_equal(outs[2], want[4])
    # -2 from the call: the table is asked (entry 21), then the loop runs
    fake.calls.clear()
    fake.rc = -2
    stats = {}
    H = rm.get_hessians_many(mods, Xs, stats=stats)
    kinds = [c[0] for c in fake.calls]
    assert kinds[:2] == ["batch", "after"] and fake.calls[1] == ("after", 21, -2) and kinds[2:] == ["single"] * 5 and stats["path"] == "loop"
    assert all(np.array_equal(a, b) for a, b in zip(H, want))
    # any other code is an error
    fake.rc = -3
    with pytest.raises(_lib.MrbfError):
        rm.get_hessians_many(mods, Xs)
    # a job count the table refuses, models of two contexts, no pairs: the loop
    fake.rc = 0
    fake.calls.clear()
    other = _fake_models(fake, _FakeCtx(fake), [(4, 3)])
    fake.dims[10] = (4, 3)
    rm.get_hessians_many([mods[0]] * 3 + other, [Xs[0]] * 4, min_jobs=1, stats=stats)
    assert "batch" not in [c[0] for c in fake.calls] and stats["path"] == "loop"
    assert rm.get_hessians_many([], [], stats=stats) == [] and stats["path"] == "loop" and stats["nsplit"] == []
    for mod in mods + other:
        mod.model = None


def test_container_functions_route_through_one_batch():
    from morbit.jl_amd import surrogates as sg

    fake = _FakeLib()
    ctx = _FakeCtx(fake)
    d = 3
    starts, Xs = [], []
    rng = np.random.default_rng(2)
    all_mods = []
    for p in range(5):
        fake_mods = _fake_models(fake, ctx, [])
        a_h, b_h = 100 + 2 * p, 101 + 2 * p
        fake.dims[a_h], fake.dims[b_h] = (d, 4), (d, 2)
        from morbit.jl_amd import rbf_model as rm

        A = rm.RbfModel(ctx, ctypes.c_void_p(a_h), 10, d, 4, 0)
        B = rm.RbfModel(ctx, ctypes.c_void_p(b_h), 10, d, 2, 0)
        all_mods += [A, B] + fake_mods
        sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(A, [3, 0]), sg.RefSurrogate(B, [1]), sg.RefSurrogate(A, [0])],
                                   nl_ineq_constraints=[sg.RefSurrogate(B, [0, 1])])
        starts.append((sc, A, B))
        Xs.append(rng.standard_normal((2, d)))
    scs = [s[0] for s in starts]
    # single container: one hessian_sites call per distinct inner model with the union of the rows, ascending, each once
    sc, A, B = starts[0]
    H = sg.eval_container_objectives_hessians_at_scaled_sites(sc, None, Xs[0])
    assert [c[:4] for c in fake.calls] == [("single", 100, 2, 2), ("single", 101, 2, 1)]
    assert fake.calls[0][4] == [0, 3] and fake.calls[1][4] == [1]
    SA, SB = _surface(100, Xs[0], range(4), d), _surface(101, Xs[0], range(2), d)
    assert H.shape == (2, 4, d, d) and np.array_equal(H, np.stack([SA[:, 3], SA[:, 0], SB[:, 1], SA[:, 0]], axis=1))
    H1 = sg.eval_container_objectives_hessians_at_scaled_site(sc, None, Xs[0][1])
    assert np.array_equal(H1, H[1])
    Hc = sg.eval_container_nl_ineq_constraints_hessians_at_scaled_sites(sc, None, Xs[0])
    assert np.array_equal(Hc, SB[:, [0, 1]])
    # an empty list: 0 x d x d at a site, m x 0 x d x d at sites, nothing asked of the library
    n_calls = len(fake.calls)
    assert sg.eval_container_nl_eq_constraints_hessians_at_scaled_site(sc, None, Xs[0][0]).shape == (0, d, d)
    assert sg.eval_container_nl_eq_constraints_hessians_at_scaled_sites(sc, None, Xs[0]).shape == (2, 0, d, d)
    assert len(fake.calls) == n_calls
    # many-start: all distinct inner models of all containers in ONE batch call (10 jobs >= the threshold of 4)
    fake.calls.clear()
    stats = {}
    many = sg.eval_container_objectives_hessians_at_scaled_sites_many(scs, None, Xs, stats=stats)
    assert [c[0] for c in fake.calls] == ["batch"] and stats["path"] == "batch" and stats["jobs"] == 10
    rec = fake.calls[0][2]
    assert [r[0] for r in rec] == list(range(100, 110)) and [r[3] for r in rec] == [[0, 3], [1]] * 5
    for p, (scp, _, _) in enumerate(starts):
        assert np.array_equal(many[p], scp._hess_at_sites("objective", None, Xs[p]))
    # below the threshold: the loop, same results
    fake.calls.clear()
    loop = sg.eval_container_objectives_hessians_at_scaled_sites_many(scs, None, Xs, stats=stats, min_jobs=11)
    assert "batch" not in [c[0] for c in fake.calls] and stats["path"] == "loop"
    assert all(np.array_equal(a, b) for a, b in zip(many, loop))
    assert [h.shape for h in sg.eval_container_nl_eq_constraints_hessians_at_scaled_sites_many(scs, None, Xs)] == [(2, 0, d, d)] * 5
    # a CompositeSurrogate is refused as get_hessian refuses it, before anything is asked of the library
    fake.calls.clear()
    bad = sg.SurrogateContainer(objectives=[sg.RefSurrogate(A, [1]), sg.CompositeSurrogate(B, None, [0, 1], num_outputs=1)])
    with pytest.raises(NotImplementedError) as e1:
        sg.eval_container_objectives_hessians_at_scaled_sites(bad, None, Xs[0])
    with pytest.raises(NotImplementedError):
        sg.eval_container_objectives_hessians_at_scaled_sites_many([scs[0], bad], None, Xs[:2])
    with pytest.raises(NotImplementedError) as e2:
        sg.get_hessian(bad.lists["objective"][1], None, Xs[0][0], 0)
    assert str(e1.value) == str(e2.value) and not fake.calls
    for mod in all_mods:
        mod.model = None
