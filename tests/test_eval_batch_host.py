"""CPU tests of the many-start evaluation entry (mrbf_eval_batch): its decision-table rows, the job's struct mirrors against the header,
the host logic of the call (tools/eval_batch_host_check.cpp, a stand-alone program under AddressSanitizer and UBSan), and the routing
of `rbf_model.eval_models_many`, the containers' many-start twins and `manystart.gpu_solve_shard_keep_models` with a recording fake
library: when they make the one call, what they put into the jobs, and that both routes hand back the same results.  No GPU."""
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


@pytest.mark.parametrize("n_jobs, device", [(1, True), (2, True), (64, True), (65535, True), (0, False), (-1, False), (65536, False)])
def test_decision_table_row(lib, n_jobs, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_eval_batch(n_jobs) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)


def test_return_codes_that_mean_loop(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_EVAL_BATCH == 20
    assert lib.mrbf_dispatch_after(20, -2) == 1
    for rc in (0, -1, -3, -4, _lib.MRBF_EHIP, _lib.MRBF_ENOMEM):
        assert lib.mrbf_dispatch_after(20, rc) == 0, rc
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_EVAL_BATCH = 20\b", text)
    # the threshold the bindings consult: a job count from which on the batch is taken (monotone by construction)
    assert lib.mrbf_dispatch_eval_batch_min_jobs() >= 1


def test_job_mirrors_match_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_eval_job;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ptr = "*" in decl
            names = decl.replace("*", " ").split()[-1 if ptr else 1:] if ptr else decl.split(None, 1)[1].split(",")
            ctype = decl.split()[0] if not ptr else "ptr"
            fields += [(n.strip(), 8 if ptr else {"int32_t": 4, "int64_t": 8}[ctype]) for n in names]
    off, layout = 0, []
    for name, size in fields:       # natural alignment
        off = (off + size - 1) // size * size
        layout.append((name, off, size))
        off += size
    total = (off + 7) // 8 * 8
    assert total == 48 == ctypes.sizeof(_lib.EvalJob)
    assert [f[0] for f in _lib.EvalJob._fields_] == [n for n, _, _ in layout]
    for name, o, size in layout:
        fld = getattr(_lib.EvalJob, name)
        assert (fld.offset, fld.size) == (o, size), name
    # the Julia mirror carries the same fields in the same order and sizes
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfEvalJob\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = re.findall(r"(\w+)::(Int32|Int64|Ptr\{\w+\})", jbody)
    assert [(n, 4 if t == "Int32" else 8) for n, t in jfields] == fields


def test_eval_batch_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "eval_batch_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "eval_batch_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "eval_batch_host_check: ok" in res.stdout


# ---- a recording fake: the decision table is the library's own, the device call is a host function of (model, site, output) ---------
def _surface(tag, X, k):
    """what the fake "model" `tag` gives at the rows of X: values (m x k) and per-point k x d column-major Jacobian blocks (m x d x k)"""
    X = np.asarray(X, dtype=np.float64)
    ls = np.arange(1, k + 1, dtype=np.float64)
    vals = tag + np.sin(X).sum(axis=1)[:, None] * ls[None, :]
    jac = np.cos(X)[:, :, None] * ls[None, None, :] + 0.001 * tag
    return vals, jac


class _FakeLib:
    def __init__(self, real, min_jobs):
        self.real, self.min_jobs, self.batch_calls, self.rc = real, min_jobs, [], 0

    def mrbf_dispatch_eval_batch(self, n):
        return self.real.mrbf_dispatch_eval_batch(n)

    def mrbf_dispatch_eval_batch_min_jobs(self):
        return self.min_jobs

    def mrbf_dispatch_after(self, entry, rc):
        return self.real.mrbf_dispatch_after(entry, rc)

    def mrbf_eval_batch(self, h, n, jobs, ms):
        seen = []
        for i in range(n):
            J = jobs[i]
            seen.append((J.model, J.m, J.X is not None, J.vals_out is not None, J.jac_out is not None))
        self.batch_calls.append(seen)
        if self.rc != 0:
            return self.rc
        for i in range(n):
            J = jobs[i]
            if J.m == 0:
                continue
            mod = _FakeModel.registry[J.model]
            X = np.ctypeslib.as_array((ctypes.c_double * (J.m * mod.d)).from_address(J.X)).reshape(J.m, mod.d)
            vals, jac = _surface(mod.tag, X, mod.k)
            if J.vals_out:
                np.ctypeslib.as_array((ctypes.c_double * vals.size).from_address(J.vals_out))[:] = vals.ravel()
            if J.jac_out:
                np.ctypeslib.as_array((ctypes.c_double * jac.size).from_address(J.jac_out))[:] = jac.ravel()
        return 0


class _FakeCtx:
    h = None

    def __init__(self, lib):
        self.lib = lib

    def check(self, rc):
        from morbit.jl_amd import _lib

        if rc != 0:
            raise _lib.MrbfError(rc, "fake")

    def get_option(self, key):
        return 0.0


class _FakeModel:
    registry = {}
    fully_linear = True

    def __init__(self, ctx, tag, d, k):
        self.ctx, self.tag, self.d, self.k, self.num_outputs = ctx, tag, d, k, k
        self.model = ctypes.c_void_p(1000 + len(_FakeModel.registry))
        _FakeModel.registry[self.model.value] = self
        self.single_calls = []
        self.info, self.weights = {"path": 1, "rel_residual": 1e-12, "ms_total": 0.5}, np.full((3, k), float(tag))

    def eval_sites(self, X, want_values=True, want_jac=False, out_vals=None, out_jac=None, info=None):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, self.d)
        self.single_calls.append((X.shape[0], bool(want_values), bool(want_jac)))
        vals, jac = _surface(self.tag, X, self.k)
        if info is not None:
            info["ms_total"] = 0.25
        return (vals if want_values else None), (np.transpose(jac, (0, 2, 1)) if want_jac else None)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and np.array_equal(a, b)


def test_eval_models_many_routing(lib):
    from morbit.jl_amd import _lib, rbf_model as rm

    fake = _FakeLib(lib, min_jobs=4)
    ctx = _FakeCtx(fake)
    rng = np.random.default_rng(0)
    mods = [_FakeModel(ctx, tag, d, k) for tag, d, k in ((1, 3, 2), (2, 5, 1), (3, 3, 17), (4, 2, 3))]
    order = [0, 1, 2, 3, 0]                    # one model twice
    ms = [4, 1, 0, 7, 2]                       # an empty block among them
    Xs = [rng.standard_normal((m, mods[i].d)) for i, m in zip(order, ms)]
    wv, wj = [True, True, True, False, True], [False, True, True, True, True]
    # 3 pairs: below the threshold -> the loop, no device call
    stats = {}
    res = rm.eval_models_many([mods[i] for i in order[:3]], Xs[:3], want_values=True, want_jac=True, stats=stats)
    assert fake.batch_calls == [] and stats["path"] == "loop" and stats["jobs"] == 0 and len(stats["ms_jobs"]) == 3
    assert [m.single_calls for m in mods[:3]] == [[(4, True, True)], [(1, True, True)], [(0, True, True)]]
    # 5 pairs: one call, jobs in order, a NULL pointer for what is not wanted and for the empty block
    for m in mods:
        m.single_calls.clear()
    stats = {}
    res = rm.eval_models_many([mods[i] for i in order], Xs, want_values=wv, want_jac=wj, stats=stats)
    assert len(fake.batch_calls) == 1 and all(m.single_calls == [] for m in mods)
    assert stats["path"] == "batch" and stats["jobs"] == 5 and len(stats["ms_jobs"]) == 5 and stats["single_inside"] == 0
    assert fake.batch_calls[0] == [(mods[i].model.value, m, m > 0, v and m > 0, j and m > 0) for i, m, v, j in zip(order, ms, wv, wj)]
    loop = [mods[i].eval_sites(Xs[p], want_values=wv[p], want_jac=wj[p]) for p, i in enumerate(order)]
    for (V, J), (V0, J0) in zip(res, loop):
        assert _same(V, V0) and _same(J, J0)
    wide = _FakeModel(ctx, 7, 300, 2)      # outside the fused kernels' range: the single call's chain inside the one call
    st = {}
    rm.eval_models_many([wide, mods[0], wide, wide], [np.zeros((2, 300)), Xs[0], np.zeros((0, 300)), np.ones((1, 300))], stats=st)
    assert st["path"] == "batch" and st["jobs"] == 4 and st["single_inside"] == 2
    # min_jobs overrides the table's threshold, in both directions
    fake.batch_calls.clear()
    rm.eval_models_many([mods[0]], Xs[:1], min_jobs=1)
    assert len(fake.batch_calls) == 1
    rm.eval_models_many([mods[i] for i in order], Xs, min_jobs=6)
    assert len(fake.batch_calls) == 1
    # the library refuses the call (-2): the loop, same results; any other code is an error
    fake.rc = -2
    for m in mods:
        m.single_calls.clear()
    stats = {}
    res2 = rm.eval_models_many([mods[i] for i in order], Xs, want_values=wv, want_jac=wj, stats=stats)
    assert stats["path"] == "loop" and sum(len(m.single_calls) for m in mods) == 5
    for (V, J), (V0, J0) in zip(res2, loop):
        assert _same(V, V0) and _same(J, J0)
    fake.rc = -3
    with pytest.raises(_lib.MrbfError):
        rm.eval_models_many([mods[i] for i in order], Xs)
    fake.rc = 0
    # more pairs than the call takes, and models of two contexts: the loop
    fake.batch_calls.clear()
    stats = {}
    other = _FakeModel(_FakeCtx(fake), 9, 3, 2)
    rm.eval_models_many([mods[0]] * 4 + [other], [Xs[0]] * 5, stats=stats)
    assert fake.batch_calls == [] and stats["path"] == "loop"
    assert rm.eval_models_many([], [], stats=stats) == [] and stats["jobs"] == 0


class _Outer:
    """an exact outer function of xi = [t; g] for a CompositeSurrogate"""
    num_outputs = 2

    def __init__(self, n):
        self.n = n

    def eval(self, xi):
        return np.array([np.sum(xi ** 2), xi[0] * xi[-1]])

    def jacobian(self, xi):
        J = np.zeros((2, xi.size))
        J[0] = 2 * xi
        J[1, 0], J[1, -1] = xi[-1], xi[0]
        return J


def _containers(ctx, ns, d):
    from morbit.jl_amd import surrogates as sg

    scs = []
    for p in range(ns):
        a, b, c = _FakeModel(ctx, 10 * p + 1, d, 3), _FakeModel(ctx, 10 * p + 2, d, 2), _FakeModel(ctx, 10 * p + 3, d, 2)
        scs.append(sg.SurrogateContainer(
            objectives=[sg.RefSurrogate(a, [2, 0]), sg.RefSurrogate(b, [1]), sg.CompositeSurrogate(b, _Outer(d), [0, 1]), sg.RefSurrogate(a, [1])],
            nl_ineq_constraints=[sg.RefSurrogate(c, [0, 1])]))
    return scs


def test_container_twins_make_one_call_and_agree_with_the_single_twins(lib):
    from morbit.jl_amd import surrogates as sg

    fake = _FakeLib(lib, min_jobs=2)
    ctx = _FakeCtx(fake)
    ns, d = 5, 4
    rng = np.random.default_rng(1)
    scs = _containers(ctx, ns, d)
    Xs = [rng.standard_normal((1 + p, d)) for p in range(ns)]
    for plural, n_inner in (("objectives", 2), ("nl_ineq_constraints", 1), ("nl_eq_constraints", 0)):
        for jac in (False, True):
            name = "eval_container_%s%s_at_scaled_sites" % (plural, "_jacobian" if jac else "")
            fake.batch_calls.clear()
            stats = {}
            got = getattr(sg, name + "_many")(scs, None, Xs, stats=stats)
            want = [getattr(sg, name)(scs[p], None, Xs[p]) for p in range(ns)]
            assert len(got) == ns
            for g, w in zip(got, want):
                assert g.shape == w.shape and np.array_equal(g, w), name
            if n_inner:   # the distinct inner models of ALL containers in one call
                assert len(fake.batch_calls) == 1 and len(fake.batch_calls[0]) == ns * n_inner and stats["path"] == "batch"
                if jac and plural == "objectives":   # values ride along only where a CompositeSurrogate's chain rule needs them
                    assert sorted(set(j[3] for j in fake.batch_calls[0])) == [False, True]
            else:
                assert fake.batch_calls == []
    # below the threshold the twins take the loop and agree as well
    fake.min_jobs = 1000
    fake.batch_calls.clear()
    got = sg.eval_container_objectives_jacobian_at_scaled_sites_many(scs, None, Xs)
    assert fake.batch_calls == []
    for p in range(ns):
        assert np.array_equal(got[p], sg.eval_container_objectives_jacobian_at_scaled_sites(scs[p], None, Xs[p]))


def test_keep_models_evaluates_through_eval_models_many(lib, monkeypatch):
    from morbit.jl_amd import manystart, rbf_model as rm

    fake = _FakeLib(lib, min_jobs=2)
    ctx = _FakeCtx(fake)
    rng = np.random.default_rng(2)
    mods = [_FakeModel(ctx, 1, 3, 2), None, _FakeModel(ctx, 3, 3, 2), _FakeModel(ctx, 4, 3, 2)]
    problems = [{"id": p, "cfg": None, "sites": None, "values": None, "X": rng.standard_normal((3 + p, 3)), "want_jac": p != 2} for p in range(4)]
    problems[3]["X"] = None

    def fake_update(cfgs, sites, values, deltas, ctx=None, stats=None):
        stats.update(path="batch", status=[0, 2, 0, 0], ms_total=1.0, wide=0, lu=0)
        return mods

    monkeypatch.setattr(rm, "update_models_many", fake_update)
    tables = {}
    for floor, path in ((None, "batch"), (100, "loop")):
        fake.batch_calls.clear()
        stats = {}
        table, kept = manystart.gpu_solve_shard_keep_models(problems, stats=stats, eval_min_jobs=floor)
        assert kept is mods and stats["path"] == "batch" and stats["eval"]["path"] == path
        assert len(fake.batch_calls) == (1 if path == "batch" else 0)
        if path == "batch":
            assert [j[0] for j in fake.batch_calls[0]] == [mods[0].model.value, mods[2].model.value]
            assert [(j[3], j[4]) for j in fake.batch_calls[0]] == [(True, True), (True, False)]
        tables[path] = table
    a, b = tables["batch"], tables["loop"]
    assert a.shape == b.shape == (4, manystart.RECORD_LEN)
    assert np.array_equal(a[:, :7], b[:, :7], equal_nan=True)   # everything but the evaluation's own clock
    assert a[1, 1] == 2.0 and np.isnan(a[1, 2]) and a[3, 5] == 0.0
    assert a[0, 5] == float(np.sum(_surface(1, problems[0]["X"], 2)[0]))
