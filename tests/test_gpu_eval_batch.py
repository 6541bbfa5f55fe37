"""The many-start evaluation on the device (run with -m gpu): mrbf_eval_batch against the loop of mrbf_eval.  Bit identity is the
contract -- np.array_equal throughout, on buffers that start as NaN, so that an entry the call did not write shows as well.  Shapes are
the smallest at which each launch path differs: d = 3 / 65 / 130 for dpad 64 / 128 / 256 and d = 300 outside the fused range (the single
call's chain inside the call); n = 20 (one centre tile, never split), 257 (five tiles: split for a small query batch), 600 (ten tiles:
the cost rule); m = 0, 1, 63, 64, 65 around the 64-query tile; k = 1, 2, 3, 17 (one and two outputs per pass, an odd remainder, more
than 16).  Models come from mrbf_model_from_coeffs with random coefficients wherever the fit is not what is tested: identity of the
evaluation does not need an interpolant."""
import ctypes
import zlib

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, manystart
    from morbit.jl_amd import rbf_model as rm
    from morbit.jl_amd import surrogates as sg

# name -> (kernel, shape parameter, polynomial degree); the last two take the difference form
KERNELS = {"cubic3": ("cubic", 3.0, 1), "mq": ("multiquadric", float("nan"), 0), "gauss": ("gaussian", float("nan"), -1),
           "cubic1": ("cubic", 1.0, 1), "tps1": ("thin_plate_spline", 1.0, 1)}
MS = (0, 1, 63, 64, 65)
KS = (1, 2, 3, 17)
SELECT = ((True, False), (False, True), (True, True))   # values only, Jacobians only, both


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


_ZOO = {}


def model(ctx, kern, n, d, k):
    """a resident model with random coefficients (one per key for the whole module)"""
    key = (id(ctx), kern, n, d, k)
    if key not in _ZOO:
        kernel, sp, deg = KERNELS[kern]
        rng = np.random.default_rng(zlib.crc32(repr((kern, n, d, k)).encode()))
        q = 0 if deg < 0 else (1 if deg == 0 else d + 1)
        cfg = pkg.RbfConfig(kernel=kernel, shape_parameter=sp, polynomial_degree=deg)
        _ZOO[key] = rm.model_from_coeffs(cfg, rng.uniform(-2.0, 2.0, (n, d)), rng.standard_normal((n, k)) / n,
                                         rng.standard_normal((q, k)) if q else None, ctx=ctx)
    return _ZOO[key]


def queries(m, d, seed=0):
    return np.random.default_rng(1000 * m + d + seed).uniform(-2.0, 2.0, (m, d))


def job(mod, m, vals=True, jac=True, seed=0):
    return dict(mod=mod, X=queries(m, mod.d, seed), vals=vals, jac=jac)


def _buffers(spec):
    mod, m = spec["mod"], spec["X"].shape[0]
    return (np.full((m, mod.k), np.nan) if spec["vals"] else None), (np.full((m, mod.d, mod.k), np.nan) if spec["jac"] else None)


def loop(ctx, specs):
    """the reference: one mrbf_eval per job on host arrays"""
    res = []
    for s in specs:
        V, J = _buffers(s)
        if V is not None or J is not None:    # (a job without outputs does nothing)
            rc = ctx.lib.mrbf_eval(ctx.h, s["mod"].model, s["X"].shape[0], _lib.as_ptr(s["X"]), _lib.as_ptr(V), _lib.as_ptr(J), None)
            assert rc == 0, (rc, ctx.lib.mrbf_last_error(ctx.h))
        res.append((V, J))
    return res


def batch(ctx, specs, limit=None, expect_rc=0):
    """one mrbf_eval_batch call on host arrays"""
    n = len(specs)
    jobs = (_lib.EvalJob * max(n, 1))()
    outs = []
    for i, s in enumerate(specs):
        V, J = _buffers(s)
        outs.append((V, J))
        jobs[i].model, jobs[i].m = s["mod"].model.value, s["X"].shape[0]
        jobs[i].X = s["X"].ctypes.data if s["X"].size else None
        jobs[i].vals_out, jobs[i].jac_out = (a.ctypes.data if a is not None else None for a in (V, J))
        jobs[i].status = 77
    ms = ctypes.c_float(-1.0)
    if limit is None:
        rc = ctx.lib.mrbf_eval_batch(ctx.h, n, jobs, ctypes.byref(ms))
    else:
        rc = ctx.lib.mrbf_eval_batch_limited(ctx.h, n, jobs, ctypes.byref(ms), limit)
    assert rc == expect_rc, (rc, ctx.lib.mrbf_last_error(ctx.h))
    if rc == 0:
        assert all(jobs[i].status == 0 for i in range(n)) and ms.value >= 0.0
    return outs


def same(got, ref, tag=""):
    assert len(got) == len(ref)
    for i, ((V, J), (V0, J0)) in enumerate(zip(got, ref)):
        for a, b in ((V, V0), (J, J0)):
            assert (a is None) == (b is None), (tag, i)
            if a is not None:
                assert not np.isnan(b).any(), (tag, i)
                assert np.array_equal(a, b), (tag, i, float(np.abs(a - b).max()))


# ---- dimension x centre tiles, with every query count, output count and output selection in the call ------------------------------
@pytest.mark.parametrize("n", [20, 257, 600])
@pytest.mark.parametrize("d", [3, 65, 130, 300])
def test_dimension_and_centre_tiles(ctx, d, n):
    specs = []
    for ik, k in enumerate(KS):
        mod = model(ctx, "cubic3", n, d, k)
        for im, m in enumerate(MS):
            v, j = SELECT[(ik + im) % 3]
            specs.append(job(mod, m, v, j))
    same(batch(ctx, specs), loop(ctx, specs), (d, n))


@pytest.mark.parametrize("kern", sorted(KERNELS))
def test_kernels(ctx, kern):
    specs = []
    for d in (3, 65, 300):
        for n in (20, 257):
            mod = model(ctx, kern, n, d, 2)
            specs += [job(mod, m, v, j) for m in (1, 65) for v, j in SELECT]
    same(batch(ctx, specs), loop(ctx, specs), kern)


def test_the_same_model_split_and_unsplit_in_one_call(ctx):
    # eval_nsplit: a model of 4 .. 8 centre tiles is split while the query tiles fill at most an eighth of the 2 * ncu workgroup slots
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    m_unsplit = 64 * (slots // 8 + 1)          # the first query count whose tiles exceed that eighth (4160 on 256 compute units)
    for d in (65, 3):
        mod = model(ctx, "cubic3", 257, d, 2)
        specs = [job(mod, m_unsplit), job(mod, 1), job(mod, m_unsplit - 64, True, False), job(mod, m_unsplit, True, False)]
        same(batch(ctx, specs), loop(ctx, specs), d)


def test_values_do_not_depend_on_the_output_selection(ctx):
    specs = []
    for kern, n, d, k in (("cubic3", 257, 65, 2), ("mq", 600, 130, 3), ("tps1", 257, 3, 2), ("gauss", 20, 300, 17)):
        mod = model(ctx, kern, n, d, k)
        specs += [job(mod, 65, True, False), job(mod, 65, True, True)]
    got = batch(ctx, specs)
    for i in range(0, len(specs), 2):
        assert np.array_equal(got[i][0], got[i + 1][0]), i


def _mixed(ctx):
    """40 jobs over every path above, permuted; several models appear more than once"""
    pool = []
    for i in range(40):
        kern = sorted(KERNELS)[i % 5]
        d = (3, 65, 130, 300)[i % 4]
        n = (20, 257, 600)[i % 3]
        k = KS[(i // 2) % 4]
        v, j = SELECT[i % 3]
        pool.append(job(model(ctx, kern, n, d, k), MS[(i // 3) % 5], v, j, seed=i))
    order = np.random.default_rng(5).permutation(len(pool))
    return [pool[i] for i in order]


@pytest.fixture(scope="module")
def mixed(ctx):
    specs = _mixed(ctx)
    return specs, loop(ctx, specs)


@pytest.mark.parametrize("count", [1, 9, 40])
def test_mixed_batches(ctx, mixed, count):
    specs, ref = mixed
    same(batch(ctx, specs[:count]), ref[:count], count)
    if count == 9:   # position and company do not matter: the same jobs reversed, and one model in two jobs of one call
        same(batch(ctx, specs[:count][::-1]), ref[:count][::-1], "reversed")
        twice = [specs[0], specs[1], dict(specs[0], X=specs[0]["X"].copy())]
        same(batch(ctx, twice), [ref[0], ref[1], ref[0]], "one model twice")


def test_model_sources_and_release_order(ctx):
    from tests.test_gpu_fit_batch import _spec, batch as fit_batch, single as fit_single

    base = ctx.get_option(_lib.OPT_LIVE_HANDLES)
    fitted = [m for _, m in fit_batch(ctx, [_spec("cubic", 1, 129, 3, 2, seed) for seed in (1, 2, 3)])]
    fitted.append(fit_single(ctx, _spec("multiquadric", 0, 140, 65, 2, 4))[1])
    cfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    rng = np.random.default_rng(6)
    fitted.append(rm.model_from_coeffs(cfg, rng.uniform(-2, 2, (33, 3)), rng.standard_normal((33, 2)), rng.standard_normal((4, 2)), ctx=ctx))
    assert all(m is not None for m in fitted) and ctx.get_option(_lib.OPT_LIVE_HANDLES) == base + 5
    specs = [job(m, 65) for m in fitted] + [job(fitted[1], 7, True, False)]
    same(batch(ctx, specs), loop(ctx, specs))
    for i in (3, 0, 4, 2, 1):
        fitted[i].free()
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == base


def test_host_and_device_pointers_mixed(ctx, mixed):
    specs, ref = mixed
    specs, ref = specs[:12], ref[:12]
    dev = torch.device("cuda")
    n = len(specs)
    jobs = (_lib.EvalJob * n)()
    keep, where = [], []
    for i, s in enumerate(specs):
        mod, m = s["mod"], s["X"].shape[0]
        V, J = _buffers(s)
        # job i keeps X / values / Jacobians on the device by the bits of i; job 1's device buffers start on an odd double
        on_dev = [(i >> b) & 1 == 1 and a is not None and a.size > 0 for b, a in enumerate((s["X"], V, J))]
        odd = 1 if i % 4 == 1 else 0
        bufs = []
        for a, dv in zip((s["X"], V, J), on_dev):
            if dv:
                t = torch.full((a.size + odd,), float("nan"), dtype=torch.float64, device=dev)[odd:]
                if a is s["X"]:
                    t.copy_(torch.from_numpy(a.ravel()))
                assert t.data_ptr() % 16 == (8 if odd else 0)
                bufs.append(t)
            else:
                bufs.append(a)
        keep.append(bufs)
        where.append(on_dev)
        jobs[i].model, jobs[i].m = mod.model.value, m
        jobs[i].X, jobs[i].vals_out, jobs[i].jac_out = (None if a is None or (isinstance(a, np.ndarray) and a.size == 0) else _lib.as_ptr(a).value
                                                        for a in bufs)
    assert any(w[0] for w in where) and any(w[1] for w in where) and any(w[2] for w in where) and not all(w[0] for w in where)
    rc = ctx.lib.mrbf_eval_batch(ctx.h, n, jobs, None)     # ms_total may be NULL
    assert rc == 0, ctx.lib.mrbf_last_error(ctx.h)
    torch.cuda.synchronize()
    got = []
    for s, bufs in zip(specs, keep):
        V, J = _buffers(s)
        out = []
        for a, shaped in ((bufs[1], V), (bufs[2], J)):
            out.append(None if a is None else (a.cpu().numpy().reshape(shaped.shape) if isinstance(a, torch.Tensor) else a))
        got.append(tuple(out))
    same(got, ref, "pointers")


def test_gemm_pipeline_option(ctx, mixed):
    specs, ref_default = mixed
    specs = specs[:12]
    ctx.set_option(_lib.OPT_EVAL_IMPL, 1)
    try:
        ref = loop(ctx, specs)       # the single call under the same option
        same(batch(ctx, specs), ref, "eval_impl = 1")
    finally:
        ctx.set_option(_lib.OPT_EVAL_IMPL, 0)
    same(batch(ctx, specs), ref_default[:12], "back to the default")


def test_second_call_allocates_nothing(ctx, mixed):
    specs, ref = mixed
    same(batch(ctx, specs), ref)
    before = ctx.get_option(_lib.OPT_ARENA_BYTES)
    same(batch(ctx, specs), ref)
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) == before


def test_chunks_of_jobs():
    c = pkg.Context()       # a context of its own: its arena shows how much one call asked for
    try:
        specs = [job(model(c, "cubic3", 257, 65, 17), 65, True, True, seed=i) for i in range(6)] + [job(model(c, "tps1", 20, 3, 2), 64, seed=9)]
        ref = loop(c, specs)
        base = c.get_option(_lib.OPT_ARENA_BYTES)
        same(batch(c, specs, limit=1 << 20), ref, "1 MiB")      # a job's scratch and outputs are 2 MB: one job per chunk
        chunked = c.get_option(_lib.OPT_ARENA_BYTES) - base
        same(batch(c, specs, limit=1), ref, "1 byte")           # every job a chunk of its own
        assert c.get_option(_lib.OPT_ARENA_BYTES) - base == chunked
        same(batch(c, specs), ref, "one chunk")
        whole = c.get_option(_lib.OPT_ARENA_BYTES) - base
        print("arena: %d bytes in chunks, %d bytes in one" % (chunked, whole))
        assert 3 * chunked < whole
    finally:
        for key in [k for k in _ZOO if k[0] == id(c)]:
            _ZOO.pop(key).free()
        c.close()


def test_refusals(ctx):
    mod = model(ctx, "cubic3", 20, 3, 2)
    good = [job(mod, 5), job(mod, 3)]
    batch(ctx, [], expect_rc=-2)
    assert ctx.lib.mrbf_eval_batch(None, 1, None, None) == -1
    assert ctx.lib.mrbf_eval_batch(ctx.h, 65536, None, None) == -2
    assert ctx.lib.mrbf_eval_batch(ctx.h, 1, None, None) == -3
    for defect in ("model", "m", "X"):
        jobs = (_lib.EvalJob * 3)()
        outs = []
        for i, s in enumerate(good + [job(mod, 4)]):
            V, J = _buffers(s)
            outs.append((V, J))
            jobs[i].model, jobs[i].m, jobs[i].X = mod.model.value, s["X"].shape[0], s["X"].ctypes.data
            jobs[i].vals_out, jobs[i].jac_out = V.ctypes.data, J.ctypes.data
        if defect == "model":
            jobs[2].model = None
        elif defect == "m":
            jobs[2].m = -1
        else:
            jobs[2].X = None
        assert ctx.lib.mrbf_eval_batch(ctx.h, 3, jobs, None) == -3, defect
        assert all(np.isnan(V).all() and np.isnan(J).all() for V, J in outs), defect      # nothing launched, nothing written
        assert [jobs[i].status for i in range(3)] == [0, 0, {"model": -2, "m": -3, "X": -4}[defect]]
    # a model of another context
    other = pkg.Context()
    try:
        foreign = model(other, "cubic3", 20, 3, 2)
        s = job(foreign, 5)
        V, J = _buffers(s)
        jobs = (_lib.EvalJob * 1)()
        jobs[0].model, jobs[0].m, jobs[0].X, jobs[0].vals_out, jobs[0].jac_out = foreign.model.value, 5, s["X"].ctypes.data, V.ctypes.data, J.ctypes.data
        assert ctx.lib.mrbf_eval_batch(ctx.h, 1, jobs, None) == -4
        assert np.isnan(V).all() and np.isnan(J).all()
    finally:
        for key in [k for k in _ZOO if k[0] == id(other)]:
            _ZOO.pop(key).free()
        other.close()
    # legal: an empty block with a NULL X, a job without outputs
    specs = [job(mod, 0), job(mod, 5, False, False), job(mod, 5)]
    same(batch(ctx, specs), loop(ctx, specs), "legal")


# ---- bindings ---------------------------------------------------------------------------------------------------------------------
def test_eval_models_many(ctx, mixed):
    specs, ref = mixed
    specs, ref = specs[:12], ref[:12]
    stats = {}
    got = rm.eval_models_many([s["mod"] for s in specs], [s["X"] for s in specs], want_values=[s["vals"] for s in specs],
                              want_jac=[s["jac"] for s in specs], stats=stats, min_jobs=1)
    assert stats["path"] == "batch" and stats["jobs"] == len(specs)
    assert stats["single_inside"] == sum(1 for s in specs if s["mod"].d > 256 and s["X"].shape[0] > 0)
    for s, (V, J), (V0, J0) in zip(specs, got, ref):
        V1, J1 = s["mod"].eval_sites(s["X"], want_values=s["vals"], want_jac=s["jac"])
        for a, b in ((V, V1), (J, J1)):
            assert (a is None) == (b is None)
            assert a is None or (a.shape == b.shape and np.array_equal(a, b))
        assert J is None or np.array_equal(np.transpose(J, (0, 2, 1)), J0)
    # device tensors, in place
    s = next(s for s in specs if s["vals"] and s["jac"] and s["X"].shape[0] > 0)
    m, mod = s["X"].shape[0], s["mod"]
    Xd = torch.from_numpy(s["X"]).cuda()
    Vd = torch.full((m, mod.k), float("nan"), dtype=torch.float64, device="cuda")
    Jd = torch.full((m, mod.d, mod.k), float("nan"), dtype=torch.float64, device="cuda")
    out = rm.eval_models_many([mod, mod], [Xd, s["X"]], want_jac=True, outs=[(Vd, Jd), (None, None)], min_jobs=1)
    assert out[0][0] is Vd and out[0][1] is Jd
    assert np.array_equal(Vd.cpu().numpy(), out[1][0]) and np.array_equal(Jd.cpu().numpy().transpose(0, 2, 1), out[1][1])


class _Outer:
    num_outputs = 2

    def eval(self, xi):
        return np.array([np.sum(xi ** 2), xi[0] * xi[-1]])

    def jacobian(self, xi):
        J = np.zeros((2, xi.size))
        J[0] = 2 * xi
        J[1, 0], J[1, -1] = xi[-1], xi[0]
        return J


def test_container_twins(ctx):
    ns, d = 5, 65
    scs = []
    for p in range(ns):   # two grouped models for the objectives (one of them under a CompositeSurrogate as well), one modelled constraint
        a, b, c = model(ctx, "cubic3", 257 if p % 2 else 140, d, 3), model(ctx, "mq", 257, d, 2), model(ctx, "cubic1" if p == 3 else "gauss", 20, d, 2)
        scs.append(sg.SurrogateContainer(
            objectives=[sg.RefSurrogate(a, [2, 0]), sg.RefSurrogate(b, [1]), sg.CompositeSurrogate(b, _Outer(), [0, 1]), sg.RefSurrogate(a, [1])],
            nl_ineq_constraints=[sg.RefSurrogate(c, [0, 1])]))
    Xs = [queries(1 + 16 * p, d, seed=p) for p in range(ns)]
    for plural, n_inner in (("objectives", 2), ("nl_ineq_constraints", 1), ("nl_eq_constraints", 0)):
        for jac in (False, True):
            name = "eval_container_%s%s_at_scaled_sites" % (plural, "_jacobian" if jac else "")
            stats = {}
            got = getattr(sg, name + "_many")(scs, None, Xs, stats=stats, min_jobs=1)
            assert stats.get("jobs", 0) == ns * n_inner
            for p in range(ns):
                want = getattr(sg, name)(scs[p], None, Xs[p])
                assert got[p].shape == want.shape and np.array_equal(got[p], want), (name, p)


def test_keep_models_records(ctx):
    from tests.test_gpu_fit_batch import _data

    problems = []
    for p, (n, d) in enumerate([(20, 3), (129, 3), (140, 65), (257, 65), (33, 3)]):
        C, Y = _data(n, d, 2, 40 + p)
        problems.append({"id": p, "cfg": pkg.RbfConfig(kernel="cubic", polynomial_degree=1), "sites": C, "values": Y, "X": queries(70, d, p),
                         "want_jac": p % 2 == 0})
    tables = {}
    for floor in (1, 1 << 20):
        stats = {}
        table, kept = manystart.gpu_solve_shard_keep_models(problems, ctx=ctx, stats=stats, eval_min_jobs=floor)
        assert stats["eval"]["path"] == ("batch" if floor == 1 else "loop") and all(table[:, 1] == 0)
        tables[floor] = table
        for p, m in enumerate(kept):     # the record's checksum against one mrbf_eval on the very model the record was made from
            V, _ = m.eval_sites(problems[p]["X"], want_values=True, want_jac=problems[p]["want_jac"])
            assert table[p, manystart.RECORD_FIELDS.index("checksum_vals")] == float(np.sum(V)), (floor, p)
            m.free()
    cols = [manystart.RECORD_FIELDS.index(f) for f in ("problem_id", "status", "path", "checksum_w", "checksum_vals")]
    assert np.array_equal(tables[1][:, cols], tables[1 << 20][:, cols])
