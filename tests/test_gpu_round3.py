"""Round 3 for a batch of starts on the device (run with -m gpu): mrbf_db_round3_batch, mrbf_db_append_batch, mrbf_db_set_values_batch
and the resident phase-I driver against the host mirror (sampling._rbf_round3 on descent.intersect_box).  No tolerance anywhere: every
comparison is an equality of integers or of bits (uint64 views of the doubles, -0.0 counts), with one class: where the mirror has a NaN
the device must have a NaN and the payload is not compared -- IEEE 754 leaves the sign and payload of the NaN an invalid operation
(Inf * 0, Inf - Inf) produces to the implementation, and x86 and the GPU choose differently.

d in {1, 2, 3, 65, 128, 130, 257}: a single coordinate, the smallest even and odd row lengths, one lane stride crossed with an odd tail,
the two-coordinates-per-lane path filling a wave exactly, the same with a second, partial trip, and an odd row of five trips with more
than 256 fail flags on the axes (a second pass of the decision's loop); one start and five starts per call.  The boxes lie on a grid of step 1/8 and many
coordinates sit exactly on a bound."""
import ctypes

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, database, sampling
    from morbit.jl_amd.rbf_model import RbfConfig, update_models_many, update_models_resident

DS = (1, 2, 3, 65, 128, 130, 257)
SENTINEL = -777.25


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """equal bits, NaNs as a class (module docstring)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(bits(a)[ok], bits(b)[ok])


def real_Z(ctx, d, n_seeds, seed):
    """the final Z (d x dz) of a real mrbf_affine_select_batch over n_seeds random seeds around 0 (the identity for d = 1 or no seeds)"""
    if d == 1 or n_seeds == 0:
        return np.eye(d)
    rng = np.random.default_rng(seed)
    flt = sampling.AffinelyIndependentPointFilter(np.zeros(d), list(rng.uniform(-1, 1, (n_seeds, d))), pivot_val=1e-3)
    out, qr, S, i, _ = flt._begin()
    Sd, want = flt._device_job(out, qr, S, i)
    rc, res, _ = sampling.affine_select_batch_device([(Sd, qr, want, flt.pivot_val)], d, np.inf, ctx=ctx)
    assert rc == 0
    got, Z = res[0]
    assert Z.shape == (d, d - 1 - len(got))
    return Z


def box(d, seed, fixed=()):
    """x, lb, ub on the grid of step 1/8 inside [0, 1]^d, some coordinates of x exactly on lb or ub; `fixed`: lb = ub = x there"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 8, d) / 8.0
    lb, ub = x - rng.integers(0, 3, d) / 8.0, x + rng.integers(0, 3, d) / 8.0
    for j in range(d):
        if lb[j] == ub[j]:
            ub[j] += 0.125                       # (only `fixed` coordinates are pinched)
    for j in fixed:
        lb[j] = ub[j] = x[j]
    return x, lb, ub


def start(d, seed, dirs=None, rev=False, n_missing=None, max_new=10 ** 6, efl=False, force=False, mode=0, device=False, piv=1.0 / 64, fixed=(),
          n0=None, xlu=None):
    x, lb, ub = xlu if xlu is not None else box(d, seed, fixed)
    rows = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, d)
    n_dirs = d if rows is None else rows.shape[0]
    return dict(d=d, x=x, lb=lb, ub=ub, piv=piv, rows=rows, rev=rev, n_missing=n_dirs if n_missing is None else n_missing, max_new=max_new,
                efl=efl, force=force, mode=mode, device=device, n0=(seed % 4) if n0 is None else n0, seed=seed)


def expected(s):
    """(new_points, fully_linear, status, n_dirs_used) by the host mirror, or None for a job the reference's @assert refuses"""
    d = s["d"]
    n_dirs = d if s["rows"] is None else s["rows"].shape[0]
    if s["mode"] == 1:
        r = sampling._improve_host(s["lb"], s["ub"], s["x"], s["piv"], sampling._direction_rows(s["rows"], d, s["rev"]))
        return r.new_points, r.fully_linear, 0, min(n_dirs, 1)
    if n_dirs < max(0, min(s["n_missing"], s["max_new"])):
        return None
    (r,) = sampling.rbf_round3_many([s["lb"]], [s["ub"]], [s["x"]], s["piv"], [s["rows"]], s["max_new"], s["n_missing"], s["efl"], s["force"],
                                    reversed_order=s["rev"])
    return r.new_points, r.fully_linear, int(r.rebuilt), r.new_points.shape[0]


def make_db(ctx, s, k=2):
    """a database of capacity 4 with n0 evaluated rows"""
    db = database.DeviceDatabase(s["d"], k, ctx=ctx, capacity=4)
    rng = np.random.default_rng(1000 + s["seed"])
    if s["n0"]:
        db.append(rng.uniform(0, 1, (s["n0"], s["d"])), rng.uniform(-1, 1, (s["n0"], k)))
    return db


def call(ctx, d, starts, dbs):
    """one raw mrbf_db_round3_batch -> (rc, jobs, new_sites_out buffers)"""
    ns = len(starts)
    jobs = (_lib.Round3Job * max(ns, 1))()
    keep, outs = [], []
    for q, s in enumerate(starts):
        x, lb, ub = (np.ascontiguousarray(s[n], dtype=np.float64) for n in ("x", "lb", "ub"))
        D = s["rows"]
        if D is not None and s["device"]:
            D = torch.from_numpy(D.copy()).cuda()
        buf = np.full((max(s["n_missing"], d, 1), d), SENTINEL)
        keep.append((x, lb, ub, D))
        outs.append(buf)
        J = jobs[q]
        J.db, J.x, J.lb, J.ub, J.pivot_val = dbs[q].h, x.ctypes.data, lb.ctypes.data, ub.ctypes.data, s["piv"]
        if D is not None and int(D.shape[0]) == 0:                                     # an empty list is not the axes: a valid pointer, no columns
            keep.append(np.zeros(1))
            J.dirs = keep[-1].ctypes.data
        else:
            J.dirs = None if D is None else (D.data_ptr() if s["device"] else D.ctypes.data)
        J.n_dirs, J.reversed, J.n_missing, J.max_new = (0 if D is None else int(D.shape[0])), int(s["rev"]), s["n_missing"], min(s["max_new"], 2 ** 31 - 1)
        J.ensure_fully_linear, J.force_rebuild, J.mode = int(s["efl"]), int(s["force"]), s["mode"]
        J.new_sites_out = buf.ctypes.data
        J.rc, J.n_new, J.fully_linear, J.status, J.n_dirs_used, J.first_index = -9, -9, -9, -9, -9, -9
    rc = ctx.lib.mrbf_db_round3_batch(ctx.h, ns, d, jobs, None)
    torch.cuda.synchronize()
    return rc, jobs, outs, keep


def run(ctx, d, starts, tag=""):
    """the batch on fresh databases against the mirror, start by start; returns what the device gave per start"""
    dbs = [make_db(ctx, s) for s in starts]
    before = [db.read() for db in dbs]
    rc, jobs, outs, _ = call(ctx, d, starts, dbs)
    assert rc == 0, (tag, rc)
    got = []
    for q, s in enumerate(starts):
        J, db, exp, t = jobs[q], dbs[q], expected(s), (tag, q)
        n, _, k = db.dims()
        if exp is None:
            assert J.rc == -3 and n == s["n0"] and np.all(outs[q] == SENTINEL), t
            assert (J.n_new, J.fully_linear, J.status, J.n_dirs_used, J.first_index) == (-9, -9, -9, -9, -9), t     # outputs untouched
            got.append(None)
            continue
        pts, fl, status, used = exp
        m = pts.shape[0]
        print(t, "n_new", J.n_new, m, "fl", J.fully_linear, fl, "status", J.status, status)
        assert J.rc == 0, (t, J.rc)
        assert (J.n_new, bool(J.fully_linear), J.status, J.n_dirs_used, J.first_index) == (m, fl, status, used, s["n0"]), t
        assert n == s["n0"] + m, t                                                     # the row count, also after a rebuild
        assert same(outs[q][:m], pts) and np.all(outs[q][m:] == SENTINEL), t
        S = np.empty((n, d))
        V = np.empty((n, k))
        ctx.check(ctx.lib.mrbf_db_read(ctx.h, db.h, 0, n, _lib.as_ptr(S), _lib.as_ptr(V)))
        assert np.array_equal(bits(S[: s["n0"]]), bits(before[q][0])) and np.array_equal(bits(V[: s["n0"]]), bits(before[q][1])), t   # earlier rows keep their bits
        assert same(S[s["n0"]:], pts) and np.isnan(V[s["n0"]:]).all(), t
        got.append((bits(outs[q][:m]).copy(), int(J.fully_linear), int(J.status)))
    for db in dbs:
        db.free()
    return got


@pytest.mark.parametrize("ns", (1, 5))
@pytest.mark.parametrize("d", DS)
def test_directions_of_a_real_filter(ctx, d, ns):
    """Z of mrbf_affine_select_batch as a host array and as a device pointer, in order and reversed; n_new in {0, 1, dz}"""
    for device in (False, True):
        starts = []
        for q in range(ns):
            Z = real_Z(ctx, d, min(d - 1, 1 + q), 10 * d + q)                         # one to five seeds: dz from d - 1 down
            rows = np.ascontiguousarray(Z.T)                                          # the memory of the column-major d x dz Z
            dz = rows.shape[0]
            starts.append(start(d, 100 * d + q, rows, rev=bool(q % 2), n_missing=(dz, 1, 0, dz, dz)[q % 5], device=device,
                                max_new=(10 ** 6, 10 ** 6, 5, 1, 10 ** 6)[q % 5]))
        run(ctx, d, starts, ("filter", d, ns, device))


@pytest.mark.parametrize("ns", (1, 5))
@pytest.mark.parametrize("d", DS)
def test_axes_and_growth(ctx, d, ns):
    """dirs = NULL: the coordinate axes, n_new = d new rows on databases of capacity 4 (they grow for every d > 1)"""
    run(ctx, d, [start(d, 200 * d + q, None, n0=q % 4, max_new=10 ** 6 if q != 3 else 0) for q in range(ns)], ("axes", d, ns))


def failing(d, q, efl, force, seed):
    """a start whose coordinate 0 is fixed and whose directions (the axes, as an explicit list, last to first) include e0"""
    return start(d, seed, np.eye(d), rev=True, efl=efl, force=force, fixed=(0,), n0=q % 4)


@pytest.mark.parametrize("d", DS)
def test_failing_direction_beside_passing_starts(ctx, d):
    """each of the four (ensure_fully_linear, force_rebuild) settings on a failing start, beside starts that pass; a start's result
    does not depend on its position"""
    starts = [failing(d, 0, False, False, 300 * d), start(d, 300 * d + 1, np.eye(d), efl=True), failing(d, 2, True, False, 300 * d + 2),
              failing(d, 3, False, True, 300 * d + 3), failing(d, 4, True, True, 300 * d + 4)]
    got = run(ctx, d, starts, ("fail", d))
    assert [g[2] for g in got] == [0, 0, 1, 0, 0]                                      # only (efl, !force) rebuilds
    assert [g[1] for g in got] == [0, 1, 0, 0, 0]                                      # e0 fails on every other start, also after the rebuild
    perm = [3, 0, 4, 2, 1]
    again = run(ctx, d, [starts[p] for p in perm], ("fail-permuted", d))
    for pos, p in enumerate(perm):
        assert np.array_equal(again[pos][0], got[p][0]) and again[pos][1:] == got[p][1:], (d, p)
    for ref, s in zip(got, starts):                                                   # ... nor on having neighbours at all
        (alone,) = run(ctx, d, [s], ("fail-alone", d))
        assert np.array_equal(alone[0], ref[0]) and alone[1:] == ref[1:]


@pytest.mark.parametrize("d", (2, 3, 65, 128, 130))
def test_rebuild_that_succeeds(ctx, d):
    """x = (.5, ..), box [.25, .75]^d but lb0 = .5 - 2^-10 and ub1 = .5 + 2^-10.  Along e0 + e1 the steps are -2^-10, +.25 (coordinate 0)
    and -.25, +2^-10 (coordinate 1): sigma+ = sigma- = 2^-10, the offset's norm is below the pivot and the direction fails, while every
    axis reaches .25: with ensure_fully_linear the start is rebuilt and is fully linear; without it is kept and is not"""
    x, lb, ub = np.full(d, 0.5), np.full(d, 0.25), np.full(d, 0.75)
    lb[0], ub[1] = 0.5 - 2.0 ** -10, 0.5 + 2.0 ** -10
    rows = np.eye(d)
    rows[0, 1] = 1.0
    a, b = run(ctx, d, [start(d, 1, rows, efl=True, xlu=(x, lb, ub), piv=0.1, n0=3), start(d, 2, rows, xlu=(x, lb, ub), piv=0.1, n0=3)], ("rebuild", d))
    assert (a[1], a[2]) == (1, 1) and (b[1], b[2]) == (0, 0)
    # a pivot value no axis passes: rebuilt, and still not fully linear
    (c,) = run(ctx, d, [start(d, 3, rows, efl=True, xlu=(x, lb, ub), piv=0.3)], ("rebuild-fails", d))
    assert (c[1], c[2]) == (0, 1)


@pytest.mark.parametrize("d", DS)
def test_zero_direction_and_signed_zeros(ctx, d):
    """a zero direction gives len = Inf and a NaN row, which does not fail (no rebuild with ensure_fully_linear); -0.0 in x and in the
    directions comes out as the host's x .+ len .* dir has it"""
    rows = np.zeros((2, d))
    rows[1, d - 1] = 1.0
    rows[1, 0] = -0.0 if d > 1 else 1.0
    x, lb, ub = np.zeros(d), np.full(d, -1.0), np.full(d, 1.0)
    x[0] = -0.0
    (g,) = run(ctx, d, [start(d, 5, rows, efl=True, xlu=(x, lb, ub), n0=1)], ("zero", d))
    assert g[2] == 0 and g[1] == 1
    neg = -np.eye(d)                                                                   # offsets len * (-0.0) and len * (-1)
    run(ctx, d, [start(d, 6, neg, xlu=(x, lb, ub)), start(d, 7, neg, rev=True, xlu=(-x, lb, ub), device=True)], ("signed", d))


@pytest.mark.parametrize("d", DS)
def test_improve_mode(ctx, d):
    rows = np.eye(d)[::-1].copy()
    starts = [start(d, 400 * d, rows, mode=1),                                          # passes; fully linear only with one direction
              start(d, 400 * d + 1, rows[:1], mode=1, device=True),
              start(d, 400 * d + 2, np.eye(d), mode=1, fixed=(0,)),                     # e0 in a fixed coordinate: nothing appended
              start(d, 400 * d + 3, np.zeros((1, d)), mode=1),                          # NaN norm: nothing appended (RbfModel.jl:718)
              start(d, 400 * d + 4, np.zeros((0, d)), mode=1)]                          # no directions left
    got = run(ctx, d, starts, ("improve", d))
    assert [g[0].shape[0] for g in got] == [1, 1, 0, 0, 0]
    assert [g[1] for g in got] == [1 if d == 1 else 0, 1, 0, 0, 0]


def test_refusals_and_a_failing_job_beside_good_ones(ctx):
    d = 3
    good = [start(d, 500 + q, np.eye(d)) for q in range(3)]
    dbs = [make_db(ctx, s) for s in good]
    other = database.DeviceDatabase(4, 2, ctx=ctx)
    assert ctx.lib.mrbf_db_round3_batch(ctx.h, 0, d, (_lib.Round3Job * 1)(), None) == -2
    assert ctx.lib.mrbf_db_round3_batch(ctx.h, 3, 4097, (_lib.Round3Job * 3)(), None) == -2
    assert ctx.lib.mrbf_db_round3_batch(ctx.h, 3, d, None, None) == -4
    for what in ("other_d", "twice", "null_x", "mode", "n_dirs", "null_db"):
        rc, jobs, outs, keep = None, None, None, None
        use = list(dbs)
        if what == "other_d":
            use[1] = other
        if what == "twice":
            use[2] = dbs[0]
        ns = len(good)
        jobs = (_lib.Round3Job * ns)()
        bufs = []
        for q, s in enumerate(good):
            arrs = [np.ascontiguousarray(s[n]) for n in ("x", "lb", "ub", "rows")] + [np.full((d, d), SENTINEL)]
            bufs.append(arrs)
            J = jobs[q]
            J.db, J.x, J.lb, J.ub, J.dirs, J.new_sites_out = use[q].h, *(a.ctypes.data for a in arrs)
            J.pivot_val, J.n_dirs, J.n_missing, J.max_new = s["piv"], d, d, 100
        if what == "null_x":
            jobs[1].x = None
        if what == "mode":
            jobs[2].mode = 2
        if what == "n_dirs":
            jobs[0].n_dirs = -1
        if what == "null_db":
            jobs[1].db = None
        assert ctx.lib.mrbf_db_round3_batch(ctx.h, ns, d, jobs, None) == -4, what
        assert [db.dims()[0] for db in dbs] == [s["n0"] for s in good], what           # nothing written
        assert all(np.all(b[4] == SENTINEL) for b in bufs), what
    for db in dbs + [other]:
        db.free()
    # n_dirs < n_new is the job's own failure (-3): its outputs and its database stay as they were, the others are served
    bad = start(d, 510, np.eye(d)[:2], n_missing=3)
    run(ctx, d, [good[0], bad, good[1]], "assert")


def test_second_identical_call_allocates_nothing(ctx):
    d = 65
    starts = [start(d, 600 + q, None, efl=True, fixed=(q,)) for q in range(5)]
    dbs = [make_db(ctx, s) for s in starts]
    for db in dbs:                                                                    # room for both calls: no reallocation of a database either
        db.append(np.zeros((300, d)), np.zeros((300, 2)))
    assert call(ctx, d, starts, dbs)[0] == 0
    arena = ctx.get_option(_lib.OPT_ARENA_BYTES)
    rc, jobs, _, _ = call(ctx, d, starts, dbs)
    assert rc == 0 and all(J.rc == 0 and J.status == 1 for J in jobs)
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) == arena
    for db in dbs:
        db.free()


# ---- the batched siblings of append and set_values ------------------------------------------------------------------------------------

def test_append_many_and_set_values_many_match_the_single_calls(ctx):
    rng = np.random.default_rng(7)
    shapes = [(1, 1), (3, 2), (65, 1), (128, 3), (2, 17)]                              # (d, k): the databases of a call may differ
    a = [database.DeviceDatabase(d, k, ctx=ctx, capacity=4) for d, k in shapes]
    b = [database.DeviceDatabase(d, k, ctx=ctx, capacity=4) for d, k in shapes]
    for rnd, ms in enumerate(([3, 0, 5, 70, 1], [2, 4, 0, 1, 130])):                   # growth from capacity 4, past 64 rows, empty jobs
        S = [rng.uniform(-1, 1, (m, d)) for m, (d, k) in zip(ms, shapes)]
        V = [rng.uniform(-1, 1, (m, k)) if q % 2 == rnd % 2 else None for q, (m, (d, k)) in enumerate(zip(ms, shapes))]
        for q in (2, 3):                                                              # device-side rows are read in place
            S[q] = torch.from_numpy(S[q]).cuda()
        st = {}
        firsts = database.append_many(a, S, V, ctx=ctx, stats=st)
        assert st["path"] == "device"
        assert firsts == [db.append(S[q], V[q]) for q, db in enumerate(b)]
    for da, db_ in zip(a, b):
        assert len(da) == len(db_) and da.dims() == db_.dims()
        for x, y in zip(da.read(), db_.read()):
            assert same(x, y) and np.array_equal(np.isnan(x), np.isnan(y))
        assert same(da.sites, db_.sites) and same(da.values, db_.values)               # the host copies too
    # eval_missing!: the NaN rows of every database, one of the jobs with a device tensor; NaN payloads are the library's own here, so
    # plain bit equality holds
    idx = [np.flatnonzero(np.isnan(db.values).any(axis=1)) for db in a]
    vals = [rng.uniform(-1, 1, (i.size, db.k)) for i, db in zip(idx, a)]
    vals_in = list(vals)
    vals_in[4] = torch.from_numpy(vals[4]).cuda()
    st = {}
    assert database.set_values_many(a, idx, vals_in, ctx=ctx, stats=st) == [0] * 5 and st["path"] == "device"
    for q, db_ in enumerate(b):
        db_.set_values(idx[q], vals[q])
    for da, db_ in zip(a, b):
        for x, y in zip(da.read(), db_.read()):
            assert np.array_equal(bits(x), bits(y))
        assert np.array_equal(bits(da.values), bits(db_.values))
    # a bad index in one job only: that job's rc is -4 and nothing of it is written, the others are
    before = a[1].read()[1].copy()
    new = [np.full((2, db.k), 3.5) for db in a]
    lists = [[0, len(db) - 1] for db in a]
    lists[1] = [0, len(a[1])]
    assert database.set_values_many(a, lists, new, ctx=ctx, strict=False) == [0, -4, 0, 0, 0]
    assert np.array_equal(bits(a[1].read()[1]), bits(before)) and np.array_equal(bits(a[1].values), bits(before))
    for q in (0, 2, 3, 4):
        V = a[q].read()[1]
        assert np.all(V[[0, -1]] == 3.5) and np.array_equal(bits(V), bits(a[q].values))
    with pytest.raises(_lib.MrbfError):
        database.set_values_many(a, lists, new, ctx=ctx)
    # refusals: no starts; a database named twice; a NULL sites pointer
    assert ctx.lib.mrbf_db_append_batch(ctx.h, 0, (_lib.DbAppendJob * 1)(), None) == -2
    assert ctx.lib.mrbf_db_set_values_batch(ctx.h, 0, (_lib.DbSetValuesJob * 1)(), None) == -2
    jobs = (_lib.DbAppendJob * 2)()
    row = np.zeros(3)
    for J in jobs:
        J.db, J.m, J.sites = a[1].h, 1, row.ctypes.data
    n = len(a[1])
    assert ctx.lib.mrbf_db_append_batch(ctx.h, 2, jobs, None) == -3 and a[1].dims()[0] == n
    jobs[1].db, jobs[1].sites = a[0].h, None
    assert ctx.lib.mrbf_db_append_batch(ctx.h, 2, jobs, None) == -3 and a[1].dims()[0] == n
    for db in a + b:
        db.free()


# ---- phase I + fit, resident against host ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", (3, 65, 130))
def test_three_iterations_of_phase_one_and_fit(ctx, d):
    """five starts, start 2 with a fixed coordinate (it rebuilds): prepare_update_models + update_models_resident on resident databases against
    prepare_update_models + update_models_many on host databases: equal metas, equal database contents, equal weights"""
    ns, k = 5, 2
    cfg = RbfConfig(kernel="cubic")
    rng = np.random.default_rng(d)
    lb, ub = np.zeros(d), np.ones(d)
    f = lambda X: np.stack([np.sum(X * X, axis=1), np.sum(np.cos(X), axis=1)], axis=1)
    host = [database.HostDatabase(d, k) for _ in range(ns)]
    dev = [database.DeviceDatabase(d, k, ctx=ctx, capacity=4) for _ in range(ns)]
    fixed_lb, fixed_ub = lb.copy(), ub.copy()
    fixed_lb[d - 1] = fixed_ub[d - 1] = 0.5
    for p in range(ns):
        X = rng.integers(2, 7, (1 + 2 * p, d)) / 8.0
        if p == 2:
            X[:, d - 1] = 0.5
        for db in (host[p], dev[p]):
            db.append(X, f(X))
    x_idx = [0] * ns
    delta, delta_max = 0.125, 0.5
    for it in range(3):
        efl = it != 1
        metas = []
        for dbs, prep in ((host, sampling.prepare_update_models), (dev, sampling.prepare_update_models)):
            ms = [None] * ns
            for group, (l, u) in (([0, 1, 3, 4], (lb, ub)), ([2], (fixed_lb, fixed_ub))):      # the bounds are one per call
                res = prep(cfg, [dbs[p] for p in group], [dbs[p].sites[x_idx[p]].copy() for p in group], [x_idx[p] for p in group], delta,
                           delta_max, l, u, ensure_fully_linear=efl, ctx=ctx)
                for p, m in zip(group, res):
                    ms[p] = m
            metas.append(ms)
        for p in range(ns):
            mh, md = metas[0][p], metas[1][p]
            print(it, p, {key: mh[key] for key in mh if key != "improving_directions"})
            for key in ("center_index", "round1_indices", "round2_indices", "round3_indices", "round4_indices", "fully_linear", "rebuilt"):
                assert mh[key] == md[key], (it, p, key, mh[key], md[key])
            assert len(mh["improving_directions"]) == len(md["improving_directions"])
            for u, v in zip(mh["improving_directions"], md["improving_directions"]):
                assert same(u, v), (it, p)
        assert metas[0][2]["rebuilt"] == efl                                           # the fixed coordinate: rebuilt whenever full linearity is asked for
        # eval_missing! for every start
        miss = [np.flatnonzero(np.isnan(db.values).any(axis=1)) for db in host]
        vals = [f(db.sites[i]) for db, i in zip(host, miss)]
        for db, i, v in zip(host, miss, vals):
            db.set_values(i, v)
        database.set_values_many(dev, miss, vals, ctx=ctx)
        for p in range(ns):
            S, V = dev[p].read()
            assert len(dev[p]) == len(host[p]) == dev[p].dims()[0]
            assert same(S, host[p].sites) and same(V, host[p].values) and same(dev[p].sites, S) and same(dev[p].values, V), (it, p)
        idx = [[m["center_index"], *m["round1_indices"], *m["round2_indices"], *m["round3_indices"], *m["round4_indices"]] for m in metas[0]]
        fls = [m["fully_linear"] for m in metas[0]]
        mh = update_models_many(cfg, [host[p].sites[idx[p]] for p in range(ns)], [host[p].values[idx[p]] for p in range(ns)], delta, fls, ctx=ctx)
        md = update_models_resident(cfg, dev, idx, delta, fls, ctx=ctx)
        for p in range(ns):
            assert (mh[p] is None) == (md[p] is None), (it, p)
            if mh[p] is not None:
                assert np.array_equal(bits(mh[p].weights), bits(md[p].weights)) and np.array_equal(bits(mh[p].poly), bits(md[p].poly)), (it, p)
        # the next iterate: the newest row of every start
        x_idx = [len(db) - 1 for db in host]
        delta = 0.25 if it == 0 else 0.125


def test_one_round_on_resident_and_on_host_databases(ctx):
    """d = 8, three starts of 40 sites: find, round 3 with its sites appended, round 4 -- the three drivers called directly, once on
    DeviceDatabases and once on HostDatabases holding the same rows: equal tuples, Round3Results, accepted lists, routing stats and
    database contents.  Every round has work: 5 + p unit steps inside the inner box, the other sites spread over [0, 1]^8."""
    d, ns, n, k = 8, 3, 40, 2
    rng = np.random.default_rng(8)
    cfg = RbfConfig(kernel="cubic")
    f = lambda X: np.stack([np.sum(X * X, axis=1), np.sum(np.cos(X), axis=1)], axis=1)
    host = [database.HostDatabase(d, k) for _ in range(ns)]
    dev = [database.DeviceDatabase(d, k, ctx=ctx, capacity=4) for _ in range(ns)]
    for p in range(ns):
        X = rng.integers(0, 65, (n, d)) / 64.0
        X[: 6 + p] = 0.5
        for i in range(5 + p):
            X[1 + i, i] += (8 + i) / 64.0
        for db in (host[p], dev[p]):
            db.append(X, f(X))
    xs, x_idx, piv = [np.full(d, 0.5) for _ in range(ns)], [0] * ns, 1.0 / 16
    lb1, ub1 = [x - 0.25 for x in xs], [x + 0.25 for x in xs]
    lb2, ub2 = [np.zeros(d)] * ns, [np.ones(d)] * ns
    runs = []
    for dbs in (dev, host):
        s1, s3, s4 = {}, {}, {}
        r1 = sampling.find_suitable_points_many(dbs, lb1, ub1, xs, x_idx, piv, stats=s1, ctx=ctx)
        r3 = sampling.rbf_round3_append(dbs, lb1, ub1, xs, piv, [r[1] for r in r1], 10 ** 9, [d - len(r[0]) for r in r1], ctx=ctx, stats=s3)
        found = [[0, *r1[p][0], *r3[p].indices] for p in range(ns)]
        r4 = sampling.rbf_round4_many(dbs, lb2, ub2, xs, 0.125, found, cfg, ctx=ctx, stats=s4, min_starts=1)
        runs.append((r1, r3, found, r4, s1, s3["path"], s4))
    (r1d, r3d, fd, r4d, s1d, p3d, s4d), (r1h, r3h, fh, r4h, s1h, p3h, s4h) = runs
    assert s1d == s1h and s4d == s4h and (p3d, p3h) == ("device", "host") and fd == fh and r4d == r4h
    for p in range(ns):
        a, b = r1d[p], r1h[p]
        assert a[0] == b[0] and a[2] == b[2] and len(a[0]) >= 5 + p and same(a[3], b[3]) and same(a[4], b[4]), p
        assert len(a[1]) == len(b[1]) and all(same(u, v) for u, v in zip(a[1], b[1])), p
        a, b = r3d[p], r3h[p]
        assert same(a.new_points, b.new_points) and a.indices == b.indices and len(a.indices) == d - len(r1h[p][0]) > 0, p
        assert (a.fully_linear, a.rebuilt) == (b.fully_linear, b.rebuilt) and len(a.remaining_directions) == len(b.remaining_directions), p
        assert all(same(u, v) for u, v in zip(a.remaining_directions, b.remaining_directions)) and len(r4h[p]) > 0, p
        S, V = dev[p].read()
        assert len(dev[p]) == len(host[p]) == dev[p].dims()[0] == n + len(a.indices)
        assert same(S, host[p].sites) and same(V, host[p].values) and same(dev[p].sites, S) and same(dev[p].values, V), p
    for db in dev:
        db.free()


def test_filter_Z_left_on_the_device_feeds_round3_in_place(ctx):
    """d = 65, five starts whose databases lie in the subspace x_60 .. x_64 = 1/2 (80 sites around the centre): the batched pick loop
    serves every start and leaves at least five columns in Z.  With `keep_Z_on_device` the final Z is a device tensor holding the bits
    the host array holds without it, and phase I with ensure_fully_linear (round 2 skipped, Z read in place by round 3) gives the metas
    and the database contents of the host-array driver."""
    d, ns, k = 65, 5, 1
    rng = np.random.default_rng(65)
    cfg = RbfConfig(kernel="cubic")
    host = [database.HostDatabase(d, k) for _ in range(ns)]
    dev = [database.DeviceDatabase(d, k, ctx=ctx) for _ in range(ns)]
    for p in range(ns):
        X = 0.5 + rng.uniform(-0.2, 0.2, (80 + p, d))
        X[:, 60:] = 0.5
        X[0] = 0.5
        for db in (host[p], dev[p]):
            db.append(X, np.sum(X, axis=1, keepdims=True))
    xs, x_idx = [np.full(d, 0.5) for _ in range(ns)], [0] * ns
    lb1, ub1 = [x - 0.25 for x in xs], [x + 0.25 for x in xs]
    plain = sampling.find_suitable_points_many(dev, lb1, ub1, xs, x_idx, 1.0 / 16, ctx=ctx)
    st = {}
    kept = sampling.find_suitable_points_many(dev, lb1, ub1, xs, x_idx, 1.0 / 16, ctx=ctx, keep_Z_on_device=[True, True, False, True, True], stats=st)
    assert st["batched"] == list(range(ns))
    for p in range(ns):
        assert plain[p][0] == kept[p][0] and plain[p][2] == kept[p][2] and same(plain[p][3], kept[p][3])
        Z = plain[p][4]
        assert isinstance(Z, np.ndarray) and Z.shape[0] == d and Z.shape[1] >= 5
        if p == 2:
            assert isinstance(kept[p][4], np.ndarray) and same(kept[p][4], Z)
            continue
        T = kept[p][4]
        assert T.is_cuda and kept[p][1] is T and tuple(T.shape) == (Z.shape[1], d)
        assert np.array_equal(bits(T.cpu().numpy()), bits(Z.T))                      # rows of the tensor = columns of Z
        rows = [r for r in T.cpu().numpy()][::-1]
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(rows, plain[p][1]))  # last to first = the improving directions
    mh = sampling.prepare_update_models(cfg, host, xs, x_idx, 0.125, 0.5, np.zeros(d), np.ones(d), ensure_fully_linear=True, ctx=ctx)
    md = sampling.prepare_update_models(cfg, dev, xs, x_idx, 0.125, 0.5, np.zeros(d), np.ones(d), ensure_fully_linear=True, ctx=ctx)
    for p in range(ns):
        for key in ("center_index", "round1_indices", "round2_indices", "round3_indices", "round4_indices", "fully_linear", "rebuilt"):
            assert mh[p][key] == md[p][key], (p, key, mh[p][key], md[p][key])
        assert len(mh[p]["round3_indices"]) >= 5 and not mh[p]["rebuilt"] and mh[p]["improving_directions"] == md[p]["improving_directions"] == []
        S, V = dev[p].read()
        assert same(S, host[p].sites) and same(V, host[p].values) and same(dev[p].sites, S)
    for db in dev:
        db.free()


def test_prepare_improve_models_resident(ctx):
    """the improvement step of five metas in one call against prepare_improve_model's lines on the host: a meta that is fully linear or
    has no direction left is not touched; a step that passes moves its index into round 1 and drops the direction; the last direction
    makes the model fully linear; a direction in a fixed coordinate is dropped without a new site"""
    d, k = 3, 1
    cfg = RbfConfig()
    lb, ub = np.array([0.0, 0.0, 0.5]), np.array([1.0, 1.0, 0.5])                     # coordinate 2 is fixed
    x = np.array([0.5, 0.5, 0.5])
    E3 = np.eye(d)
    dirs = [[E3[0], E3[1]], [E3[1]], [E3[2], E3[0]], [], [E3[0]]]
    metas = [dict(fully_linear=(p == 4), improving_directions=list(dirs[p]), round1_indices=[7]) for p in range(5)]
    dbs = [database.DeviceDatabase(d, k, ctx=ctx, capacity=4) for _ in range(5)]
    for db in dbs:
        db.append(x[None, :], np.zeros((1, k)))
    sampling.prepare_improve_models(dbs, metas, cfg, [x] * 5, 0.125, lb, ub, ctx=ctx)
    # Delta_1 = .25, box [.25, .75]^2 x {.5}, pivot 1/16: e0 and e1 reach .25 (the tie picks +), e2 reaches 0
    want = [([7, 1], [[0.75, 0.5, 0.5]], [E3[1]], False), ([7, 1], [[0.5, 0.75, 0.5]], [], True), ([7], [], [E3[0]], False), ([7], [], [], False),
            ([7], [], [E3[0]], True)]
    for p, (r1, new, rem, fl) in enumerate(want):
        m = metas[p]
        assert m["round1_indices"] == r1 and m["fully_linear"] is fl and len(m["improving_directions"]) == len(rem), (p, m)
        assert all(np.array_equal(a, b) for a, b in zip(m["improving_directions"], rem)), p
        S, V = dbs[p].read()
        assert S[1:].tolist() == new and np.isnan(V[1:]).all() and len(dbs[p]) == 1 + len(new) and same(dbs[p].sites, S), p
        dbs[p].free()
