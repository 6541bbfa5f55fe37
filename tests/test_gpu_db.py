"""The resident site database on the device (run with -m gpu): mrbf_db_* / mrbf_db_box_batch / mrbf_db_gather_batch and the resident
twins of the many-start drivers against the host mirror.  No tolerance anywhere: every comparison is an equality of integers or of
bits (uint64 views of the doubles; -0.0 and NaN payloads count).

B = 64 is the number of database rows a workgroup of the flag and compaction kernels takes (csrc/db_host.hpp, db::ROWS): the box scans
run on n_sites in {1, B - 1, B, B + 1, 3 B + 7} = {1, 63, 64, 65, 199}, on d in {1, 3, 65, 128, 130, 257} (less than a wave, an odd row
length, more than a wave with an odd tail, two coordinates per lane in exactly one trip, the same with a second, partial trip, an odd
row of five trips); one scan and one gather run at the library's limit d = 4096.

The sites of test 1 lie on a grid of step 1/2 with the bounds and the centre on that grid: many coordinates sit exactly on lb or ub,
rows tie in norm, and the sums of squares of the 2-norm are exact in fp64 whatever their order (multiples of 1/4 below 2^11), so that
np.linalg.norm gives the norms the device gives, bit for bit."""
import ctypes

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, database, sampling

B = 64
SIZES = (1, B - 1, B, B + 1, 3 * B + 7)
SENTINEL = -777.25


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def grid_sites(n, d, seed):
    """rows on the grid {-1, -1/2, 0, 1/2, 1}^d (inside [-1, 1]^d, many coordinates exactly on a bound); about a third of them with one
    coordinate at +-3/2; row 2 (where there is one) with a NaN"""
    rng = np.random.default_rng(seed)
    S = rng.integers(-2, 3, (n, d)) * 0.5
    for i in range(n):
        if rng.random() < 0.35:
            S[i, rng.integers(d)] = 1.5 * rng.choice([-1.0, 1.0])
    if n > 2:
        S[2, rng.integers(d)] = np.nan
    return S


def reference(S, lb, ub, x0, exclude, p, zero):
    idx = sampling.results_in_box_indices(S, lb, ub, exclude)
    sites = S[idx].reshape(len(idx), S.shape[1])
    shifted = sites - x0
    pick, first = -1, None
    if idx:
        pick = int(np.argmax(np.linalg.norm(shifted, ord=p, axis=1)))
        first = shifted[pick].copy()
        if zero:
            shifted[pick] = 0.0
    return idx, sites, shifted, pick, first


def raw_box(ctx, dbs, lbs, ubs, x0s, excludes, p, zero, d):
    """one mrbf_db_box_batch call with every optional output given: (rc, jobs, [(indices, sites_out, shifted_out, first_row)])"""
    ns = len(dbs)
    jobs = (_lib.DbBoxJob * ns)()
    keep = []
    for q, db in enumerate(dbs):
        n = len(db)
        ex = np.ascontiguousarray(excludes[q], dtype=np.int64).reshape(-1)
        bufs = (np.ascontiguousarray(lbs[q], dtype=np.float64), np.ascontiguousarray(ubs[q], dtype=np.float64),
                np.ascontiguousarray(x0s[q], dtype=np.float64), ex, np.full(max(n, 1), -5, dtype=np.int64), np.full((max(n, 1), d), SENTINEL),
                np.full((max(n, 1), d), SENTINEL), np.full(d, SENTINEL))
        keep.append(bufs)
        J = jobs[q]
        J.db, J.lb, J.ub, J.x0 = db.h, bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data
        J.n_exclude, J.exclude, J.zero_first_pick = ex.size, ex.ctypes.data if ex.size else None, 1 if zero else 0
        J.indices_out, J.sites_out, J.shifted_out, J.first_row = (b.ctypes.data for b in bufs[4:])
        J.mc, J.first_pick, J.rc = -9, -9, -9
    rc = ctx.lib.mrbf_db_box_batch(ctx.h, ns, d, 1 if np.isinf(p) else 0, jobs, None)
    return rc, jobs, [b[4:] for b in keep]


def check_box(ctx, J, out, S, lb, ub, x0, exclude, p, zero, tag):
    idx, sites, shifted, pick, first = reference(S, lb, ub, x0, exclude, p, zero)
    indices_out, sites_out, shifted_out, first_row = out
    assert J.rc == 0 and J.mc == len(idx), (tag, J.rc, J.mc, len(idx))
    mc = len(idx)
    assert list(indices_out[:mc]) == idx and np.all(indices_out[mc:] == -5), tag
    assert same_bits(sites_out[:mc], sites) and same_bits(shifted_out[:mc], shifted), tag
    assert np.all(sites_out[mc:] == SENTINEL) and np.all(shifted_out[mc:] == SENTINEL), tag       # nothing behind the candidates
    assert J.first_pick == pick, (tag, J.first_pick, pick)
    if mc:
        assert same_bits(first_row, first), tag
        if zero:
            assert not shifted_out[pick].any(), tag
        else:
            assert same_bits(shifted_out[pick], first), tag
        # the views hold what the copies hold
        assert same_bits(view_to_host(ctx, J.cand_sites_dev, mc, S.shape[1]), sites), tag
        assert same_bits(view_to_host(ctx, J.shifted_dev, mc, S.shape[1]), shifted), tag
    else:
        assert np.all(first_row == SENTINEL), tag


def view_to_host(ctx, ptr, rows, d):
    """the `rows` x d doubles at device address `ptr`, read through the library itself: appended in place to a scratch database"""
    tmp = database.DeviceDatabase(d, 1, ctx=ctx, capacity=rows)
    ctx.check(ctx.lib.mrbf_db_append(ctx.h, tmp.h, rows, ctypes.c_void_p(ptr), None, None))
    out = np.empty((rows, d))
    ctx.check(ctx.lib.mrbf_db_read(ctx.h, tmp.h, 0, rows, _lib.as_ptr(out), None))
    tmp.free()
    return out


def exclude_variants(n, centre):
    return {"none": [], "centre": [centre], "dups": [centre, centre, n + 5, -1, min(1, n - 1)], "all": list(range(n))}


def bounds_variants(d):
    lb, ub = np.full(d, -1.0), np.full(d, 1.0)
    lbi, ubi = lb.copy(), ub.copy()
    lbi[0], ubi[d - 1] = -np.inf, np.inf
    if d > 1:
        lbi[d - 1] = -np.inf
    return {"finite": (lb, ub), "inf": (lbi, ubi)}


@pytest.mark.parametrize("d", [1, 3, 65, 128, 130, 257])
def test_box_scan_against_the_host_mirror(ctx, d):
    """test 1, one start per call: every size, exclude list, bound vector, norm and both settings of zero_first_pick"""
    for n in SIZES:
        S = grid_sites(n, d, 1000 * d + n)
        db = database.DeviceDatabase(d, 1, ctx=ctx)
        db.append(S)
        centre = n // 2
        x0 = np.nan_to_num(S[centre], nan=0.5)
        for ename, ex in exclude_variants(n, centre).items():
            for bname, (lb, ub) in bounds_variants(d).items():
                for p in (np.inf, 2):
                    for zero in (True, False):
                        rc, jobs, outs = raw_box(ctx, [db], [lb], [ub], [x0], [ex], p, zero, d)
                        assert rc == 0, ctx.lib.mrbf_last_error(ctx.h)
                        check_box(ctx, jobs[0], outs[0], S, lb, ub, x0, ex, p, zero, (d, n, ename, bname, p, zero))
        db.free()


@pytest.mark.parametrize("d", [1, 3, 65, 128, 130, 257])
def test_box_scan_five_starts_in_one_call(ctx, d):
    """test 1, a batch: five starts with different n_sites and exclude lists, the B-row start with an empty box, one with infinite bounds"""
    sizes = (B - 1, B, 3 * B + 7, 1, B + 1)
    Ss = [grid_sites(n, d, 2000 * d + n) for n in sizes]
    dbs = []
    for S in Ss:
        dbs.append(database.DeviceDatabase(d, 2, ctx=ctx, capacity=len(S)))
        dbs[-1].append(S)
    x0s = [np.nan_to_num(S[len(S) // 2], nan=-0.5) for S in Ss]
    fin, inf = bounds_variants(d)["finite"], bounds_variants(d)["inf"]
    lbs, ubs = [fin[0], np.full(d, 7.0), inf[0], fin[0], fin[0]], [fin[1], np.full(d, 7.0), inf[1], fin[1], fin[1]]
    exs = [exclude_variants(len(S), len(S) // 2)[k] for S, k in zip(Ss, ("dups", "none", "centre", "none", "all"))]
    for p in (np.inf, 2):
        for zero in (True, False):
            rc, jobs, outs = raw_box(ctx, dbs, lbs, ubs, x0s, exs, p, zero, d)
            assert rc == 0, ctx.lib.mrbf_last_error(ctx.h)
            for q in range(5):
                check_box(ctx, jobs[q], outs[q], Ss[q], lbs[q], ubs[q], x0s[q], exs[q], p, zero, (d, q, p, zero))
            assert jobs[1].mc == 0 and jobs[1].first_pick == -1 and jobs[4].mc == 0
    # the Python mirror gives the same, and the host path (what the decision table's refusal takes) gives what the device gives
    got = database.box_many(dbs, lbs, ubs, x0s, exs, p=np.inf, zero_first_pick=True, ctx=ctx)
    for q in range(5):
        idx, sites, shifted, pick, first = reference(Ss[q], lbs[q], ubs[q], x0s[q], exs[q], np.inf, True)
        host = database._box_host(dbs[q], lbs[q], ubs[q], x0s[q], exs[q], np.inf, True)
        assert got[q].indices == idx == host.indices and got[q].first_pick == pick == host.first_pick
        assert same_bits(np.asarray(got[q].shifted), shifted) and same_bits(host.shifted, shifted) and same_bits(np.asarray(got[q].sites), sites)
    for db in dbs:
        db.free()


@pytest.mark.parametrize("zero", [True, False])
def test_box_scan_at_the_widest_row(ctx, zero):
    """test 1 at the library's limit d = 4096 (32 trips of two coordinates per lane), n = B + 1 (a second, one-row workgroup), inf-norm"""
    d, n = 4096, B + 1
    S = grid_sites(n, d, 4096)
    db = database.DeviceDatabase(d, 1, ctx=ctx)
    db.append(S)
    centre = n // 2
    x0 = np.nan_to_num(S[centre], nan=0.5)
    for ename, ex in exclude_variants(n, centre).items():
        for bname, (lb, ub) in bounds_variants(d).items():
            rc, jobs, outs = raw_box(ctx, [db], [lb], [ub], [x0], [ex], np.inf, zero, d)
            assert rc == 0, ctx.lib.mrbf_last_error(ctx.h)
            check_box(ctx, jobs[0], outs[0], S, lb, ub, x0, ex, np.inf, zero, (d, n, ename, bname, zero))
    rc, jobs, outs = raw_box(ctx, [db], [np.full(d, -1.0)], [np.full(d, 1.0)], [x0], [[]], np.inf, zero, d)
    assert rc == 0 and 10 < jobs[0].mc < n              # the scan tells rows apart: some in the box, some out
    db.free()


def test_growth_keeps_every_row(ctx):
    """test 2: hint 4, appends of 3, 3 and 300 rows (host arrays, a device tensor, unevaluated rows), then set_values: mrbf_db_read of
    the whole database equals the host copy bit for bit after every step; the handle count is back where it was after free"""
    d, k = 5, 3
    live = ctx.get_option(_lib.OPT_LIVE_HANDLES)
    rng = np.random.default_rng(5)
    db = database.DeviceDatabase(d, k, ctx=ctx, capacity=4)
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live + 1
    S_all, V_all = np.empty((0, d)), np.empty((0, k))

    def step(S, V, device=False):
        nonlocal S_all, V_all
        first = db.append(torch.tensor(S, device="cuda") if device else S,
                          None if V is None else (torch.tensor(V, device="cuda") if device else V))
        assert first == len(S_all)
        S_all = np.vstack([S_all, S])
        V_all = np.vstack([V_all, np.full((len(S), k), np.nan) if V is None else V])
        check()

    def check():
        Sd, Vd = db.read()
        assert db.dims() == (len(S_all), d, k) and len(db) == len(S_all)
        assert same_bits(Sd, S_all) and same_bits(Vd, V_all)            # (NaN rows: the quiet NaN of np.nan, bit for bit)
        assert same_bits(db.sites, S_all) and same_bits(db.values, V_all)

    step(rng.standard_normal((3, d)), rng.standard_normal((3, k)))
    step(rng.standard_normal((3, d)), None)                               # beyond the hint: the first growth
    step(rng.standard_normal((300, d)), rng.standard_normal((300, k)), device=True)
    step(rng.standard_normal((7, d)), None, device=True)
    missing = [3, 4, 5, 311, 306, 312]                                    # (some unevaluated rows, in any order)
    vals = rng.standard_normal((len(missing), k))
    db.set_values(missing, vals)
    V_all[missing] = vals
    check()
    Sd, Vd = db.read(300, 13)
    assert same_bits(Sd, S_all[300:313]) and same_bits(Vd, V_all[300:313])
    assert ctx.lib.mrbf_db_set_values(ctx.h, db.h, 1, _lib.as_ptr(np.array([313], dtype=np.int64)), _lib.as_ptr(vals)) == -4
    check()
    db.free()
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live


def test_gather(ctx):
    """test 3: shuffled index lists with repeats; a job with an index out of range sets its own rc and leaves its outputs untouched
    while the other jobs of the call are right; a database named twice is an invalid `jobs`"""
    d = 65
    rng = np.random.default_rng(6)
    sizes, ks = (B + 1, 3 * B + 7, 9), (1, 2, 5)
    dbs, Ss, Vs = [], [], []
    for n, k in zip(sizes, ks):
        S, V = rng.standard_normal((n, d)), rng.standard_normal((n, k))
        db = database.DeviceDatabase(d, k, ctx=ctx)
        db.append(S, V)
        dbs.append(db), Ss.append(S), Vs.append(V)
    lists = [np.concatenate([rng.permutation(n), rng.integers(0, n, 11)]).astype(np.int64) for n in sizes]
    lists[2] = np.array([3, 8, 9, 0], dtype=np.int64)                     # 9 is not a row of the third database
    jobs = (_lib.DbGatherJob * 3)()
    outs = []
    for q in range(3):
        so, vo = np.full((len(lists[q]), d), SENTINEL), np.full((len(lists[q]), ks[q]), SENTINEL)
        outs.append((so, vo))
        J = jobs[q]
        J.db, J.n_idx, J.indices, J.sites_out, J.values_out = dbs[q].h, len(lists[q]), lists[q].ctypes.data, so.ctypes.data, vo.ctypes.data
        J.rc, J.sites_dev, J.values_dev = 55, 0x10, 0x20
    assert ctx.lib.mrbf_db_gather_batch(ctx.h, 3, d, jobs, None) == 0
    for q in range(2):
        assert jobs[q].rc == 0
        assert same_bits(outs[q][0], Ss[q][lists[q]]) and same_bits(outs[q][1], Vs[q][lists[q]])
    assert jobs[2].rc == -3 and jobs[2].sites_dev == 0x10 and jobs[2].values_dev == 0x20
    assert np.all(outs[2][0] == SENTINEL) and np.all(outs[2][1] == SENTINEL)
    # the Python mirror: views whose host side is the host copy, rc per start
    got = database.gather_many(dbs, lists, ctx=ctx)
    assert [g.rc for g in got] == [0, 0, -3] and got[2].sites is None
    assert same_bits(view_to_host(ctx, got[1].sites.data_ptr(), len(lists[1]), d), Ss[1][lists[1]]) and same_bits(np.asarray(got[1].values), Vs[1][lists[1]])
    # a database twice in one call
    jobs[2].db, jobs[2].n_idx = dbs[0].h, 2
    assert ctx.lib.mrbf_db_gather_batch(ctx.h, 3, d, jobs, None) == -4
    bj = (_lib.DbBoxJob * 2)()
    lb, ub, row = np.full(d, -1.0), np.full(d, 1.0), np.empty(d)
    for J in bj:
        J.db, J.lb, J.ub, J.x0, J.first_row, J.mc = dbs[1].h, lb.ctypes.data, ub.ctypes.data, lb.ctypes.data, row.ctypes.data, -9
    assert ctx.lib.mrbf_db_box_batch(ctx.h, 2, d, 1, bj, None) == -5 and bj[0].mc == -9
    for db in dbs:
        db.free()


def test_gather_at_the_widest_row(ctx):
    """test 3 at d = 4096: a shuffled index list with repeats out of B + 1 rows"""
    d, n, k = 4096, B + 1, 2
    rng = np.random.default_rng(4096)
    S, V = rng.standard_normal((n, d)), rng.standard_normal((n, k))
    db = database.DeviceDatabase(d, k, ctx=ctx)
    db.append(S, V)
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, 11)]).astype(np.int64)
    so, vo = np.full((len(idx) + 1, d), SENTINEL), np.full((len(idx) + 1, k), SENTINEL)
    jobs = (_lib.DbGatherJob * 1)()
    J = jobs[0]
    J.db, J.n_idx, J.indices, J.sites_out, J.values_out, J.rc = db.h, len(idx), idx.ctypes.data, so.ctypes.data, vo.ctypes.data, 55
    assert ctx.lib.mrbf_db_gather_batch(ctx.h, 1, d, jobs, None) == 0 and J.rc == 0
    assert same_bits(so[:-1], S[idx]) and same_bits(vo[:-1], V[idx]) and np.all(so[-1] == SENTINEL) and np.all(vo[-1] == SENTINEL)
    assert same_bits(view_to_host(ctx, J.sites_dev, len(idx), d), S[idx])
    db.free()


def test_optional_outputs_may_be_device_memory(ctx):
    """sites_out / shifted_out of the scan and sites_out / values_out of the gather as device pointers: the same bits as on the host"""
    d, n = 65, 3 * B + 7
    S = grid_sites(n, d, 77)
    V = np.random.default_rng(8).standard_normal((n, 2))
    db = database.DeviceDatabase(d, 2, ctx=ctx)
    db.append(S, V)
    lb, ub, x0 = np.full(d, -1.0), np.full(d, 1.0), np.zeros(d)
    idx, sites, shifted, pick, first = reference(S, lb, ub, x0, [], np.inf, True)
    so = torch.full((n, d), SENTINEL, dtype=torch.float64, device="cuda")
    ho = torch.full((n, d), SENTINEL, dtype=torch.float64, device="cuda")
    row = np.empty(d)
    jobs = (_lib.DbBoxJob * 1)()
    J = jobs[0]
    J.db, J.lb, J.ub, J.x0, J.zero_first_pick = db.h, lb.ctypes.data, ub.ctypes.data, x0.ctypes.data, 1
    J.sites_out, J.shifted_out, J.first_row = so.data_ptr(), ho.data_ptr(), row.ctypes.data
    assert ctx.lib.mrbf_db_box_batch(ctx.h, 1, d, 1, jobs, None) == 0 and J.rc == 0 and J.mc == len(idx) > 0
    assert same_bits(so.cpu().numpy()[: J.mc], sites) and same_bits(ho.cpu().numpy()[: J.mc], shifted)
    assert np.all(so.cpu().numpy()[J.mc:] == SENTINEL) and J.first_pick == pick and same_bits(row, first)
    lst = np.array([5, 0, 5, n - 1], dtype=np.int64)
    gs = torch.empty((4, d), dtype=torch.float64, device="cuda")
    gv = torch.empty((4, 2), dtype=torch.float64, device="cuda")
    gj = (_lib.DbGatherJob * 1)()
    gj[0].db, gj[0].n_idx, gj[0].indices, gj[0].sites_out, gj[0].values_out = db.h, 4, lst.ctypes.data, gs.data_ptr(), gv.data_ptr()
    assert ctx.lib.mrbf_db_gather_batch(ctx.h, 1, d, gj, None) == 0 and gj[0].rc == 0
    assert same_bits(gs.cpu().numpy(), S[lst]) and same_bits(gv.cpu().numpy(), V[lst])
    db.free()


# ---- tests 4 and 5: three starts at (d, n_db) = (3, 40), (65, 300), (65, 140), sites in [-2, 2]^d (the bounded-conditioning setting of
# tests/test_gpu_fit_batch.py), package-default kernel shapes
STARTS = ((3, 40), (65, 300), (65, 140))
K_OUT = 2


def start_database(d, n, seed, steps=None):
    """row 0 the centre (the origin), rows 1 .. steps (default d) the centre + a unit step each (affinely independent), the rest uniform
    in [-2, 2]^d, except that every tenth row from row d + 1 on is a small vector with one coordinate at 3/2 (and, with `steps`, rows in
    the span of the unit steps)"""
    rng = np.random.default_rng(seed)
    S = rng.uniform(-2.0, 2.0, (n, d))
    S[0] = 0.0
    for i in range(min(d if steps is None else steps, n - 1)):
        S[1 + i] = 0.02 * rng.standard_normal(d)
        S[1 + i, i] += 1.0 if i % 2 == 0 else -1.0
    for i in range(d + 1, n, 10):
        S[i] *= 0.15
        S[i, (3 * i) % d] = 1.5
    if steps is not None:     # every fifth row (offset 2) lies in the span of the unit steps, inside the inner box: candidates, not picks
        for i in range(d + 3, n, 5):
            S[i, :steps] = rng.uniform(-1.0, 1.0, steps)
            S[i, steps:] = 0.0
    return S


def objectives(S):
    S = np.asarray(S, dtype=np.float64).reshape(-1, S.shape[-1])
    return np.ascontiguousarray(np.stack([np.sum((S - 1.0) ** 2, axis=1), np.sum((S + 1.0) ** 2, axis=1) + S[:, 0]], axis=1)[:, :K_OUT])


@pytest.fixture(scope="module")
def three_starts(ctx):
    Ss = [start_database(d, n, 40 + p) for p, (d, n) in enumerate(STARTS)]
    dbs = []
    for S in Ss:
        dbs.append(database.DeviceDatabase(S.shape[1], K_OUT, ctx=ctx))
        dbs[-1].append(S, objectives(S))
    yield Ss, dbs
    for db in dbs:
        db.free()


def by_d():
    groups = {}
    for p, (d, _) in enumerate(STARTS):
        groups.setdefault(d, []).append(p)
    return groups


def test_views_feed_the_affine_filter_unchanged(ctx, three_starts):
    """test 4: mrbf_affine_select_batch on shifted_dev returns the picks and the Z_out bits it returns on the host array"""
    Ss, dbs = three_starts
    for d, members in by_d().items():
        lb, ub, x0 = np.full(d, -2.0), np.full(d, 2.0), np.zeros(d)
        boxes = database.box_many([dbs[p] for p in members], [lb] * len(members), [ub] * len(members), [x0] * len(members),
                                  [[0]] * len(members), ctx=ctx)
        items_view, items_host = [], []
        for B_, p in zip(boxes, members):
            idx, _, shifted, pick, first = reference(Ss[p], lb, ub, x0, [0], np.inf, True)
            assert B_.indices == idx and B_.first_pick == pick and B_.mc > d
            qr = sampling._GrowingQR(d)
            qr.append(first)
            items_view.append((B_.shifted, qr, d - 1, 0.25))
            items_host.append((shifted, qr, d - 1, 0.25))
        rc_v, res_v, _ = sampling.affine_select_batch_device(items_view, d, ctx=ctx)
        rc_h, res_h, _ = sampling.affine_select_batch_device(items_host, d, ctx=ctx)
        assert rc_v == 0 and rc_h == 0
        for (got_v, Z_v), (got_h, Z_h) in zip(res_v, res_h):
            assert got_v == got_h and len(got_v) >= 1 and same_bits(Z_v, Z_h)


def test_views_feed_round4_and_the_fit_unchanged(ctx, three_starts):
    """test 4: mrbf_round4_batch on a gather view (start sites) and a box view (candidates), both alive at once, returns the accepted
    lists it returns on host arrays; mrbf_fit_batch on gathered sites_dev / values_dev returns the same weights, tail coefficients,
    info.path and the same mrbf_eval values at 70 queries"""
    Ss, dbs = three_starts
    cfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    for d, members in by_d().items():
        ns = len(members)
        lb, ub, x0 = np.full(d, -2.0), np.full(d, 2.0), np.zeros(d)
        found = list(range(d + 1))
        boxes = database.box_many([dbs[p] for p in members], [lb] * ns, [ub] * ns, [x0] * ns, [found] * ns, zero_first_pick=False, ctx=ctx)
        starts = database.gather_many([dbs[p] for p in members], [found] * ns, ctx=ctx)
        for B_, g, p in zip(boxes, starts, members):
            assert g.rc == 0 and B_.indices == sampling.results_in_box_indices(Ss[p], lb, ub, found) and B_.mc > 10
        rc_v, res_v, _ = sampling.rbf_round4_batch_device([(cfg, g.sites, B_.sites, 1.0) for g, B_ in zip(starts, boxes)], d, ctx=ctx)
        rc_h, res_h, _ = sampling.rbf_round4_batch_device([(cfg, Ss[p][found], Ss[p][B_.indices], 1.0) for p, B_ in zip(members, boxes)], d, ctx=ctx)
        assert rc_v == 0 and rc_h == 0 and res_v == res_h
        assert all(rc_p == 0 and len(acc) > 5 for rc_p, acc in res_v)
        train = [found + [B_.indices[a] for a in acc] for B_, (_, acc) in zip(boxes, res_v)]
        # the fit: gathered views against host arrays
        sets = database.gather_many([dbs[p] for p in members], train, ctx=ctx)
        st_v, st_h = {}, {}
        mods_v = pkg.rbf_model.update_models_many(cfg, [g.sites for g in sets], [g.values for g in sets], 1.0, ctx=ctx, stats=st_v)
        mods_h = pkg.rbf_model.update_models_many(cfg, [Ss[p][t] for p, t in zip(members, train)],
                                                  [objectives(Ss[p][t]) for p, t in zip(members, train)], 1.0, ctx=ctx, stats=st_h)
        assert st_v["path"] == st_h["path"] == "batch" and st_v["status"] == st_h["status"] == [0] * ns
        X = np.random.default_rng(4242 + d).uniform(-2.0, 2.0, (70, d))
        for mv, mh in zip(mods_v, mods_h):
            assert same_bits(mv.weights, mh.weights) and same_bits(mv.poly, mh.poly) and mv.info["path"] == mh.info["path"]
            assert same_bits(mv.eval_sites(X)[0], mh.eval_sites(X)[0])
            mv.free(), mh.free()


def test_three_iterations_resident_against_host(ctx):
    """test 5: three iterations of phase I + fit -- rounds 1 and 2, round-3 sites appended unevaluated then set_values, round 4, fit --
    through the resident twins and through the host-array drivers: index lists, Y / Z, accepted lists and model coefficients are
    identical at every iteration.  The databases are laid out so that every round has work to do (asserted at the end): the inner box
    (radius 1.1) holds the unit steps, which span d - 30 directions at d = 65, and rows in their span (more candidates than directions
    at n_db = 300: that start's filter runs on the device, the other two on the host, as the decision table says); the middle box (radius 1.6) adds the few rows with a
    coordinate at 3/2 for round 2; round 3 has to supply the rest; the outer box (radius 3) gives round 4 everything else."""
    ns = len(STARTS)
    Ss = [start_database(d, n, 50 + p, steps=max(1, d - 30)) for p, (d, n) in enumerate(STARTS)]
    cfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    host = [S.copy() for S in Ss]
    hvals = [objectives(S) for S in Ss]
    dbs = []
    for S in Ss:
        dbs.append(database.DeviceDatabase(S.shape[1], K_OUT, ctx=ctx, capacity=8))
        dbs[-1].append(S, objectives(S))
    x_idx = [0] * ns
    piv1, piv2 = 0.25, 0.25
    round2_picks = round3_sites = 0
    for it in range(3):
        xs = [host[p][x_idx[p]].copy() for p in range(ns)]
        lb1, ub1 = [x - 1.1 for x in xs], [x + 1.1 for x in xs]
        lb2, ub2 = [x - 1.6 for x in xs], [x + 1.6 for x in xs]
        lb4, ub4 = [x - 3.0 for x in xs], [x + 3.0 for x in xs]
        # ---- round 1
        s1, s2 = {}, {}
        r1h = sampling.find_suitable_points_many(host, lb1, ub1, xs, x_idx, piv1, stats=s1, ctx=ctx)
        r1r = sampling.find_suitable_points_many(dbs, lb1, ub1, xs, x_idx, piv1, stats=s2, ctx=ctx)
        assert s1 == s2, (s1, s2)
        same_rounds(r1h, r1r, ("round 1", it))
        print("iteration %d round 1: %r, picks %r" % (it, s1, [len(r[0]) for r in r1h]))
        if it == 0:
            assert s1["path"] == "batch" and 1 in s1["batched"], s1    # the start with 300 sites: its pick loop ran on the device
        # ---- round 2: the larger box without what round 1 inspected, from round 1's Y and Z
        missing = [xs[p].size - len(r1h[p][0]) for p in range(ns)]
        inspected = [r1h[p][2] for p in range(ns)]
        Ys, Zs = [r[3] for r in r1h], [r[4] for r in r1h]
        todo = [p for p in range(ns) if missing[p] > 0]
        found = [[x_idx[p]] + list(r1h[p][0]) for p in range(ns)]
        dirs = {p: r1h[p][1] for p in range(ns)}
        if todo:
            s1, s2 = {}, {}
            sel = lambda seq: [seq[p] for p in todo]
            r2h = sampling.find_suitable_points_many(sel(host), sel(lb2), sel(ub2), sel(xs), sel(x_idx), piv2, sel(inspected), sel(Ys), sel(Zs),
                                                     sel(missing), stats=s1, ctx=ctx)
            r2r = sampling.find_suitable_points_many(sel(dbs), sel(lb2), sel(ub2), sel(xs), sel(x_idx), piv2, sel(inspected), sel(Ys),
                                                         sel(Zs), sel(missing), stats=s2, ctx=ctx)
            assert s1 == s2, (s1, s2)
            same_rounds(r2h, r2r, ("round 2", it))
            for pos, p in enumerate(todo):
                found[p] += list(r2h[pos][0])
                missing[p] -= len(r2h[pos][0])
                dirs[p] = r2h[pos][1]
                round2_picks += len(r2h[pos][0])
        # ---- round 3: a new site along every improving direction still missing, appended unevaluated, then evaluated
        for p in range(ns):
            if missing[p] <= 0:
                continue
            new = np.array([xs[p] + 1.0 * dirs[p][j] for j in range(missing[p])])
            first = dbs[p].append(new)                      # unevaluated
            assert first == len(host[p])
            ids = list(range(first, first + len(new)))
            host[p], hvals[p] = np.vstack([host[p], new]), np.vstack([hvals[p], np.full((len(new), K_OUT), np.nan)])
            assert same_bits(dbs[p].read()[1], hvals[p])
            dbs[p].set_values(ids, objectives(new))
            hvals[p][ids] = objectives(new)
            found[p] += ids
            round3_sites += len(new)
        for p in range(ns):
            Sd, Vd = dbs[p].read()
            assert same_bits(Sd, host[p]) and same_bits(Vd, hvals[p])
            assert len(found[p]) == xs[p].size + 1
        # ---- round 4
        s1, s2 = {}, {}
        a4h = sampling.rbf_round4_many(host, lb4, ub4, xs, 1.0, found, cfg, ctx=ctx, stats=s1, min_starts=1)
        a4r = sampling.rbf_round4_many(dbs, lb4, ub4, xs, 1.0, found, cfg, ctx=ctx, stats=s2, min_starts=1)
        assert a4h == a4r and s1 == s2 and s1["path"] == "batch" and s1["fallback"] == [], (it, s1, s2)
        # ---- fit
        train = [found[p] + a4h[p] for p in range(ns)]
        s1, s2 = {}, {}
        mh = pkg.rbf_model.update_models_many(cfg, [host[p][train[p]] for p in range(ns)], [hvals[p][train[p]] for p in range(ns)], 1.0,
                                              ctx=ctx, stats=s1)
        mr = pkg.rbf_model.update_models_resident(cfg, dbs, train, 1.0, ctx=ctx, stats=s2)
        assert s1["path"] == s2["path"] == "batch" and s1["status"] == s2["status"] == [0] * ns
        for p in range(ns):
            assert same_bits(mh[p].weights, mr[p].weights) and same_bits(mh[p].poly, mr[p].poly), (it, p)
            assert mh[p].info["path"] == mr[p].info["path"]
        # ---- the next iterate: a new evaluated site next to the centre becomes the centre
        for p in range(ns):
            step = np.full((1, xs[p].size), 0.05 * (it + 1))
            new = xs[p][None, :] + step
            x_idx[p] = dbs[p].append(new, objectives(new))
            host[p], hvals[p] = np.vstack([host[p], new]), np.vstack([hvals[p], objectives(new)])
            mh[p].free(), mr[p].free()
    print("round-2 picks %d, round-3 sites %d" % (round2_picks, round3_sites))
    assert round2_picks > 0 and round3_sites > 0
    for db in dbs:
        db.free()


def same_rounds(a, b, tag):
    assert len(a) == len(b)
    for p, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0] and ra[2] == rb[2], (tag, p, ra[0], rb[0])
        assert len(ra[1]) == len(rb[1]) and all(same_bits(u, v) for u, v in zip(ra[1], rb[1])), (tag, p)
        assert same_bits(ra[3], rb[3]) and same_bits(ra[4], rb[4]), (tag, p)


@pytest.mark.parametrize("n_starts,d", [(0, 3), (2, 4097), (65536, 3), (2, 0)])
def test_refused_shapes(ctx, n_starts, d):
    """test 6: -2, and nothing has been written to the jobs"""
    assert ctx.lib.mrbf_dispatch_db_batch(n_starts, d) == _lib.DISPATCH_REFERENCE
    for Job, call in ((_lib.DbBoxJob, lambda j: ctx.lib.mrbf_db_box_batch(ctx.h, n_starts, d, 1, j, None)),
                      (_lib.DbGatherJob, lambda j: ctx.lib.mrbf_db_gather_batch(ctx.h, n_starts, d, j, None))):
        jobs = (Job * 2)()
        ctypes.memset(jobs, 0x5A, ctypes.sizeof(jobs))
        before = bytes(jobs)
        assert call(jobs) == -2
        assert bytes(jobs) == before
    assert ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DB_BOX, -2) == 1 and ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DB_GATHER, -2) == 1
