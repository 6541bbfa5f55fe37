"""GPU tests of mrbf_affine_select_batch: the pick loops of many filters in one call.  Every case compares the batched call with
mrbf_affine_select per start on the same context: the same number of picks, the same pick lists, Z_out equal bit for bit.  The sites
are random points of a box (seeded: no ties in the scores)."""
import ctypes

import numpy as np
import pytest

import morbit.jl_amd as pkg
from morbit.jl_amd import _lib, sampling

pytestmark = pytest.mark.gpu

I64P = ctypes.POINTER(ctypes.c_int64)


def _start(seed, d, mc, j0, pivot, max_picks=None):
    """one start: mc shifted candidates in a box, j0 directions chosen so far (Q0 from `_GrowingQR`, None with j0 = 0)"""
    rng = np.random.default_rng(seed)
    S = np.ascontiguousarray(0.1 * (2.0 * rng.random((mc, d)) - 1.0))
    Q0 = np.asfortranarray(sampling._GrowingQR(d, rng.standard_normal((d, j0))).Q) if j0 > 0 else None
    return dict(S=S, d=d, mc=mc, j0=j0, Q0=Q0, pivot=pivot, max_picks=d - j0 if max_picks is None else max_picks)


def _outputs(st):
    picks = np.full(max(st["max_picks"], 1), -7, dtype=np.int64)
    Z = np.full(st["d"] * max(st["d"] - st["j0"], 1), -7.0)
    return picks, Z


def _result(st, n, picks, Z):
    used = st["d"] * (st["d"] - st["j0"] - n)
    assert np.all(picks[n:] == -7) and np.all(Z[used:] == -7.0)          # nothing written beyond what was promised
    return n, picks[:n].copy(), Z[:used].copy()


def run_single(ctx, st, p_is_inf=1):
    picks, Z = _outputs(st)
    n = ctypes.c_int32(-7)
    ctx.check(ctx.lib.mrbf_affine_select(ctx.h, st["mc"], st["d"], _lib.as_ptr(st["S"]) if st["mc"] else None, st["j0"], _lib.as_ptr(st["Q0"]),
                                         st["max_picks"], st["pivot"], p_is_inf, picks.ctypes.data_as(I64P), ctypes.byref(n), _lib.as_ptr(Z)))
    return _result(st, n.value, picks, Z)


def run_batch(ctx, starts, p_is_inf=1, d=None, expect_rc=0):
    jobs = (_lib.AffineJob * len(starts))()
    outs = [_outputs(st) for st in starts]
    for jb, st, (picks, Z) in zip(jobs, starts, outs):
        jb.mc, jb.j0, jb.max_picks, jb.pivot_val = st["mc"], st["j0"], st["max_picks"], st["pivot"]
        jb.shifted = st["S"].ctypes.data if st["mc"] else None
        jb.Q0 = st["Q0"].ctypes.data if st["Q0"] is not None else None
        jb.picked_out, jb.Z_out, jb.n_picked = picks.ctypes.data, Z.ctypes.data, -7
    ms = ctypes.c_float(-1.0)
    rc = ctx.lib.mrbf_affine_select_batch(ctx.h, len(starts), starts[0]["d"] if d is None else d, p_is_inf, jobs, ctypes.byref(ms))
    assert rc == expect_rc, (rc, ctx.lib.mrbf_last_error(ctx.h))
    if rc != 0:
        return [(jb.n_picked, picks, Z) for jb, (picks, Z) in zip(jobs, outs)]
    assert ms.value > 0.0
    return [_result(st, jb.n_picked, picks, Z) for jb, st, (picks, Z) in zip(jobs, starts, outs)]


def same(got, want):
    assert got[0] == want[0], (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2])


@pytest.fixture(scope="module")
def ctx():
    return pkg.default_context()


# case 1: d = 33 pads the row count to 64; mc = 0, 1, 7, 8 (fewer candidates than a group, exactly one group), 203 (26 groups, the last one
# ragged); d - j0 = 28 > 16 picks for the last start: the loop crosses the host's look at the done words
def _ragged():
    return [_start(101, 33, 0, 0, 1e-3), _start(102, 33, 1, 5, 2e-3), _start(103, 33, 7, 11, 3e-3, max_picks=33), _start(104, 33, 8, 0, 4e-3),
            _start(105, 33, 203, 5, 5e-3, max_picks=40)]


@pytest.fixture(scope="module")
def ragged(ctx):
    starts = _ragged()
    return starts, [run_single(ctx, st) for st in starts]


def test_ragged_batch(ctx, ragged):
    starts, want = ragged
    got = run_batch(ctx, starts)
    for g, w in zip(got, want):
        same(g, w)
    # what the single calls found: every start short of candidates takes them all, the large one fills its complement
    assert [w[0] for w in want] == [0, 1, 7, 8, 28]


def test_different_lengths_of_loop(ctx):
    starts = [_start(201, 33, 150, 0, 1e-3, max_picks=2),        # plenty of good candidates, two wanted
              _start(202, 33, 150, 5, 1e6),                      # the pivot stops it after its first scan
              _start(203, 33, 150, 0, 1e-3)]                     # all d picks
    want = [run_single(ctx, st) for st in starts]
    got = run_batch(ctx, starts)
    for g, w in zip(got, want):
        same(g, w)
    assert [g[0] for g in got] == [2, 0, 33]
    assert got[0][2].size == 33 * 31 and got[1][2].size == 33 * 28 and got[2][2].size == 0


def test_position_independence(ctx, ragged):
    starts, want = ragged
    got = run_batch(ctx, starts[::-1])
    for g, w in zip(got, want[::-1]):
        same(g, w)
    same(run_batch(ctx, [starts[4]])[0], want[4])
    again = run_batch(ctx, starts[::-1])
    for g, a in zip(got, again):
        same(a, g)


def test_workload_dimension(ctx):
    starts = [_start(401, 128, 90, 0, 1e-3), _start(402, 128, 130, 7, 2e-3), _start(403, 128, 300, 0, 1e-3)]
    want = [run_single(ctx, st) for st in starts]
    got = run_batch(ctx, starts)
    for g, w in zip(got, want):
        same(g, w)
    assert [g[0] for g in got] == [90, 121, 128]


def test_many_groups_tiny_basis(ctx):
    starts = [_start(501, 7, 5000, 0, 1e-3), _start(502, 7, 5000, 2, 0.45)]
    want = [run_single(ctx, st) for st in starts]
    got = run_batch(ctx, starts)
    for g, w in zip(got, want):
        same(g, w)
    assert got[0][0] == 7


def test_refusals_launch_nothing(ctx):
    starts = [_start(601, 33, 40, 0, 1e-3), _start(602, 33, 40, 3, 1e-3)]
    for n, picks, Z in run_batch(ctx, starts, p_is_inf=0, expect_rc=-2):
        assert n == -7 and np.all(picks == -7) and np.all(Z == -7.0)
    wide = [dict(_start(603, 8, 4, 0, 1e-3), d=1024, S=np.zeros((4, 1024)), max_picks=3)]
    for n, picks, Z in run_batch(ctx, wide, d=1024, expect_rc=-2):
        assert n == -7 and np.all(picks == -7) and np.all(Z == -7.0)
    assert ctx.lib.mrbf_dispatch_after(_lib.ENTRY_AFFINE_BATCH, -2) == 1


# ---- case 7: end to end through find_suitable_points_many ------------------------------------------------------------------------------
def end_to_end_databases(d=33, seed=11):
    """three starts: the small box's sites span 10 / 14 / 18 directions only (round 1 stops at the pivot test), the large box's span all"""
    rng = np.random.default_rng(seed)
    dbs = []
    for p, rank in enumerate((10, 14, 18)):
        w = np.full(d, 1e-5)
        w[:rank] = 0.1
        dbs.append(np.vstack([np.full(d, 0.5), 0.5 + w * (2 * rng.random((1100 + 10 * p, d)) - 1), 0.5 + 0.3 * (2 * rng.random((1100, d)) - 1)]))
    return dbs


def host_filter_with_gaps(x, seeds, n, Y, Z, piv):
    """the host filter's loop (sampling.AffinelyIndependentPointFilter.collect, host branch) with, per decision, the distance of the top
    score from the runner-up -- and, at the scan that stops the loop, from the pivot -- relative to the top score"""
    flt = sampling.AffinelyIndependentPointFilter(x, seeds, n=n, Y=Y, Z=Z, pivot_val=piv)
    S = np.array(flt.shifted)
    first = np.sort(np.abs(S).max(axis=1))[::-1]
    gaps = [(first[0] - first[1]) / first[0]]
    out, qr, S, i, cand = flt._begin()
    while len(out) < flt.n and cand:
        vals = np.abs((S[cand] @ flt.Z) @ flt.Z.T).max(axis=1) if flt.Z.shape[1] else np.zeros(len(cand))
        order = np.argsort(-vals, kind="stable")
        top = vals[order[0]]
        if not top > piv:
            gaps.append(abs(top - piv) / max(top, piv))
            break
        gaps.append(min(top - vals[order[1]], top - piv) / top)
        best = cand[int(order[0])]
        flt._take(qr, best)
        cand.remove(best)
        out.append(best)
    return out, min(gaps)


def host_rounds(dbs, piv=0.02):
    """rounds 1 and 2 per start with the host filter forced -> (round-1 tuples, round-2 tuples, missing, smallest gap)"""
    lib = _lib.load()
    real = lib.mrbf_dispatch_affine
    r1, r2, missing, gap = [], [], [], np.inf
    try:
        lib.mrbf_dispatch_affine = lambda *a: _lib.DISPATCH_REFERENCE
        for db in dbs:
            x = db[0]
            a = sampling._find_suitable_points(db, x - 0.1, x + 0.1, x, 0, piv)
            m = x.size - len(a[0])
            b = sampling._find_suitable_points(db, x - 0.3, x + 0.3, x, 0, piv, already_inspected_indices=a[2], Y=a[3], Z=a[4], n_missing=m)
            # the same two filters once more with the gaps recorded; they must be the filters that just ran
            p1, g1 = host_filter_with_gaps(x, [db[i] for i in a[2]], x.size, None, None, piv)
            p2, g2 = host_filter_with_gaps(x, [db[i] for i in b[2]], m, a[3], a[4], piv)
            assert [a[2][i] for i in p1] == a[0] and [b[2][i] for i in p2] == b[0]
            r1.append(a), r2.append(b), missing.append(m)
            gap = min(gap, g1, g2)
    finally:
        lib.mrbf_dispatch_affine = real
    return r1, r2, missing, gap


def test_end_to_end_two_rounds(ctx):
    dbs = end_to_end_databases()
    w1, w2, missing, gap = host_rounds(dbs)
    # no decision of the host filter hangs on rounding: a different pick on the device would be a fault of the kernel, not a tie
    assert gap > 1e-7, gap
    assert missing == [23, 19, 15] and [len(w[0]) for w in w2] == missing
    xs = [db[0] for db in dbs]
    stats = {}
    r1 = sampling.find_suitable_points_many(dbs, [x - 0.1 for x in xs], [x + 0.1 for x in xs], xs, [0] * 3, 0.02, stats=stats, ctx=ctx)
    assert stats["path"] == "batch" and stats["batched"] == [0, 1, 2]
    stats = {}
    r2 = sampling.find_suitable_points_many(dbs, [x - 0.3 for x in xs], [x + 0.3 for x in xs], xs, [0] * 3, 0.02,
                                            already_inspected_indices=[r[2] for r in r1], Ys=[r[3] for r in r1], Zs=[r[4] for r in r1],
                                            n_missing=[x.size - len(r[0]) for x, r in zip(xs, r1)], stats=stats, ctx=ctx)
    assert stats["path"] == "batch" and stats["batched"] == [0, 1, 2]
    for got, want in ((r1, w1), (r2, w2)):
        for g, w in zip(got, want):
            assert g[0] == w[0] and g[2] == w[2] and np.array_equal(g[3], w[3])
            assert g[4].shape == w[4].shape and (g[4].size == 0 or np.abs(g[4] - w[4]).max() < 1e-10)
            assert len(g[1]) == len(w[1]) and all(np.abs(a - b).max() < 1e-10 for a, b in zip(g[1], w[1]))
