"""The host scaffold the seven batched selection calls share (run with -m gpu): mrbf_affine_select_batch, mrbf_round4_batch,
mrbf_db_box_batch, mrbf_db_gather_batch, mrbf_db_append_batch, mrbf_db_set_values_batch and mrbf_db_round3_batch through the raw ABI at
3 starts, d = 8, on databases of 5 / 64 / 65 rows (below, at and above one 64-row block of the database kernels).  What the calls compute
is the business of their own test files; here every comparison is between two runs of the same call that must not differ: with and
without ms_total, with host arrays and with device pointers wherever the job struct allows one, a batch against its halves, a batch
with a start that takes the single call against the batch without it.  No tolerance: integers, and the bits of every double."""
import ctypes

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, database
    from tests import round4_batch_util as u

D, K = 8, 2
ROWS = (5, 64, 65)
SENTINEL = -777.25


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


def make_dbs(ctx):
    """three resident databases with sites on the grid of step 1/8 in [0, 1]^d; the same bits at every call"""
    rng = np.random.default_rng(11)
    dbs = []
    for n in ROWS:
        db = database.DeviceDatabase(D, K, ctx=ctx)
        db.append(rng.integers(0, 9, (n, D)) / 8.0, rng.uniform(-1, 1, (n, K)))
        dbs.append(db)
    return dbs


def free(dbs):
    for db in dbs:
        db.free()


def rows_of(ctx, db, n):
    S, V = np.empty((n, D)), np.empty((n, K))
    ctx.check(ctx.lib.mrbf_db_read(ctx.h, db.h, 0, n, _lib.as_ptr(S), _lib.as_ptr(V)))
    return S, V


def place(a, device):
    """the array itself, or a device copy of it"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).cuda() if device else a


def room(shape, device):
    a = np.full(shape, SENTINEL)
    return torch.from_numpy(a).cuda() if device else a


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def timer(timed):
    ms = ctypes.c_float(-1.0)
    return ms, (ctypes.byref(ms) if timed else None)


def same(a, b):
    """two results of one call: the same integers, the same bits in every array"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            same(x, y)
        elif isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype
            assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
        else:
            assert x == y


def variants(run, has_device=True):
    """untimed on host arrays is the reference; timed on host arrays and timed on device pointers must repeat it, with a time"""
    ref, _ = run(False, False)
    for device in (False, True) if has_device else (False,):
        got, ms = run(True, device)
        same(ref, got)
        assert ms > 0.0
    return ref


# ------------------------------------------------------------------------------------------------------------------ the database calls
def run_box(ctx, dbs, timed, device):
    jobs = (_lib.DbBoxJob * 3)()
    keep = []
    for p, db in enumerate(dbs):
        n = ROWS[p]
        x0 = np.full(D, 0.5)
        bufs = dict(lb=x0 - 0.375, ub=x0 + 0.375, x0=x0, ex=np.array([0, 3, 3, 10 ** 6], dtype=np.int64), idx=np.full(n, -1, dtype=np.int64),
                    first=np.full(D, SENTINEL), sites=room((n, D), device), shifted=room((n, D), device))
        keep.append(bufs)
        J = jobs[p]
        J.db, J.lb, J.ub, J.x0 = db.h, _lib.as_ptr(bufs["lb"]), _lib.as_ptr(bufs["ub"]), _lib.as_ptr(bufs["x0"])
        J.n_exclude, J.exclude, J.zero_first_pick = 4, _lib.as_ptr(bufs["ex"]), 1
        J.indices_out, J.sites_out, J.shifted_out = _lib.as_ptr(bufs["idx"]), _lib.as_ptr(bufs["sites"]), _lib.as_ptr(bufs["shifted"])
        J.first_row = _lib.as_ptr(bufs["first"])
    ms, arg = timer(timed)
    assert ctx.lib.mrbf_db_box_batch(ctx.h, 3, D, 1, jobs, arg) == 0
    res = []
    for p, b in enumerate(keep):
        assert jobs[p].rc == 0
        mc = int(jobs[p].mc)
        res.append((mc, int(jobs[p].first_pick), b["idx"][:mc].copy(), b["first"], host(b["sites"])[:mc].copy(), host(b["shifted"])[:mc].copy()))
    return res, ms.value


def test_box(ctx):
    dbs = make_dbs(ctx)
    ref = variants(lambda timed, device: run_box(ctx, dbs, timed, device))
    assert any(r[0] > 0 for r in ref) and all(r[0] < n for r, n in zip(ref, ROWS))  # (the box takes some rows and leaves some)
    free(dbs)


def run_gather(ctx, dbs, timed, device):
    jobs = (_lib.DbGatherJob * 3)()
    keep = []
    for p, db in enumerate(dbs):
        idx = np.array([ROWS[p] - 1, 0, 2, 0], dtype=np.int64)
        bufs = dict(idx=idx, sites=room((4, D), device), values=room((4, K), device))
        keep.append(bufs)
        J = jobs[p]
        J.db, J.n_idx, J.indices = db.h, 4, _lib.as_ptr(idx)
        J.sites_out, J.values_out = _lib.as_ptr(bufs["sites"]), _lib.as_ptr(bufs["values"])
    ms, arg = timer(timed)
    assert ctx.lib.mrbf_db_gather_batch(ctx.h, 3, D, jobs, arg) == 0
    assert all(jobs[p].rc == 0 for p in range(3))
    return [(host(b["sites"]).copy(), host(b["values"]).copy()) for b in keep], ms.value


def test_gather(ctx):
    dbs = make_dbs(ctx)
    ref = variants(lambda timed, device: run_gather(ctx, dbs, timed, device))
    for p, db in enumerate(dbs):  # (and the rows are the databases')
        S, V = rows_of(ctx, db, ROWS[p])
        same(ref[p], (S[[ROWS[p] - 1, 0, 2, 0]], V[[ROWS[p] - 1, 0, 2, 0]]))
    free(dbs)


def run_append(ctx, timed, device):
    dbs = make_dbs(ctx)
    rng = np.random.default_rng(12)
    jobs = (_lib.DbAppendJob * 3)()
    keep = []
    for p, db in enumerate(dbs):
        S, V = place(rng.uniform(0, 1, (3, D)), device), place(rng.uniform(-1, 1, (3, K)), device)
        keep.append((S, V))
        jobs[p].db, jobs[p].m, jobs[p].sites = db.h, 3, _lib.as_ptr(S)
        jobs[p].values = None if p == 1 else _lib.as_ptr(V)  # (start 1: unevaluated rows)
    ms, arg = timer(timed)
    assert ctx.lib.mrbf_db_append_batch(ctx.h, 3, jobs, arg) == 0
    res = [(int(jobs[p].rc), int(jobs[p].first_index)) + rows_of(ctx, db, ROWS[p] + 3) for p, db in enumerate(dbs)]
    free(dbs)
    return res, ms.value


def test_append(ctx):
    ref = variants(lambda timed, device: run_append(ctx, timed, device))
    assert [r[:2] for r in ref] == [(0, n) for n in ROWS]
    assert np.isnan(ref[1][3][ROWS[1]:]).all() and not np.isnan(ref[0][3]).any()


def run_set_values(ctx, timed, device):
    dbs = make_dbs(ctx)
    rng = np.random.default_rng(13)
    jobs = (_lib.DbSetValuesJob * 3)()
    keep = []
    for p, db in enumerate(dbs):
        idx, V = np.array([ROWS[p] - 1, 0], dtype=np.int64), place(rng.uniform(-1, 1, (2, K)), device)
        keep.append((idx, V))
        jobs[p].db, jobs[p].m, jobs[p].indices, jobs[p].values = db.h, 2, _lib.as_ptr(idx), _lib.as_ptr(V)
    ms, arg = timer(timed)
    assert ctx.lib.mrbf_db_set_values_batch(ctx.h, 3, jobs, arg) == 0
    res = [(int(jobs[p].rc),) + rows_of(ctx, db, ROWS[p]) for p, db in enumerate(dbs)]
    free(dbs)
    return res, ms.value


def test_set_values(ctx):
    ref = variants(lambda timed, device: run_set_values(ctx, timed, device))
    assert [r[0] for r in ref] == [0, 0, 0]


def run_round3(ctx, timed, device):
    dbs = make_dbs(ctx)
    rng = np.random.default_rng(14)
    jobs = (_lib.Round3Job * 3)()
    keep = []
    x = np.full(D, 0.5)
    for p, db in enumerate(dbs):
        dirs = place(np.linalg.qr(rng.normal(size=(D, 4)))[0].T, device)  # 4 directions: the rows are the columns of the d x 4 matrix
        bufs = dict(x=x, lb=x - 0.25, ub=x + 0.25, dirs=dirs, out=np.full((D, D), SENTINEL))
        keep.append(bufs)
        J = jobs[p]
        J.db, J.x, J.lb, J.ub, J.pivot_val = db.h, _lib.as_ptr(bufs["x"]), _lib.as_ptr(bufs["lb"]), _lib.as_ptr(bufs["ub"]), 1.0 / 64
        J.max_new, J.new_sites_out = 10, _lib.as_ptr(bufs["out"])
        if p == 1:    # the axes, all d of them
            J.dirs, J.n_dirs, J.n_missing, J.ensure_fully_linear = None, 0, D, 1
        else:         # an update along three of four directions, last first; an improvement step
            J.dirs, J.n_dirs, J.n_missing, J.reversed, J.mode = _lib.as_ptr(dirs), 4, 3, 1, (0 if p == 0 else 1)
    ms, arg = timer(timed)
    assert ctx.lib.mrbf_db_round3_batch(ctx.h, 3, D, jobs, arg) == 0
    res = []
    for p, db in enumerate(dbs):
        J = jobs[p]
        res.append((int(J.rc), int(J.n_new), int(J.fully_linear), int(J.status), int(J.n_dirs_used), int(J.first_index),
                    keep[p]["out"][: J.n_new].copy()) + rows_of(ctx, db, ROWS[p] + J.n_new))
    free(dbs)
    return res, ms.value


def test_round3(ctx):
    ref = variants(lambda timed, device: run_round3(ctx, timed, device))
    assert [r[:2] for r in ref] == [(0, 3), (0, D), (0, 1)]


# ------------------------------------------------------------------------------------------------------------------- the affine batch
def run_affine(ctx, d, starts, timed, device):
    """starts: (shifted rows, j0, Q0 as the rows of its transpose or None, max_picks) -> per start (n_picked, picks, Z as stored)"""
    n = len(starts)
    jobs = (_lib.AffineJob * n)()
    keep = []
    for p, (S, j0, Q0, max_picks) in enumerate(starts):
        bufs = dict(S=place(S, device), Q0=None if Q0 is None else place(Q0, device), picks=np.full(max(max_picks, 1), -1, dtype=np.int64),
                    Z=room((d, d), device))
        keep.append(bufs)
        J = jobs[p]
        J.mc, J.j0, J.max_picks, J.pivot_val = S.shape[0], j0, max_picks, 1e-3
        J.shifted, J.Q0, J.picked_out, J.Z_out = _lib.as_ptr(bufs["S"]), _lib.as_ptr(bufs["Q0"]), _lib.as_ptr(bufs["picks"]), _lib.as_ptr(bufs["Z"])
    ms, arg = timer(timed)
    assert ctx.lib.mrbf_affine_select_batch(ctx.h, n, d, 1, jobs, arg) == 0
    res = []
    for p, b in enumerate(keep):
        got = int(jobs[p].n_picked)
        res.append((got, b["picks"][:got].copy(), host(b["Z"]).reshape(-1)[: d * (d - starts[p][1] - got)].copy()))
    return res, ms.value


def test_affine(ctx):
    dbs = make_dbs(ctx)
    rng = np.random.default_rng(15)
    Q = np.linalg.qr(rng.normal(size=(D, 1)), mode="complete")[0]  # one direction chosen already: its full Q
    starts = []
    for p, db in enumerate(dbs):
        S = rows_of(ctx, db, ROWS[p])[0] - 0.5
        starts.append((S, 1, np.ascontiguousarray(Q.T), D) if p == 1 else (S, 0, None, D))
    ref = variants(lambda timed, device: run_affine(ctx, D, starts, timed, device))
    assert [r[0] for r in ref] == [min(ROWS[0], D), D - 1, D]  # (generic rows: every start picks all it may)
    free(dbs)


def test_affine_pageable_upload_and_batch_composition(ctx):
    """64 starts, d = 96, j0 = 0, 4 candidates each: the start bases alone are 64 x 96 x 96 x 8 B = 4.5 MiB, beyond the 4 MiB a host
    block may take of the pinned area, so the upload goes from pageable memory; the same starts in two calls of 32 upload from the
    pinned block.  "They do not depend on the start's position in the batch or on which other starts share it" (include/mrbf.h)."""
    d, n = 96, 64
    assert n * d * d * 8 > 4 << 20 >= (n // 2) * d * d * 8
    rng = np.random.default_rng(16)
    starts = [(rng.uniform(-1, 1, (4, d)), 0, None, 4) for _ in range(n)]
    whole, _ = run_affine(ctx, d, starts, True, False)
    first, _ = run_affine(ctx, d, starts[:32], True, False)
    second, _ = run_affine(ctx, d, starts[32:], False, False)
    same(whole, first + second)
    assert all(r[0] == 4 for r in whole)


# ------------------------------------------------------------------------------------------------------------------ the round-4 batch
def run_round4(ctx, starts, timed, device):
    """starts: (start sites, candidates, poly_deg) with the cubic kernel -> per start (rc, accepted positions)"""
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel="cubic", polynomial_degree=1))
    n = len(starts)
    jobs = (_lib.Round4Job * n)()
    keep = []
    for p, (C0, Xc, deg) in enumerate(starts):
        bufs = dict(C0=place(C0, device), Xc=place(Xc, device), acc=np.full(Xc.shape[0], -1, dtype=np.int32))
        keep.append(bufs)
        J = jobs[p]
        J.n0, J.mc, J.start_sites, J.cand_sites = C0.shape[0], Xc.shape[0], _lib.as_ptr(bufs["C0"]), _lib.as_ptr(bufs["Xc"])
        J.kernel_id, J.poly_deg, J.a, J.b, J.max_points, J.theta_pivot_cholesky = kid, deg, a, b, 0, 1e-7
        J.accepted_out = _lib.as_ptr(bufs["acc"])
    ms, arg = timer(timed)
    assert ctx.lib.mrbf_round4_batch(ctx.h, n, D, jobs, arg) == 0
    return [(int(jobs[p].rc), keep[p]["acc"][: jobs[p].n_accepted].copy()) for p in range(n)], ms.value


def test_round4(ctx):
    starts = [u.random_case(20 + p, D, D + 1, mc) + (1,) for p, mc in enumerate(ROWS)]
    ref = variants(lambda timed, device: run_round4(ctx, starts, timed, device))
    cap = (D + 1) * (D + 2) // 2 - (D + 1)
    assert [(rc, len(acc)) for rc, acc in ref] == [(0, min(mc, cap)) for mc in ROWS]


def test_round4_single_start_between_batched_ones(ctx):
    """a start with n0 < q is routed to mrbf_round4 inside the call, behind the batched chain: the batched starts' lists are those of the
    call without it, and the start carries mrbf_round4's own return code (which that call gives before it touches the pinned block:
    the ordering of guard and copy-out is the next test's business)"""
    C0, Xc = u.random_case(30, D, 5, 64)  # 5 start sites, a tail of 9 terms
    batched = [u.random_case(20 + p, D, D + 1, mc) + (1,) for p, mc in ((0, 64), (2, 65))]
    ref = variants(lambda timed, device: run_round4(ctx, [batched[0], (C0, Xc, 1), batched[1]], timed, device))
    alone, _ = run_round4(ctx, batched, True, False)
    same([ref[0], ref[2]], alone)
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel="cubic", polynomial_degree=1))
    acc, nacc = np.zeros(64, dtype=np.int32), ctypes.c_int32()
    rc = ctx.lib.mrbf_round4(ctx.h, 5, D, _lib.as_ptr(C0), 64, _lib.as_ptr(Xc), kid, a, b, 1, 0, 1e-7, _lib.as_ptr(acc), ctypes.byref(nacc), None)
    assert rc != 0 and ref[1][0] == rc and len(ref[1][1]) == 0
    assert all(r[0] == 0 and len(r[1]) > 0 for r in alone)


def test_round4_single_start_that_runs_between_batched_ones(ctx):
    """a start of 4097 candidates is beyond the small range (mc <= 4096) and really runs mrbf_round4 inside the call, which arms the
    pinned block again and stages through it: the chain's read-back must have been copied out of the block and the guard released
    before.  The batched starts' lists are those of the call without it; its own list is the one mrbf_round4 returns alone."""
    C0, Xc = u.random_case(31, D, D + 1, 4097)
    batched = [u.random_case(20 + p, D, D + 1, mc) + (1,) for p, mc in ((0, 64), (2, 65))]
    ref = variants(lambda timed, device: run_round4(ctx, [batched[0], (C0, Xc, 1), batched[1]], timed, device))
    alone, _ = run_round4(ctx, batched, True, False)
    same([ref[0], ref[2]], alone)
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel="cubic", polynomial_degree=1))
    acc, nacc = np.full(4097, -1, dtype=np.int32), ctypes.c_int32()
    rc = ctx.lib.mrbf_round4(ctx.h, D + 1, D, _lib.as_ptr(C0), 4097, _lib.as_ptr(Xc), kid, a, b, 1, 0, 1e-7, _lib.as_ptr(acc), ctypes.byref(nacc), None)
    assert rc == 0 and nacc.value == (D + 1) * (D + 2) // 2 - (D + 1)
    same([ref[1]], [(0, acc[: nacc.value].copy())])
