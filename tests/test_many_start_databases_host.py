"""CPU tests of the many-start drivers over database objects (`sampling.find_suitable_points_many`, `rbf_round4_many`,
`rbf_round3_append`, `prepare_update_models`): host databases and plain arrays of sites never ask for a context, the two job packers
take NumPy arrays and device views alike, and the databases of one call are of one kind.  No GPU: round 4's device calls are the
stand-ins of tests/test_round4_batch_host.py."""
import ctypes

import numpy as np
import pytest

from tests.test_round4_batch_host import _cfg, lib, stand_ins as round4_stand_ins  # noqa: F401  (fixtures)

D, NS, N_DB = 3, 2, 12


@pytest.fixture
def no_context(monkeypatch):
    from morbit.jl_amd import _lib

    def refuse(*a, **kw):
        raise AssertionError("a host-kind call asked for a context")

    monkeypatch.setattr(_lib, "default_context", refuse)


def _two_starts():
    """per start: row 0 the centre (1/2, 1/2, 1/2); rows 1, 2 inside the inner box (radius 1/4), affinely independent; row 3 repeats row
    1's direction; the other rows spread over [0, 1]^3 outside the inner box.  Every number is a multiple of 1/64."""
    rng = np.random.default_rng(12)
    Ss = []
    for p in range(NS):
        S = rng.integers(0, 13, (N_DB, D)) / 64.0
        S[4:, p % D] += 0.75                                   # outside the inner box
        S[0] = 0.5
        S[1] = S[0] + np.array([0.125 + p / 64.0, 0.0, 0.0])
        S[2] = S[0] + np.array([0.0625, -0.1875, 0.0])
        S[3] = S[0] + np.array([-0.0625 - p / 64.0, 0.0, 0.0])
        Ss.append(S)
    return Ss


def _kinds(Ss):
    """the same rows as plain arrays and as HostDatabases (values: the row sums)"""
    from morbit.jl_amd import database

    dbs = []
    for S in Ss:
        dbs.append(database.HostDatabase(D, 1))
        dbs[-1].append(S, S.sum(axis=1, keepdims=True))
    return (("arrays", [S.copy() for S in Ss]), ("HostDatabase", dbs))


def _same_find(got, want):
    assert got[0] == want[0] and got[2] == want[2] and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert len(got[1]) == len(want[1]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))


def test_host_kinds_run_without_a_context(lib, round4_stand_ins, no_context):
    from morbit.jl_amd import sampling
    from morbit.jl_amd.descent import _local_bounds

    Ss = _two_starts()
    xs, x_idx = [S[0].copy() for S in Ss], [0] * NS
    cfg = _cfg()
    delta, delta_max, lb, ub = 0.125, 0.5, np.zeros(D), np.ones(D)
    d1 = cfg.θ_enlarge_1 * delta
    piv = cfg.θ_pivot * d1
    box1 = [_local_bounds(x, d1, lb, ub) for x in xs]
    box2 = [_local_bounds(x, cfg.θ_enlarge_2 * delta_max, lb, ub) for x in xs]
    lb1, ub1, lb2, ub2 = [b[0] for b in box1], [b[1] for b in box1], [b[0] for b in box2], [b[1] for b in box2]
    # what the single functions give per start (`_rbf_round4` is the stand-in)
    w1 = [sampling._find_suitable_points(Ss[p], lb1[p], ub1[p], xs[p], 0, piv) for p in range(NS)]
    assert [sorted(w[0]) for w in w1] == [[1, 2], [1, 2]]                       # one direction is missing: round 3 has work
    w3 = [sampling._rbf_round3(None, lb1[p], ub1[p], xs[p], piv, w1[p][1], 10 ** 9, 1, True, False) for p in range(NS)]
    assert all(w[0] is not None and w[0].shape == (1, D) and w[1] for w in w3)  # no rebuild, fully linear
    grown = [np.vstack([Ss[p], w3[p][0]]) for p in range(NS)]
    found = [[0, *w1[p][0], N_DB] for p in range(NS)]
    w4 = [sampling._rbf_round4(grown[p], lb2[p], ub2[p], xs[p], delta, found[p], cfg) for p in range(NS)]
    assert all(len(w) > 0 for w in w4)
    for kind, dbs in _kinds(Ss):
        round4_stand_ins["batch"].clear(), round4_stand_ins["single"].clear()
        stats = {}
        r1 = sampling.find_suitable_points_many(dbs, lb1, ub1, xs, x_idx, piv, stats=stats)
        assert stats == {"path": "loop", "batched": []}, kind
        for p in range(NS):
            _same_find(r1[p], w1[p])
        r3 = sampling.rbf_round3_append(dbs, lb1, ub1, xs, piv, [r[1] for r in r1], 10 ** 9, 1, True, False, stats=stats)
        assert stats["path"] == "host", kind
        for p in range(NS):
            assert np.array_equal(r3[p].new_points, w3[p][0]) and r3[p].fully_linear is True and not r3[p].rebuilt, kind
            assert r3[p].indices == [N_DB] and len(r3[p].remaining_directions) == len(w3[p][2]) == 0, kind
        if kind == "HostDatabase":                                               # the new sites were appended, unevaluated
            assert all(np.array_equal(dbs[p].sites, grown[p]) and np.isnan(dbs[p].values[N_DB:]).all() for p in range(NS))
        r4 = sampling.rbf_round4_many(grown if kind == "arrays" else dbs, lb2, ub2, xs, delta, found, cfg, stats=stats, min_starts=1)
        assert r4 == w4 and stats == {"path": "batch", "batched": [0, 1], "fallback": []}, kind
        assert round4_stand_ins["batch"] == [[((4, D), (N_DB - 3, D))] * NS] and round4_stand_ins["single"] == [], kind
    # phase I as one driver: round 2 skipped (ensure_fully_linear), two starts take round 4's loop by the measured rule
    for kind, dbs in _kinds(Ss):
        metas = sampling.prepare_update_models(cfg, dbs, xs, x_idx, delta, delta_max, lb, ub, ensure_fully_linear=True)
        for p, m in enumerate(metas):
            assert {k: v for k, v in m.items() if k != "improving_directions"} == dict(
                center_index=0, round1_indices=w1[p][0], round2_indices=[], round3_indices=[N_DB], round4_indices=w4[p], fully_linear=True,
                rebuilt=False), (kind, p)
            assert m["improving_directions"] == [], (kind, p)
        if kind == "HostDatabase":
            assert all(np.array_equal(dbs[p].sites, grown[p]) for p in range(NS))
        else:
            assert all(S.shape == (N_DB, D) and np.array_equal(S, S0) for S, S0 in zip(dbs, Ss))     # the caller's arrays are only read


class _RecordingLib:
    """stands for ctx.lib: records what the packers put into the job array, accepts nothing"""

    def __init__(self):
        self.seen = []

    def _record(self, jobs, n, d, names):
        for k in range(n):
            row = {f: getattr(jobs[k], f) for f in names}
            for f in names[2:]:                                 # the memory behind the pointers, while the packer keeps it alive
                m = row[names[0] if f != "start_sites" else "n0"]
                row[f + "_rows"] = np.ctypeslib.as_array((ctypes.c_double * (m * d)).from_address(row[f])).reshape(m, d).copy()
            self.seen.append(row)

    def mrbf_affine_select_batch(self, h, n, d, p_is_inf, jobs, ms):
        self._record(jobs, n, d, ("mc", "j0", "shifted"))
        return 0

    def mrbf_round4_batch(self, h, n, d, jobs, ms):
        self._record(jobs, n, d, ("mc", "n0", "cand_sites", "start_sites"))
        return 0


class _RecordingCtx:
    h = None

    def __init__(self):
        self.lib = _RecordingLib()


def test_the_packers_take_arrays_and_views(no_context):
    from morbit.jl_amd import database, sampling

    rng = np.random.default_rng(3)
    d = 5
    wide = rng.random((9, 2 * d))
    Xc, C0 = np.ascontiguousarray(wide[:, :d]), rng.random((6, d))
    view = lambda A: database.DeviceView(A.ctypes.data, A.shape)
    strided = wide[:, ::2]                                      # the same shape, not contiguous
    assert strided.shape == Xc.shape and not strided.flags.c_contiguous
    qr = sampling._GrowingQR(d)
    qr.append(Xc[0].copy())
    ctx = _RecordingCtx()
    for S in (Xc, view(Xc), strided):
        rc, res, _ = sampling.affine_select_batch_device([(S, qr, d - 1, 0.25)], d, ctx=ctx)
        assert rc == 0 and res[0][0] == [] and res[0][1].shape == (d, d - 1)
    a, v, s = ctx.lib.seen
    assert (a["mc"], a["j0"], a["shifted"]) == (v["mc"], v["j0"], v["shifted"]) == (9, 1, Xc.ctypes.data)       # both read in place
    assert (s["mc"], s["j0"]) == (9, 1) and s["shifted"] != strided.ctypes.data and np.array_equal(s["shifted_rows"], strided)
    ctx = _RecordingCtx()
    for S0, S1 in ((C0, Xc), (view(C0), view(Xc)), (C0, strided)):
        rc, res, _ = sampling.rbf_round4_batch_device([(_cfg(), S0, S1, 1.0)], d, ctx=ctx)
        assert rc == 0 and res == [(0, [])]
    a, v, s = ctx.lib.seen
    assert (a["n0"], a["mc"], a["start_sites"], a["cand_sites"]) == (v["n0"], v["mc"], v["start_sites"], v["cand_sites"]) == \
        (6, 9, C0.ctypes.data, Xc.ctypes.data)
    assert (s["n0"], s["mc"], s["start_sites"]) == (6, 9, C0.ctypes.data)
    assert s["cand_sites"] != strided.ctypes.data and np.array_equal(s["cand_sites_rows"], strided)


def test_mixed_kinds_are_refused(lib, no_context, monkeypatch):
    from morbit.jl_amd import database, sampling

    Ss = _two_starts()
    host = database.HostDatabase(D, 1)
    host.append(Ss[0], Ss[0].sum(axis=1, keepdims=True))
    resident = database.HostDatabase.__new__(database.DeviceDatabase)           # a resident database's host side: no device is asked
    resident.__dict__.update(host.__dict__, h=None, ctx=None)
    for name in ("mrbf_db_box_batch", "mrbf_db_gather_batch", "mrbf_db_round3_batch", "mrbf_db_append_batch", "mrbf_db_set_values_batch",
                 "mrbf_affine_select_batch", "mrbf_round4_batch"):
        monkeypatch.setattr(lib, name, lambda *a, name=name: pytest.fail("library call %s" % name))
    dbs, xs = [host, resident], [Ss[0][0].copy()] * 2
    lbs, ubs = [x - 0.25 for x in xs], [x + 0.25 for x in xs]
    mixed = "all resident or all on the host"
    with pytest.raises(AssertionError, match=mixed):
        sampling.find_suitable_points_many(dbs, lbs, ubs, xs, [0, 0], 0.0625)
    with pytest.raises(AssertionError, match=mixed):
        sampling.rbf_round4_many(dbs, lbs, ubs, xs, 1.0, [[0, 1, 2, 3]] * 2, _cfg(), min_starts=1)
    with pytest.raises(AssertionError, match=mixed):
        sampling.rbf_round3_append(dbs, lbs, ubs, xs, 0.0625, [None, None], 10 ** 9, 1)
    with pytest.raises(AssertionError, match=mixed):
        sampling.prepare_update_models(_cfg(), dbs, xs, [0, 0], 0.125, 0.5, np.zeros(D), np.ones(D))
    with pytest.raises(AssertionError, match=mixed):
        database.box_many(dbs, lbs, ubs, xs, [[0], [0]])
    with pytest.raises(AssertionError, match=mixed):
        database.gather_many(dbs, [[0], [0]])
    with pytest.raises(AssertionError, match=mixed):
        database.append_many(dbs, [Ss[0][:1]] * 2)
    with pytest.raises(AssertionError, match=mixed):
        database.set_values_many(dbs, [[0], [0]], [np.zeros((1, 1))] * 2)
    assert len(host) == len(resident) == N_DB
