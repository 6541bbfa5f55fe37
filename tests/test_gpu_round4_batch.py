"""mrbf_round4_batch on the device: per start the accepted list is the one mrbf_round4 returns and the one
oracle/sampling_oracle.py::rbf_round4 returns, whatever the start's place in the batch.  Every input meets the margin condition of
tests/round4_batch_util.py (no decision within a factor 100 of the threshold, checked with the oracle alone on the CPU); at least half
of the cases use theta in 0.1 .. 0.2 on clustered candidates, and between a quarter and three quarters of their decisions are
rejections (asserted on the oracle's output)."""
import ctypes
import importlib

import numpy as np
import pytest

import morbit  # noqa: F401  (registers morbit.jl_amd)

pkg = importlib.import_module("morbit.jl_amd")
from morbit.jl_amd import _lib
from tests import round4_batch_util as u

sampling = pkg.sampling
BIG = 10 ** 6   # max_points that the candidates never reach


class Start:
    """one start of a batch: sites, configuration, and (computed once, cached by key) what the oracle says"""

    def __init__(self, key, kernel, deg, theta, mp, C0, Xc, full_oracle=True):
        self.key, self.kernel, self.deg, self.theta, self.mp, self.C0, self.Xc, self.full_oracle = key, kernel, deg, theta, mp, C0, Xc, full_oracle
        self.cfg = pkg.RbfConfig(kernel=kernel, polynomial_degree=deg, max_model_points=mp, θ_pivot_cholesky=theta)

    def item(self):
        return (self.cfg, self.C0, self.Xc, 1.0)

    def expected(self):
        return u.oracle_case(self.key, self.C0, self.Xc, self.kernel, self.deg, self.theta, self.mp, self.full_oracle)


def clustered(key, kernel, deg, d, n0, mc, theta, seed, scale=10.0, mp=BIG, copies=2, eps=1e-5, full_oracle=True):
    C0, Xc = u.clustered_case(seed, d, n0, mc, scale=scale, eps=eps, copies=copies)
    return Start(key, kernel, deg, theta, mp, C0, Xc, full_oracle)


def generic(key, kernel, deg, d, n0, mc, seed, scale=1.0, mp=BIG, theta=1e-7, full_oracle=True):
    C0, Xc = u.random_case(seed, d, n0, mc, scale=scale)
    return Start(key, kernel, deg, theta, mp, C0, Xc, full_oracle)


def run_batch(starts, d):
    rc, res, ms = sampling.rbf_round4_batch_device([s.item() for s in starts], d)
    assert rc == 0
    return res


def single(start):
    return sampling.rbf_round4_device(start.cfg, start.C0, start.Xc, 1.0)


def check(starts, d, rejecting=()):
    """batch == oracle == mrbf_round4 per start; `rejecting`: positions whose share of rejections must lie in [1/4, 3/4]"""
    res = run_batch(starts, d)
    for p, s in enumerate(starts):
        want, share = s.expected()
        if p in rejecting:
            assert 0.25 <= share <= 0.75, (s.key, share)
        assert res[p] == (0, want), (s.key, res[p], want)
        assert single(s) == want, s.key
    return res


# the shapes of tests/test_sampling.py's CASES: (kernel, degree, d, sites), as batches of three seeds.  Four of the five with
# rejections; the thin plate spline (k = 2, not conditionally positive definite with a degree-1 tail outside small boxes) with the
# default theta in a box of edge 1/2.
KERNEL_CASES = [("cubic", 1, 3, 60, 0.2, 10.0, (0, 1, 2)), ("gaussian", 1, 2, 40, 0.1, 10.0, (0, 1, 2)),
                ("multiquadric", 1, 4, 80, 0.2, 10.0, (0, 1, 2)), ("inv_multiquadric", 0, 3, 50, 0.1, 10.0, (0, 1, 2)),
                ("thin_plate_spline", 1, 2, 30, 1e-7, 0.5, (1, 4, 7))]


def kernel_case(name, deg, d, n, theta, scale, seeds):
    n0 = d + 1
    if theta < 1e-3:
        return [generic(("kernel", name, sd), name, deg, d, n0, n - n0, sd, scale=scale) for sd in seeds]
    return [clustered(("kernel", name, sd), name, deg, d, n0, n - n0, theta, sd, scale=scale) for sd in seeds]


@pytest.mark.gpu
@pytest.mark.parametrize("name,deg,d,n,theta,scale,seeds", KERNEL_CASES)
def test_all_five_kernels(name, deg, d, n, theta, scale, seeds):
    starts = kernel_case(name, deg, d, n, theta, scale, seeds)
    check(starts, d, rejecting=range(3) if theta > 1e-3 else ())


def candidate_count_case():
    """mc at the edges of any 64-wide tiling, and one start without candidates"""
    starts = [clustered(("count", mc), "cubic", 1, 3, 4, mc, 0.2, 10 + mc, scale=10.0 if mc < 100 else 40.0, eps=1e-5 if mc < 100 else 1e-8, full_oracle=mc < 200) for mc in (1, 63, 64, 65, 129, 257)]
    starts.insert(3, Start(("count", 0), "cubic", 1, 0.2, BIG, starts[0].C0, np.empty((0, 3))))
    return starts


@pytest.mark.gpu
def test_candidate_counts():
    starts = candidate_count_case()
    res = check(starts, 3, rejecting=(1, 2, 4, 5, 6))
    assert res[3] == (0, []) and [len(s.Xc) for s in starts] == [1, 63, 64, 0, 65, 129, 257]


def max_points_case():
    a = clustered(("mp", "middle"), "multiquadric", 1, 4, 5, 60, 0.2, 3, mp=5 + 7)          # reached in the middle of the candidates
    b = clustered(("mp", "full"), "multiquadric", 1, 4, 5, 60, 0.2, 3, mp=5)                # max_points = n0: nothing accepted
    c = clustered(("mp", "default"), "cubic", 1, 4, 5, 60, 0.2, 5, mp=-1)                   # the default rule: (d+1)(d+2)/2 = 15
    e = generic(("mp", "default0"), "gaussian", 1, 4, 5, 60, 6, mp=0)
    return [a, b, c, e]


@pytest.mark.gpu
def test_reaching_max_points():
    starts = max_points_case()
    res = check(starts, 4)
    assert [len(r[1]) for r in res] == [7, 0, 10, 10]
    assert res[0][1][-1] < 59          # the walk stopped before the last candidate


def duplicate_case():
    C0, Xc = u.random_case(21, 3, 4, 12, scale=10.0)
    Xc[4] = C0[2]         # a candidate equal to a start site
    Xc[9] = Xc[1]         # a candidate equal to an earlier (accepted) candidate
    return [Start(("dup", k), k, 1, 0.2, BIG, C0, Xc) for k in ("cubic", "multiquadric")]


@pytest.mark.gpu
def test_duplicates_are_rejected():
    starts = duplicate_case()
    res = check(starts, 3)
    for rc, acc in res:
        assert 1 in acc and 4 not in acc and 9 not in acc


def benchmark_shape_case():
    return [generic(("bench", sd), "cubic", 1, 128, 129, 300, 40 + sd, mp=257, full_oracle=False) for sd in range(4)]


@pytest.mark.gpu
def test_benchmark_shape_once():
    starts = benchmark_shape_case()
    res = check(starts, 128)
    assert all(len(acc) == 128 for _, acc in res)


def beyond_small_range_case():
    return [generic(("d130", sd), "cubic", 1, 130, 131 + sd, (37, 24, 12)[sd], 60 + sd) for sd in range(3)]


@pytest.mark.gpu
def test_every_start_beyond_the_small_range():
    """d = 130 > 128: no start fits the batched kernel, mrbf_round4 runs inside the call for each: rc 0 per start, the lists of the single
    calls and of the oracle"""
    starts = beyond_small_range_case()
    res = check(starts, 130)
    assert [len(acc) for _, acc in res] == [37, 24, 12]
    assert run_batch(starts[::-1], 130) == res[::-1]


def ragged_case():
    return [clustered(("rag", 0), "cubic", 1, 3, 4, 40, 0.2, 31),
            generic(("rag", 1), "gaussian", 0, 3, 6, 17, 32, scale=10.0),
            clustered(("rag", 2), "multiquadric", 1, 3, 7, 90, 0.2, 33, scale=20.0),
            clustered(("rag", 3), "inv_multiquadric", -1, 3, 3, 33, 0.1, 34),
            generic(("rag", 4), "thin_plate_spline", 1, 3, 4, 9, 35, scale=0.5),
            clustered(("rag", 5), "gaussian", 1, 3, 4, 64, 0.1, 36, copies=3),
            generic(("rag", 6), "cubic", 1, 3, 9, 5, 37, mp=11),
            clustered(("rag", 7), "multiquadric", 0, 3, 2, 128, 0.2, 38, scale=40.0),
            Start(("rag", 8), "cubic", 1, 0.2, BIG, u.random_case(39, 3, 4, 1)[0], np.empty((0, 3)))]


@pytest.mark.gpu
def test_ragged_batch_and_position_independence():
    starts = ragged_case()
    res = check(starts, 3, rejecting=(0, 2, 3, 5, 7))
    perm = [4, 8, 0, 7, 2, 6, 1, 5, 3]
    again = run_batch([starts[p] for p in perm], 3)
    assert [again[perm.index(p)] for p in range(len(starts))] == res
    # alone, and next to one other start
    assert run_batch([starts[5]], 3) == [res[5]] and run_batch([starts[7], starts[5]], 3) == [res[7], res[5]]


def seventy_case():
    kern = ("cubic", "multiquadric", "gaussian")
    return [clustered(("seventy", p), kern[p % 3], 1, 5, 6, 16 + p % 5, (0.2, 0.2, 0.1)[p % 3], 100 + p) if p % 2 == 0 else
            generic(("seventy", p), kern[p % 3], 1, 5, 6, 16 + p % 5, 100 + p, scale=10.0) for p in range(70)]


@pytest.mark.gpu
def test_seventy_starts_against_the_loop():
    starts = seventy_case()
    res = run_batch(starts, 5)
    for p, s in enumerate(starts):
        want, share = s.expected()
        assert res[p] == (0, want), s.key
        if p % 2 == 0:
            assert 0.25 <= share <= 0.75, (s.key, share)
    assert [r[1] for r in res] == [single(s) for s in starts]


def out_of_range_case():
    big = generic(("oor", "big"), "cubic", 1, 3, 4, 5000, 51, mp=-1)                        # mc = 5000 > 4096: mrbf_round4 inside the call
    return [clustered(("oor", 0), "cubic", 1, 3, 4, 30, 0.2, 52), big, clustered(("oor", 2), "gaussian", 1, 3, 4, 30, 0.1, 53)]


@pytest.mark.gpu
def test_out_of_range_start_inside_a_batch():
    starts = out_of_range_case()
    res = check(starts, 3, rejecting=(0, 2))
    assert len(res[1][1]) == 6
    # the others give what they give without it
    assert run_batch([starts[0], starts[2]], 3) == [res[0], res[2]]
    # a start set that cannot carry the tail: its own rc, the others unaffected
    C0, Xc = u.random_case(54, 3, 2, 10)
    bad = Start(("oor", "tail"), "cubic", 1, 0.2, BIG, C0, Xc)
    rc, got, _ = sampling.rbf_round4_batch_device([starts[0].item(), bad.item(), starts[2].item()], 3)
    assert rc == 0 and got[1] == (-2, []) and [got[0], got[2]] == [res[0], res[2]]
    assert pkg.load().mrbf_dispatch_after(_lib.ENTRY_ROUND4_BATCH, -2) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n_starts,d", [(0, 3), (65536, 3), (2, 0), (2, 1025)])
def test_refusals(n_starts, d):
    ctx = pkg.default_context()
    jobs = (_lib.Round4Job * 2)()
    for J in jobs:
        J.n_accepted, J.rc = 77, 77
    assert ctx.lib.mrbf_dispatch_round4_batch(n_starts, d) == _lib.DISPATCH_REFERENCE
    assert ctx.lib.mrbf_round4_batch(ctx.h, n_starts, d, jobs, None) == -2
    assert all(J.n_accepted == 77 and J.rc == 77 for J in jobs)            # nothing is written
    assert ctx.lib.mrbf_dispatch_after(_lib.ENTRY_ROUND4_BATCH, -2) == 1


@pytest.mark.gpu
def test_invalid_job_field_is_an_invalid_jobs_argument():
    ctx = pkg.default_context()
    s = out_of_range_case()[0]
    for field, value in (("n0", 0), ("mc", -1), ("kernel_id", 5), ("poly_deg", 2), ("start_sites", None), ("accepted_out", None)):
        jobs = (_lib.Round4Job * 1)()
        acc = np.zeros(64, dtype=np.int32)
        J = jobs[0]
        J.n0, J.mc, J.start_sites, J.cand_sites = 4, 30, s.C0.ctypes.data, s.Xc.ctypes.data
        J.kernel_id, J.poly_deg, J.a, J.b, J.max_points, J.theta_pivot_cholesky, J.accepted_out = 0, 1, 3.0, 0.0, -1, 0.2, acc.ctypes.data
        setattr(J, field, value)
        assert ctx.lib.mrbf_round4_batch(ctx.h, 1, 3, jobs, None) == -4, field
    assert ctx.lib.mrbf_round4_batch(ctx.h, 1, 3, None, None) == -4


@pytest.mark.gpu
def test_no_state_is_left_behind():
    ctx = pkg.default_context()
    starts = ragged_case() + out_of_range_case()
    live = ctx.get_option(_lib.OPT_LIVE_HANDLES)
    first = run_batch(starts, 3)
    arena = ctx.get_option(_lib.OPT_ARENA_BYTES)
    assert run_batch(starts, 3) == first
    assert ctx.get_option(_lib.OPT_ARENA_BYTES) == arena
    assert ctx.get_option(_lib.OPT_LIVE_HANDLES) == live


@pytest.mark.gpu
def test_end_to_end_selection_then_model_update():
    """rbf_round4_many, then update_models_many on the selected sites, against _rbf_round4 and update_model per start"""
    d, ns = 4, 3
    rng = np.random.default_rng(77)
    cfgs = [pkg.RbfConfig(kernel=k, polynomial_degree=1, max_model_points=BIG, θ_pivot_cholesky=t)
            for k, t in (("cubic", 0.2), ("multiquadric", 0.2), ("gaussian", 0.1))]
    dbs, found = [], []
    for p in range(ns):
        C0, Xc = u.clustered_case(60 + p, d, d + 1, 40, scale=10.0)
        order = rng.permutation(len(C0) + len(Xc))
        db = np.vstack([C0, Xc])[order]
        dbs.append(db)
        found.append([int(np.where(order == i)[0][0]) for i in range(len(C0))])
    lb, ub, xs = [np.full(d, -1.0)] * ns, [np.full(d, 11.0)] * ns, [db[f[0]] for db, f in zip(dbs, found)]
    for p in range(ns):    # the inputs as the device sees them (start sites in `found` order, candidates in database order) are fit
        cand = sampling.results_in_box_indices(dbs[p], lb[p], ub[p], found[p])
        _, share = u.oracle_case(("e2e", p), dbs[p][found[p]], dbs[p][cand], cfgs[p].kernel, 1, cfgs[p].θ_pivot_cholesky, BIG)
        assert 0.25 <= share <= 0.75
    stats = {}
    many = sampling.rbf_round4_many(dbs, lb, ub, xs, 1.0, found, cfgs, stats=stats, min_starts=1)     # (three starts: the rule would take the loop)
    assert stats["path"] == "batch" and stats["batched"] == [0, 1, 2] and stats["fallback"] == []
    loop = [sampling._rbf_round4(dbs[p], lb[p], ub[p], xs[p], 1.0, found[p], cfgs[p]) for p in range(ns)]
    assert many == loop and all(len(m) > 5 for m in many)
    train = [found[p] + many[p] for p in range(ns)]
    vals = [np.stack([np.sum((db[t] - 1.0) ** 2, axis=1), np.sin(db[t].sum(axis=1))], axis=1) for db, t in zip(dbs, train)]
    mods = pkg.rbf_model.update_models_many(cfgs, [db[t] for db, t in zip(dbs, train)], vals, 1.0)
    X = rng.random((9, d)) * 10.0
    for p in range(ns):
        ref = pkg.update_model(cfgs[p], dbs[p][train[p]], vals[p])
        assert np.array_equal(mods[p].weights, ref.weights) and np.array_equal(mods[p].poly, ref.poly)
        assert np.array_equal(mods[p].eval_sites(X)[0], ref.eval_sites(X)[0])
        ref.free()
        mods[p].free()
