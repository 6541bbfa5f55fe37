"""CPU checks of tests/select_wide_util.py (no GPU): every case of the wide site-selection tests meets the conditions that
tests/test_gpu_select_wide.py rests on -- at every pick the reference's best score exceeds the runner-up by >= 1e-8 relative, at every
scan it is >= 1e-6 relative away from the pivot (conditions, not measurements: a seed that misses them is replaced, the numbers stay)
-- and reaches the form and thread layout it is there for; the from-scratch pick loop equals the independent oracle and the host
mirror's growing factorisation at d = 5 and 33; the extended-precision score agrees with mpmath; and the checker has teeth: a NumPy
restatement of the fused kernel's score step passes, the same with the last of the two chunks of dr = 512 left out of the sum does not."""
import numpy as np
import pytest

from morbit.jl_amd import sampling
from oracle import sampling_oracle as so
from tests import select_wide_util as u

# name: form, (dr, nch), picks of the reference, columns of the final Z
EXPECT = {
    "C1": ("fused", (256, 4), 129, 0), "C2": ("fused", (256, 4), 26, 0), "C3": ("fused", (256, 4), 20, 236),
    "C4": ("fused", (512, 2), 75, 182), "C5": ("fused", (1024, 1), 18, 495), "C6": ("fused", (1024, 1), 23, 0),
    "C7": ("fused", (1024, 1), 18, 1005), "C8": ("fused", (1024, 1), 23, 0), "C9": ("three", None, 29, 0),
    "C10": ("three", None, 30, 0), "C11": ("three", None, 20, 0), "C12": ("three", None, 3, 1021),
    "C13": ("rocblas", None, 20, 0), "C14": ("fused", (512, 2), 18, 282),
}


def test_every_case_is_listed():
    assert sorted(EXPECT) == sorted(u.CASES)


@pytest.mark.parametrize("name", sorted(u.CASES, key=lambda s: int(s[1:])))
def test_case_meets_the_conditions(name):
    case, r = u.select_case(name), u.select_case(name).ref
    form, layout, picks, dz = EXPECT[name]
    print(name, "picks", len(r.picks), "smallest gap %.3e" % min(r.gap), "smallest distance from the pivot %.3e" % min(r.pivot_distance),
          "best scores %.3e .. %.3e, pivot %.3e" % (min(r.best), max(r.best), case.pivot))
    assert case.form == form and (layout is None or case.layout == layout)
    assert case.mc > 8 and case.mc % 8 != 0 and len(r.picks) == picks and (picks > 16 or name == "C12")
    assert r.Z.shape == (case.d, dz) and len(set(r.picks)) == picks
    assert min(r.gap) >= u.GAP_MIN, (name, int(np.argmin(r.gap)), min(r.gap))
    assert min(r.pivot_distance) >= u.PIVOT_MIN, (name, int(np.argmin(r.pivot_distance)), min(r.pivot_distance))
    # a scan stopped the loop (rather than max_picks or the end of the complement) exactly where the case says so
    assert (len(r.pivot_distance) == picks + 1) == (name in ("C4", "C14"))
    if dz:
        # the Z bound is attainable in fp64: the host mirror's growing factorisation meets it with room
        ez = float(np.abs(u.mirror_Z(case.Y0, case.S, r.picks, case.p) - r.Z).max())
        print(name, "host mirror's Z against the reference:", ez)
        assert np.abs(u._norms(r.Z, case.p) - 1.0).max() < 1e-14 and ez <= 0.01 * u.Z_BOUND, (name, ez)


def test_c14_stops_at_the_pivot_beyond_the_first_look():
    case = u.select_case("C14")
    probe = u.pick_loop(case.S, case.Y0, u.C14_PICKS + 1, u.PIVOT, case.p)
    assert probe.picks[:u.C14_PICKS] == case.ref.picks and len(probe.picks) == u.C14_PICKS + 1
    assert min(probe.best[:u.C14_PICKS]) > case.pivot > probe.best[u.C14_PICKS] and u.C14_PICKS > 16


def _mirror_loop(S, Y0, max_picks, pivot, p):
    """the same rule on the host mirror's growing factorisation (sampling._GrowingQR, one reflector per pick)"""
    S = S.copy()
    qr, picks = sampling._GrowingQR(S.shape[1], Y0), []
    while len(picks) < min(max_picks, S.shape[1] - Y0.shape[1]):
        Z = qr.complement(p)
        vals = u._norms(Z @ (Z.T @ S.T), p)
        i = int(np.argmax(vals))
        if not vals[i] > pivot:
            break
        picks.append(i)
        qr.append(S[i])
        S[i] = 0.0
    return picks, qr.complement(p)


@pytest.mark.parametrize("p", [np.inf, 2])
@pytest.mark.parametrize("d,mc,pivot", [(5, 16, 1e-3), (33, 100, 1e-3), (33, 20, 1e-3)])
def test_pick_loop_is_the_oracle_and_the_host_mirror(d, mc, pivot, p):
    S, _ = u.candidate_data(700 + d + mc, d, mc, 0)
    r = u.pick_loop(S, np.empty((d, 0)), d, pivot, p)
    assert min(r.gap) >= u.GAP_MIN and min(r.pivot_distance) >= u.PIVOT_MIN
    # the oracle's first pick is unconditional; it is the rule's whenever the first score exceeds the pivot
    assert r.best[0] > pivot
    idx, Y, Z = so.affinely_independent_indices(np.zeros(d), list(S), d, pivot, p=p)
    assert idx == r.picks and np.array_equal(Y, S[r.picks].T)
    assert Z.shape == r.Z.shape and (Z.size == 0 or np.abs(Z - r.Z).max() <= 0.01 * u.Z_BOUND)
    assert len(r.picks) == min(d, mc)
    picks, Zm = _mirror_loop(S, np.empty((d, 0)), d, pivot, p)
    assert picks == r.picks and (Zm.size == 0 or np.abs(Zm - r.Z).max() <= 0.01 * u.Z_BOUND)
    # continuing from given directions (no oracle: its first pick ignores them)
    S2, Y0 = u.candidate_data(800 + d + mc, d, mc, d // 3)
    r2 = u.pick_loop(S2, Y0, d, pivot, p)
    picks2, Zm2 = _mirror_loop(S2, Y0, d, pivot, p)
    assert picks2 == r2.picks and len(picks2) > 0 and (Zm2.size == 0 or np.abs(Zm2 - r2.Z).max() <= 0.01 * u.Z_BOUND)


@pytest.mark.parametrize("p", [np.inf, 2])
def test_score_reference_matches_mpmath(p):
    rng = np.random.default_rng(5)
    S, Z = rng.standard_normal((7, 20)), so.orthogonal_complement_matrix(rng.standard_normal((20, 14)), p)
    val, B = u.score_reference(S, Z, p)
    val_mp = u._score_reference_mp(S, Z, p)
    e = u.score_errors_over_bound(val.astype(np.float64), val_mp, B, 20, 6)
    f = u.score_errors_over_bound(u.plain_scores(Z, S, p), val, B, 20, 6)
    print("extended precision against mpmath (as doubles), fp64 NumPy against extended precision, error / bound:", e.max(), f.max())
    assert e.max() <= 0.05 and f.max() < 1.0 and np.all(B >= val.astype(np.float64) * (1 - 1e-12))
    # the checker's edges: a zero row must score exactly zero, a NaN is no pass
    edge = u.score_errors_over_bound(np.array([0.0, 1e-300, np.nan]), np.zeros(3, dtype=u.LD), np.array([0.0, 0.0, 1.0]), 20, 6)
    assert edge.tolist() == [0.0, np.inf, np.inf]


def _scan_after(case, n):
    """trailing columns and candidates after the reference's first n picks"""
    S = np.array(case.S)
    S[case.ref.picks[:n]] = 0.0
    return u.trailing_columns(np.hstack([case.Y0, case.S[case.ref.picks[:n]].T])), S


@pytest.mark.parametrize("name", ["C1", "C4", "C5", "C14"])
def test_fused_restatement_passes(name):
    case = u.select_case(name)
    for n in (0, 1, 17):
        Q2, S = _scan_after(case, n)
        ref, B = u.score_reference(S, Q2 / u._norms(Q2, case.p)[None, :], case.p)
        e = u.score_errors_over_bound(u.fused_scores(Q2, S), ref, B, case.d, Q2.shape[1])
        print(name, "scan", n, "restated fused score step, error / bound:", e.max())
        assert e.max() < 1.0, (name, n, e.max())
    got = u.pick_loop(case.S, case.Y0, case.max_picks, case.pivot, case.p, scores=u.fused_scores)
    assert got.picks == case.ref.picks


def test_checker_rejects_a_dropped_chunk():
    case = u.select_case("C4")
    assert case.layout == (512, 2)
    mutant = lambda Q2, S, p: u.fused_scores(Q2, S, p, drop_last_chunk_at_dr=512)   # noqa: E731
    worst = 0.0
    for n in (0, 1, 17):
        Q2, S = _scan_after(case, n)
        ref, B = u.score_reference(S, Q2 / u._norms(Q2, case.p)[None, :], case.p)
        worst = max(worst, u.score_errors_over_bound(mutant(Q2, S, case.p), ref, B, case.d, Q2.shape[1]).max())
    got = u.pick_loop(case.S, case.Y0, case.max_picks, case.pivot, case.p, scores=mutant)
    print("C4 with the second chunk dropped: score error / bound", worst, "picks:", len(got.picks), "first difference from the reference at pick",
          next((i for i, (a, b) in enumerate(zip(got.picks, case.ref.picks)) if a != b), None))
    assert got.picks != case.ref.picks or worst > 1.0
    assert got.picks != case.ref.picks and worst > 1.0     # (both, in fact: either alone fails the GPU test)
    # the mutation is the layout's: a case of another dr does not notice it
    c1 = u.select_case("C1")
    assert u.pick_loop(c1.S, c1.Y0, c1.max_picks, c1.pivot, c1.p, scores=mutant).picks == c1.ref.picks
