"""GPU tests of the site-selection kernels above 128 dimensions (cases, references and bounds: tests/select_wide_util.py; the
conditions they rest on are asserted on the CPU by tests/test_select_wide_reference.py).

mrbf_affine_select through the raw ABI at every form and thread layout the decision table can send a shape to -- the one-launch-per-pick
kernel at dr = 256, 512, 1024 up to its 128 KiB of LDS at d = 1023, the three-launch form in both norms up to d = 1024 (dz = 1024: 64 KiB
of dynamic LDS on top of 2 KiB static), the rocBLAS form at d = 1025: the number of picks and the pick list are the reference's (whose
best score leads the runner-up by >= 1e-8 and is >= 1e-6 away from the pivot at every scan, relative), nothing is written beyond what
was promised, Z_out is the reference's final Z to 1e-10 absolute on unit-p-norm columns.  mrbf_affine_select_batch at d = 129, 257, 513,
1023 equals the single calls bit for bit.  mrbf_affine_scores at d = 300, 1025, 4096 stays inside the derived bound
|val - ref| <= 2 (d + dz + 4) eps B_c of an extended-precision reference, and argmax / maxval are the first maximiser of vals_out.

The module writes select_wide_report.json -- per case the form taken, the picks, the reference's gaps and every measured distance -- into
the directory that MRBF_REPORT_DIR names (default: test_reports/ in the repository root, kept out of git)."""
import ctypes
import json
import os

import numpy as np
import pytest

import morbit.jl_amd as pkg
from morbit.jl_amd import _lib
from oracle import sampling_oracle as so
from tests import select_wide_util as u
from tests.conftest import ROOT
from tests.test_gpu_affine_batch import I64P, run_batch, run_single, same

pytestmark = pytest.mark.gpu

REPORT = {}


@pytest.fixture(scope="module")
def ctx():
    yield pkg.default_context()
    out = os.environ.get("MRBF_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "select_wide_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


_SINGLE = {}


def single(ctx, name):
    """the single call of a case: run once, shared with the batches"""
    if name not in _SINGLE:
        case = u.select_case(name)
        _SINGLE[name] = run_single(ctx, u.start_of(case), p_is_inf=case.p_is_inf)   # (asserts the -7 sentinels behind picks and Z)
    return _SINGLE[name]


@pytest.mark.parametrize("name", sorted(u.CASES, key=lambda s: int(s[1:])))
def test_affine_select_wide(ctx, name):
    case, r = u.select_case(name), u.select_case(name).ref
    rec = REPORT.setdefault("select", {}).setdefault(name, {})
    rec.update(d=case.d, mc=case.mc, j0=case.j0, max_picks=case.max_picks, norm="inf" if case.p_is_inf else "2", pivot=case.pivot, form=case.form,
               layout=list(case.layout) if case.form == "fused" else None, reference_picks=[int(i) for i in r.picks],
               reference_smallest_gap=float(min(r.gap)), reference_smallest_pivot_distance=float(min(r.pivot_distance)))
    n, picks, Z = single(ctx, name)
    rec.update(n_picked=int(n), picks=[int(i) for i in picks])
    assert n == len(r.picks), (name, n, len(r.picks))
    assert picks.tolist() == r.picks, (name, next(i for i, (a, b) in enumerate(zip(picks.tolist(), r.picks)) if a != b))
    dz = case.d - case.j0 - n
    assert Z.size == case.d * dz
    ez = float(np.abs(Z.reshape(dz, case.d).T - r.Z).max()) if dz else 0.0
    rec.update(z_columns=dz, z_distance=ez)
    print(name, json.dumps({k: v for k, v in rec.items() if "picks" not in k or k == "max_picks"}))
    if ez > u.Z_BOUND:   # whose bound is it?  the fp64 host mirror's own distance from the same reference
        rec["z_distance_host_mirror"] = float(np.abs(u.mirror_Z(case.Y0, case.S, r.picks, case.p) - r.Z).max())
        print(name, "host mirror:", rec["z_distance_host_mirror"])
    assert ez <= u.Z_BOUND, (name, ez)


# d: the cases of that d (their data in the inf-norm: the batch has no other), and one more start with another mc / j0
BATCHES = {
    129: (("C1", "C9"), dict(seed=9201, mc=9, j0=64, pivot=2e-3)),
    257: (("C4",), dict(seed=9202, mc=300, j0=250, pivot=2e-3)),
    513: (("C5", "C6"), dict(seed=9203, mc=100, j0=500, pivot=2e-3)),
    1023: (("C7", "C8"), dict(seed=9204, mc=12, j0=1019, pivot=2e-3)),
}


@pytest.mark.parametrize("d", sorted(BATCHES))
def test_affine_select_batch_wide(ctx, d):
    names, other = BATCHES[d]
    starts, want = [], []
    for name in names:
        case = u.select_case(name)
        assert case.d == d
        starts.append(u.start_of(case))
        want.append(single(ctx, name) if case.p_is_inf else run_single(ctx, starts[-1]))
    starts.append(u.other_start(d=d, **other))
    want.append(run_single(ctx, starts[-1]))
    if len(starts) < 3:   # the first case once more, wanting five picks only
        starts.append(dict(starts[0], max_picks=5))
        want.append(run_single(ctx, starts[-1]))
        assert want[-1][0] == 5 and np.array_equal(want[-1][1], want[0][1][:5])
    assert len(starts) == 3
    got = run_batch(ctx, starts)
    for g, w in zip(got, want):
        same(g, w)
    for g, w in zip(run_batch(ctx, starts[::-1]), want[::-1]):      # position in the batch does not matter
        same(g, w)
    assert all(w[0] > 0 for w in want)
    REPORT.setdefault("batch", {})[str(d)] = dict(starts=[dict(mc=st["mc"], j0=st["j0"], max_picks=st["max_picks"]) for st in starts],
                                                  n_picked=[int(w[0]) for w in want], equal_bit_for_bit=True)


_Q = {}


def _scores_case(mc, d, dz, p):
    """candidates with two identical maximal rows (at 3 and mc - 2) and Z = the orthogonal complement of a random block; the QR is
    taken once per shape (the 2-norm's Z: the same columns at unit 2-norm)"""
    rng = np.random.default_rng(4000 + d)
    S = np.ascontiguousarray(0.1 * (2.0 * rng.random((mc, d)) - 1.0))
    if (d, dz) not in _Q:
        _Q[d, dz] = so.orthogonal_complement_matrix(rng.standard_normal((d, d - dz)), np.inf)
    Z = _Q[d, dz]
    if not np.isinf(p):
        Z = Z / np.linalg.norm(Z, axis=0)[None, :]
    S[3] = 1.5 * S[int(np.argmax(u.plain_scores(Z, S, p)))]    # the largest score by half, twice
    S[mc - 2] = S[3]
    return S, np.asfortranarray(Z)


@pytest.mark.parametrize("p", [np.inf, 2])
@pytest.mark.parametrize("mc,d,dz", [(37, 300, 150), (21, 1025, 40), (9, 4096, 5)])
def test_affine_scores_wide(ctx, mc, d, dz, p):
    S, Z = _scores_case(mc, d, dz, p)
    ref, B = u.score_reference(S, Z, p)
    assert int(np.argmax(ref)) == 3 and ref[mc - 2] == ref[3] and np.sort(ref.astype(np.float64))[-3] < 0.9 * float(ref[3])
    vals = np.full(mc + 1, -7.0)
    best, val = ctypes.c_int64(-7), ctypes.c_double(-7.0)
    ctx.check(ctx.lib.mrbf_affine_scores(ctx.h, mc, d, dz, _lib.as_ptr(S), _lib.as_ptr(Z), 1 if np.isinf(p) else 0, _lib.as_ptr(vals),
                                         ctypes.byref(best), ctypes.byref(val)))
    assert vals[mc] == -7.0
    vals = vals[:mc]
    e = u.score_errors_over_bound(vals, ref, B, d, dz)
    rec = dict(mc=mc, d=d, dz=dz, norm="inf" if np.isinf(p) else "2", error_over_bound=float(e.max()), worst_candidate=int(e.argmax()),
               argmax=int(best.value), twins_equal=bool(vals[3] == vals[mc - 2]))
    REPORT.setdefault("scores", {})["%d_%d_%d_%s" % (mc, d, dz, rec["norm"])] = rec
    print(json.dumps(rec))
    assert e.max() < 1.0, rec
    # argmax / maxval: the first maximiser of what was returned; it is one of the twins, the first when their scores are equal
    assert best.value == int(np.argmax(vals)) and val.value == vals[best.value], rec
    assert best.value in (3, mc - 2) and (vals[3] != vals[mc - 2] or best.value == 3), rec


def test_refusal_beyond_4096_writes_nothing(ctx):
    d = 4097
    S = np.zeros((2, d))
    S[0, 0] = S[1, 1] = 1.0
    picks, Z, n = np.full(4, -7, dtype=np.int64), np.full(8, -7.0), ctypes.c_int32(-7)
    rc = ctx.lib.mrbf_affine_select(ctx.h, 2, d, _lib.as_ptr(S), 0, None, 2, 1e-3, 1, picks.ctypes.data_as(I64P), ctypes.byref(n), _lib.as_ptr(Z))
    assert rc == -3 and n.value == -7 and np.all(picks == -7) and np.all(Z == -7.0)
    vals, best, val = np.full(2, -7.0), ctypes.c_int64(-7), ctypes.c_double(-7.0)
    rc = ctx.lib.mrbf_affine_scores(ctx.h, 2, d, 0, _lib.as_ptr(S), None, 1, _lib.as_ptr(vals), ctypes.byref(best), ctypes.byref(val))
    assert rc == -3 and best.value == -7 and val.value == -7.0 and np.all(vals == -7.0)
    REPORT["refusal_d_4097"] = dict(select_rc=-3, scores_rc=-3)
