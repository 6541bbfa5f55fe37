"""Shared by tests/test_select_wide_reference.py and tests/test_gpu_select_wide.py (not a test module): the site-selection pick loop
above 128 dimensions -- the cases, a from-scratch reference of the loop, an extended-precision reference of one score scan, and a
NumPy restatement of the fused kernel's score step that the CPU test mutates.

The device code under test changes structure with d (morbit.jl_amd/csrc/affine.hip, `form_of`):
  fused    inf-norm, d <= 1023: one launch per pick, 1024 threads laid out as (row, chunk) with dr = the power of two >= d (at least
           64) and nch = 1024 / dr chunks of the trailing columns, summed in a fixed order; 8 (d + 1) + 8 * 1024 doubles of LDS
  three    2-norm at d <= 1024 and the inf-norm at d = 1024: score / decide / update launches per pick
  rocblas  d >= 1025: the two products by rocBLAS

Reference of the loop (`pick_loop`), with the semantics of mrbf_affine_select: from Y0 (d x j0) repeat up to max_picks times:
Z = the trailing columns of np.linalg.qr([Y0, picked rows], mode="complete") scaled to unit p-norm, val_c = |Z (Z' s_c)|_p, the first
maximiser is picked while it exceeds pivot_val, its row joins Y and is zeroed among the candidates.  A QR from scratch per pick is
independent of the growing factorisation under test, and LAPACK's reflectors are the ones the kernels state they follow.

Conditions the GPU test rests on (asserted by the CPU test for every case; conditions, not measurements -- the kernels' errors are near
1e-13 -- so a seed that misses them is replaced, not the numbers):
  GAP_MIN    1e-8  at every pick the best score exceeds the runner-up by at least this, relative to the best
  PIVOT_MIN  1e-6  at every scan the best score is at least this far from pivot_val, relative to the larger of the two
Bounds: Z_BOUND = 1e-10 absolute on unit-p-norm columns (the bound tests/test_sampling.py uses for the same comparison) and the
derived bound of one score (`score_bound`): |val - ref| <= 2 (d + dz + 4) eps B_c with B_c = | |Z| (|Z|' |s_c|) |_p -- the standard
gamma_d + gamma_dz + gamma_d gamma_dz of two nested inner products, valid for any summation order with or without FMA; the factor 2
covers the norm and the step from n eps to gamma_n; eps = 2^-52."""
from types import SimpleNamespace

import numpy as np

from morbit.jl_amd import sampling

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
GAP_MIN, PIVOT_MIN, Z_BOUND = 1e-8, 1e-6, 1e-10
PIVOT = 1e-3

# name: d, mc, j0, max_picks, p, seed  -- the smallest shapes that reach each form; candidate counts above 8 and no multiple of 8 (several
# workgroups, a ragged last one), pick counts above 16 (the host's look at the "done" word every sixteen launches is crossed)
CASES = {
    "C1": (129, 150, 0, 129, np.inf, 9101),     # first d of dr 256: rows 129..255 idle, the whole complement consumed
    "C2": (256, 75, 230, 26, np.inf, 9102),     # dr 256 full; short trailing block (dz <= 26)
    "C3": (256, 300, 0, 20, np.inf, 9103),      # dr 256, dz near d, 38 workgroups
    "C4": (257, 75, 0, 257, np.inf, 9104),      # first d of dr 512 (nch 2); fewer candidates than directions: stops after 75 picks
    "C5": (513, 43, 0, 18, np.inf, 9105),       # first d of dr 1024 (nch 1, sixteen waves of row maxima)
    "C6": (513, 43, 490, 23, np.inf, 9106),     # the same with a short trailing block
    "C7": (1023, 43, 0, 18, np.inf, 9107),      # the largest fused shape: 128 KiB of LDS
    "C8": (1023, 43, 1000, 23, np.inf, 9108),   # the same, complement consumed
    "C9": (129, 61, 100, 29, 2, 9109),          # three-launch form above 128
    "C10": (300, 61, 270, 30, 2, 9110),         # three-launch form, rows beyond one 256-thread pass
    "C11": (1024, 21, 1004, 20, np.inf, 9111),  # three-launch form at the boundary, dz small
    "C12": (1024, 21, 0, 3, np.inf, 9112),      # the same at dz = 1024: 64 KiB of dynamic LDS on top of 2 KiB static
    "C13": (1025, 21, 1005, 20, np.inf, 9113),  # the rocBLAS form
    "C14": (300, 61, 0, 300, np.inf, 9114),     # pivot stop after 18 picks (the pivot lies between the best scores of scans 18 and 19)
}
C14_PICKS = 18


def form_of(d, p):
    """the form of mrbf_affine_select that (d, p) takes (include/mrbf.h)"""
    if d > 1024:
        return "rocblas"
    return "fused" if np.isinf(p) and d <= 1023 else "three"


def layout_of(d):
    """(dr, nch) of the fused kernel's (row, chunk) thread layout"""
    dr = 64
    while dr < d:
        dr <<= 1
    return dr, 1024 // dr


# ---- the reference of the pick loop ----------------------------------------------------------------------------------------------
def _norms(A, p):
    """p-norms of the columns of A"""
    return np.abs(A).max(axis=0) if np.isinf(p) else np.sqrt((A * A).sum(axis=0))


def trailing_columns(Y):
    """the columns of the complete QR's Q behind the first Y.shape[1] (the identity for an empty Y: no reflector yet)"""
    d, j = Y.shape
    if j == 0:
        return np.eye(d)
    Q, _ = np.linalg.qr(Y, mode="complete")
    return Q[:, j:]


def plain_scores(Q2, S, p):
    """val_c = |Z (Z' s_c)|_p with Z = Q2's columns at unit p-norm, in float64"""
    Z = Q2 / _norms(Q2, p)[None, :]
    return _norms(Z @ (Z.T @ S.T), p)


def pick_loop(S, Y0, max_picks, pivot, p, scores=plain_scores):
    """-> picks, per pick the best and second-best score and their relative gap, per scan (a final one that stops the loop included) the
    relative distance of the best score from the pivot, and the final Z (d x (d - j0 - picks), unit p-norm columns)"""
    S = np.array(S, dtype=np.float64)
    Y = np.array(Y0, dtype=np.float64).reshape(S.shape[1], -1)
    limit = min(max_picks, S.shape[1] - Y.shape[1])
    out = SimpleNamespace(picks=[], best=[], second=[], gap=[], pivot_distance=[])
    Q2 = trailing_columns(Y)
    while len(out.picks) < limit:
        vals = scores(Q2, S, p)
        i = int(np.argmax(vals))                                   # np.argmax keeps the first maximiser
        b = float(vals[i])
        s2 = float(np.delete(vals, i).max()) if vals.size > 1 else 0.0
        out.pivot_distance.append(abs(b - pivot) / max(b, pivot))
        if not b > pivot:
            break
        out.picks.append(i), out.best.append(b), out.second.append(s2), out.gap.append((b - s2) / b)
        Y = np.hstack([Y, S[i][:, None]])
        S[i] = 0.0
        Q2 = trailing_columns(Y)
    out.Z = Q2 / _norms(Q2, p)[None, :] if Q2.shape[1] else Q2
    return out


def mirror_Z(Y0, S, picks, p):
    """the host mirror's final Z (sampling._GrowingQR grown by one reflector per pick) for a given pick list"""
    qr = sampling._GrowingQR(S.shape[1], Y0)
    for i in picks:
        qr.append(S[i])
    return qr.complement(p)


# ---- one score scan in extended precision ----------------------------------------------------------------------------------------
def _score_reference_mp(S, Z, p, digits=50):
    import mpmath as mp

    with mp.workdps(digits):
        f = np.frompyfunc(lambda v: mp.mpf(float(v)), 1, 1)
        U = np.dot(np.dot(f(S), f(Z)), f(Z).T)
        if np.isinf(p):
            val = [max(abs(u) for u in row) for row in U]
        else:
            val = [mp.sqrt(mp.fsum(u * u for u in row)) for row in U]
        return np.array([float(v) for v in val]).astype(LD)


def score_reference(S, Z, p):
    """val_c = |Z (Z' s_c)|_p as np.longdouble -- computed in np.longdouble where that is the x87 format (64-bit significand), in mpmath
    at 50 digits otherwise -- and the componentwise magnitude B_c = | |Z| (|Z|' |s_c|) |_p of the error bound (float64)"""
    S, Z = np.asarray(S, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    A = np.abs(S) @ np.abs(Z) @ np.abs(Z).T
    B = np.abs(A).max(axis=1) if np.isinf(p) else np.sqrt((A * A).sum(axis=1))
    if np.finfo(LD).nmant >= 63:
        Zl = Z.astype(LD)
        U = (S.astype(LD) @ Zl) @ Zl.T
        val = np.abs(U).max(axis=1) if np.isinf(p) else np.sqrt((U * U).sum(axis=1))
    else:
        val = _score_reference_mp(S, Z, p)
    return val, B


def score_bound(d, dz, B):
    return 2.0 * (d + dz + 4) * EPS * B


def score_errors_over_bound(vals, ref, B, d, dz):
    """|val - ref| / bound per candidate (< 1 passes; a candidate with B = 0 must score exactly 0; not finite counts as inf)"""
    err = np.abs(np.asarray(vals, dtype=LD) - ref).astype(np.float64)
    bound = score_bound(d, dz, B)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(e), e, np.inf)


# ---- the fused kernel's score step in NumPy ----------------------------------------------------------------------------------------
def fused_scores(Q2, S, p=np.inf, drop_last_chunk_at_dr=None):
    """affsel_pick_body's scores for the trailing columns Q2 (d x dz): Zs = Q2 D^2 (D = 1 / column maxima), the candidates in the trailing
    basis x_c = Q2' s_c, u = sum over the nch chunks (fixed order) of Zs[:, chunk] x_c[chunk], val_c = max_r |u_r|.
    drop_last_chunk_at_dr = dr: the mutation -- the last of the nch chunks is left out of the sum when the layout's dr is that value."""
    assert np.isinf(p)
    d, dz = Q2.shape
    dr, nch = layout_of(d)
    nrm = np.abs(Q2).max(axis=0)
    Zs = Q2 * (1.0 / (nrm * nrm))[None, :]
    X = S @ Q2
    kw = -(-dz // nch)
    u = np.zeros((S.shape[0], d))
    for ch in range(nch):
        k0, k1 = ch * kw, min(dz, (ch + 1) * kw)
        if k0 >= k1 or (ch == nch - 1 and dr == drop_last_chunk_at_dr):
            continue
        u += X[:, k0:k1] @ Zs[:, k0:k1].T
    return np.abs(u).max(axis=1)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def candidate_data(seed, d, mc, j0):
    """the recipe of tests/test_gpu_affine_batch.py::_start: mc shifted candidates in a box, then the j0 directions chosen so far"""
    rng = np.random.default_rng(seed)
    S = np.ascontiguousarray(0.1 * (2.0 * rng.random((mc, d)) - 1.0))
    Y0 = rng.standard_normal((d, j0))
    return S, Y0


def select_case(name):
    """data and reference results of one case: computed once, read-only"""
    if name in _CASES:
        return _CASES[name]
    d, mc, j0, max_picks, p, seed = CASES[name]
    S, Y0 = candidate_data(seed, d, mc, j0)
    pivot = PIVOT
    if name == "C14":
        # The best score of a scan does not fall from pick to pick on rows of one size (a reflector's columns have inf-norms well below 1,
        # and the scaling to unit inf-norm raises every later score: 0.100, 0.110, 0.114 .. 0.153 over 25 picks of this recipe), so no
        # pivot separates scans 1 .. 18 from scan 19 there.  The rows of this case shrink by 0.85 from one to the next in a shuffled
        # order: the best scores fall, and the pivot lies half-way (geometric mean) between those of scans 18 and 19.
        S = np.ascontiguousarray(S * (0.85 ** np.random.default_rng(seed + 1).permutation(mc))[:, None])
        probe = pick_loop(S, Y0, C14_PICKS + 1, PIVOT, p)
        pivot = float(np.sqrt(probe.best[C14_PICKS - 1] * probe.best[C14_PICKS]))
    Q0 = np.asfortranarray(sampling._GrowingQR(d, Y0).Q) if j0 > 0 else None
    case = SimpleNamespace(name=name, d=d, mc=mc, j0=j0, max_picks=max_picks, p=p, p_is_inf=1 if np.isinf(p) else 0, pivot=pivot, S=S, Y0=Y0,
                           Q0=Q0, form=form_of(d, p), layout=layout_of(d), ref=pick_loop(S, Y0, max_picks, pivot, p))
    for arr in (S, Y0, case.ref.Z) + (() if Q0 is None else (Q0,)):
        arr.setflags(write=False)
    _CASES[name] = case
    return case


def start_of(case, **over):
    """the case as a start of tests/test_gpu_affine_batch.py (run_single / run_batch)"""
    st = dict(S=case.S, d=case.d, mc=case.mc, j0=case.j0, Q0=case.Q0, pivot=case.pivot, max_picks=case.max_picks)
    st.update(over)
    return st


def other_start(seed, d, mc, j0, pivot=PIVOT, max_picks=None):
    """a start of the same recipe that is no case (the batches' third start)"""
    S, Y0 = candidate_data(seed, d, mc, j0)
    Q0 = np.asfortranarray(sampling._GrowingQR(d, Y0).Q) if j0 > 0 else None
    return dict(S=S, d=d, mc=mc, j0=j0, Q0=Q0, pivot=pivot, max_picks=d - j0 if max_picks is None else max_picks)
