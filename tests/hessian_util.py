"""Shared by tests/test_hessian_reference.py and tests/test_gpu_hessian.py (not a test module): an extended-precision reference of
the model Hessian in DIFFERENCE form, the derived bound, the checker both files push their results through, and the shapes of the GPU
tests.

    H_l(x) = sum_c w_cl [ psi(s_c) I + chi(s_c) (x - c)(x - c)' ],   s = rho^2,  psi = phi'/rho,  chi = (phi'' - phi'/rho) / rho^2

A centre with s = 0 contributes w psi(0) I (psi(0): the limit, or 0 where none exists -- rbf_oracle.dphi_over_rho) and no rank-one term.
The long-double code below holds closed forms of its own; the mpmath evaluator obtains phi' and phi'' from phi by mpmath.diff and so
shares no closed form with the product.

Bound per entry (derived, not measured):   |H_ij - H_ref,ij| <= 2 (n + 8 d + 32) 2^-52 S_ij,
    S_ij = sum_c |w_cl| ( |chi_c| |x_i - c_i| |x_j - c_j| + [i = j] |psi_c| )
n: a recursive sum of n terms in any order; 8 d: the d-term sum of squares behind s times the condition of psi and chi in s (at most 8
for the parameters tested: a gaussian needs a^2 s <= 4 over the box, hence `gaussian_shape`); 32: the handful of operations per term;
2: spare."""
import math
from types import SimpleNamespace

import numpy as np

from oracle import rbf_oracle as orc
from tests.near_centre_util import KERNELS

LD = np.longdouble
EPS = 2.0 ** -52

# kernels of the GPU tests beyond near_centre_util.KERNELS: name -> (kernel id, a, b); the pow paths of the multiquadrics
EXTRA_KERNELS = {
    "multiquadric_b1.5": (orc.KERNEL_IDS["multiquadric"], 1.0, 1.5),
    "inv_multiquadric_b1.5": (orc.KERNEL_IDS["inv_multiquadric"], 1.0, 1.5),
}


def gaussian_shape(d):
    """a with a^2 s <= 4 over the unit box (s <= d)"""
    return 2.0 / math.sqrt(d)


def kernel_ids(kernel, d):
    """(kid, a, b) of a name of near_centre_util.KERNELS or EXTRA_KERNELS; the gaussian with the shape the bound's derivation needs"""
    if kernel in EXTRA_KERNELS:
        return EXTRA_KERNELS[kernel]
    name, sp = KERNELS[kernel]
    if name == "gaussian":
        sp = gaussian_shape(d)
    a, b = orc.kernel_params(name, sp)
    return orc.KERNEL_IDS[name], a, b


def factor(n, d):
    return 2.0 * (n + 8 * d + 32) * EPS


# ---- long double, closed forms of its own --------------------------------------------------------------------------------------
def psi_chi_ld(kid, a, b, s):
    """psi(s) and chi(s) in np.longdouble for s > 0; at s == 0: psi(0) by the convention above and chi = 0 (no rank-one term)"""
    s = np.asarray(s, dtype=LD)
    one, two = LD(1), LD(2)
    a, b = LD(a), LD(b)
    zero = s == 0
    ss = np.where(zero, one, s)                    # a stand-in where s == 0: selected away below
    if kid == 4:
        e = np.exp(-a * a * s)
        psi, chi = -two * a * a * e, LD(4) * a ** 4 * e
    elif kid == 2:
        sgn = LD((-1.0) ** math.ceil(float(b)))
        t = one + a * a * s
        psi, chi = sgn * two * a * a * b * t ** (b - one), sgn * LD(4) * a ** 4 * b * (b - one) * t ** (b - two)
    elif kid == 1:
        t = one + a * a * s
        psi, chi = -two * a * a * b * t ** (-b - one), LD(4) * a ** 4 * b * (b + one) * t ** (-b - two)
    elif kid == 0:
        sgn = LD((-1.0) ** math.ceil(float(a) / 2.0))
        rho = np.sqrt(ss)
        psi = np.where(zero, LD(0), sgn * a * rho ** (a - two))
        chi = sgn * a * (a - two) * rho ** (a - LD(4))
    elif kid == 3:
        k = int(a)
        sgn = LD((-1.0) ** (k + 1))
        lg = np.log(ss)
        psi = np.where(zero, LD(0), sgn * ss ** (k - 1) * (k * lg + one))
        chi = sgn * two * ss ** LD(k - 2) * ((k - 1) * (k * lg + one) + k)
    else:
        raise ValueError(kid)
    return psi, np.where(zero, LD(0), chi)


def _rank_one_sums(diff, g):
    """sum_c g_c diff_c diff_c' for every column of g: (r, d, d)"""
    return np.stack([(diff * g[:, j][:, None]).T @ diff for j in range(g.shape[1])])


def reference_hessian_ld(C, W, kid, a, b, X, rows=None):
    """H (m, r, d, d) and S (m, r, d, d) in np.longdouble, difference form"""
    C, W, X = np.asarray(C, dtype=LD), np.asarray(W, dtype=LD), np.asarray(X, dtype=LD)
    rows = list(range(W.shape[1])) if rows is None else list(rows)
    m, d = X.shape
    H, S = np.zeros((m, len(rows), d, d), dtype=LD), np.zeros((m, len(rows), d, d), dtype=LD)
    eye = np.eye(d, dtype=LD)
    for p in range(m):
        diff = X[p][None, :] - C                   # exact where it matters: both are doubles
        psi, chi = psi_chi_ld(kid, a, b, (diff * diff).sum(axis=1))
        Wr = W[:, rows]
        H[p] = _rank_one_sums(diff, Wr * chi[:, None]) + (Wr * psi[:, None]).sum(axis=0)[:, None, None] * eye
        S[p] = _rank_one_sums(np.abs(diff), np.abs(Wr * chi[:, None])) + np.abs(Wr * psi[:, None]).sum(axis=0)[:, None, None] * eye
    return H, S


# ---- mpmath: phi' and phi'' by mpmath.diff from phi ------------------------------------------------------------------------------
def reference_hessian_mp(C, W, kid, a, b, X, rows=None, digits=50):
    """the same at `digits` digits; object arrays of mpf.  psi = phi'/rho, chi = (phi'' - phi'/rho)/rho^2 with the derivatives taken
    numerically from phi; psi(0) = phi''(0) for the radial functions that are smooth at 0, else 0"""
    import mpmath as mp

    C, W, X = np.asarray(C, dtype=np.float64), np.asarray(W, dtype=np.float64), np.asarray(X, dtype=np.float64)
    rows = list(range(W.shape[1])) if rows is None else list(rows)
    m, d = X.shape
    n = C.shape[0]
    with mp.workdps(digits):
        a_, b_ = mp.mpf(a), mp.mpf(b)

        def phi(rho):
            if kid == 4:
                return mp.exp(-(a_ * rho) ** 2)
            if kid == 2:
                return (-1) ** math.ceil(b) * (1 + (a_ * rho) ** 2) ** b_
            if kid == 1:
                return (1 + (a_ * rho) ** 2) ** (-b_)
            if kid == 0:
                return (-1) ** math.ceil(a / 2.0) * rho ** a_
            return (-1) ** (int(a) + 1) * rho ** (2 * int(a)) * mp.log(rho)

        def psi_chi(rho):
            if rho == 0:
                return (mp.diff(phi, 0, 2) if kid in (1, 2, 4) else mp.mpf(0)), mp.mpf(0)
            d1, d2 = mp.diff(phi, rho, 1), mp.diff(phi, rho, 2)    # absolute step 2^-(prec + 10) at (n + 1)-fold working precision
            return d1 / rho, (d2 - d1 / rho) / rho ** 2

        H = np.empty((m, len(rows), d, d), dtype=object)
        S = np.empty((m, len(rows), d, d), dtype=object)
        for p in range(m):
            for jr in range(len(rows)):
                for i in range(d):
                    for j in range(d):
                        H[p, jr, i, j] = mp.mpf(0)
                        S[p, jr, i, j] = mp.mpf(0)
            for c in range(n):
                diff = [mp.mpf(float(X[p, t])) - mp.mpf(float(C[c, t])) for t in range(d)]
                psi, chi = psi_chi(mp.sqrt(mp.fsum(x * x for x in diff)))
                for jr, l in enumerate(rows):
                    w = mp.mpf(float(W[c, l]))
                    wc, wp = w * chi, w * psi
                    for i in range(d):
                        H[p, jr, i, i] += wp
                        S[p, jr, i, i] += abs(wp)
                        wci = wc * diff[i]
                        for j in range(d):
                            t = wci * diff[j]
                            H[p, jr, i, j] += t
                            S[p, jr, i, j] += abs(t)
        return H, S


def reference_hessian(C, W, kid, a, b, X, rows=None):
    """H and S as np.longdouble arrays: long double where that is the x87 format (64-bit significand), mpmath at 50 digits otherwise"""
    if np.finfo(LD).nmant >= 63:
        return reference_hessian_ld(C, W, kid, a, b, X, rows)
    H, S = reference_hessian_mp(C, W, kid, a, b, X, rows, 50)
    return H.astype(np.float64).astype(LD), S.astype(np.float64).astype(LD)


def reference_jacobian_ld(C, W, kid, a, b, X):
    """(m, k, d): the Jacobian of the radial part in long double (for the difference quotients of the reference)"""
    C, W, X = np.asarray(C, dtype=LD), np.asarray(W, dtype=LD), np.asarray(X, dtype=LD)
    J = np.zeros((X.shape[0], W.shape[1], X.shape[1]), dtype=LD)
    for p in range(X.shape[0]):
        diff = X[p][None, :] - C
        psi, _ = psi_chi_ld(kid, a, b, (diff * diff).sum(axis=1))
        J[p] = (W * psi[:, None]).T @ diff
    return J


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def errors_over_bound(H, H_ref, S, n, d):
    """error / bound per entry (same shape as H_ref), < 1 passes; a result that is not finite counts as inf; 0 / 0 (an entry whose
    terms all vanish and which is reproduced exactly) counts as 0"""
    err = np.abs(np.asarray(H, dtype=LD) - H_ref).astype(np.float64)
    bound = factor(n, d) * np.asarray(S, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    return np.where(np.isfinite(ratio), ratio, np.inf)


def gemm_form_hessian(C, W, kid, a, b, X, rows=None):
    """what a GEMM-form kernel would compute, in fp64 NumPy: s = max(|x|^2 + |c|^2 - 2 <x, c>, 0), psi and chi of that s, the
    rank-one factors still x - c.  The checker must reject this near a centre for the radial functions whose chi is unbounded."""
    C, W, X = np.asarray(C, dtype=np.float64), np.asarray(W, dtype=np.float64), np.asarray(X, dtype=np.float64)
    rows = list(range(W.shape[1])) if rows is None else list(rows)
    m, d = X.shape
    s_all = np.maximum((X * X).sum(axis=1)[:, None] + (C * C).sum(axis=1)[None, :] - 2.0 * (X @ C.T), 0.0)
    H = np.zeros((m, len(rows), d, d))
    for p in range(m):
        psi, chi = psi_chi_ld(kid, a, b, s_all[p])
        psi, chi = psi.astype(np.float64), chi.astype(np.float64)
        diff = X[p][None, :] - C
        Wr = W[:, rows]
        H[p] = _rank_one_sums(diff, Wr * chi[:, None]) + (Wr * psi[:, None]).sum(axis=0)[:, None, None] * np.eye(d)
    return H


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def random_model(d, n, k, seed):
    """centres in the unit box, normal weights"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.ascontiguousarray(rng.random((n, d))), np.ascontiguousarray(rng.standard_normal((n, k))), rng


def near_queries(C, centres, deltas, rng):
    """x = c + delta u for every (centre, delta), one random unit vector u per centre"""
    X = []
    for c in centres:
        u = rng.standard_normal(C.shape[1])
        u /= np.linalg.norm(u)
        X += [C[c] + dl * u for dl in deltas]
    return np.ascontiguousarray(np.array(X))


# name: (d, n, m, k, rows, why)  -- rows: "all", "last" ([k - 1]) or "rep" ([1, 0, 1]).  The kernel's variants (hess.hip, hess_host.hpp):
# outputs per pass RB = 1, 2 or 4 (r >= 3; a last pass with idle outputs); one block pair (d <= 64) or several; rounds of 32 centres
# with a last partial 4-centre step; the centre range in one piece (n <= 32, or m * pairs * passes >= 512) or split.
VARIANTS = {
    "one": (1, 1, 1, 1, "all", "one coordinate, one centre: 15 idle rows of the one tile, 31 padding centres, RB = 1"),
    "d3_n3": (3, 3, 2, 2, "all", "a partial 4-centre step (3 centres), RB = 2, two queries, unsplit because n <= 32"),
    "d15_n4": (15, 4, 2, 3, "last", "one short of the tile edge, exactly one 4-centre step, a single selected output of three"),
    "d16_n5": (16, 5, 65, 3, "all", "exactly one tile; r = 3 runs as one pass of four with an idle output; 4 + 1 centres; m = 65"),
    "d17_n63": (17, 63, 64, 2, "rep", "one past the tile edge (3 tiles, 2 ragged); repeated rows; split in 2: 32 + 31 centres"),
    "d64_n257": (64, 257, 1, 2, "all", "a full diagonal block pair (10 tiles over 4 waves); m = 1 splits 9 ways, the last piece 1 centre"),
    "d65_n65": (65, 65, 2, 1, "all", "the smallest d with several block pairs (3), an off-diagonal pair of one ragged tile row; split in 3"),
    "d65_unsplit": (65, 63, 63, 17, "all", "the smallest unsplit call of several rounds (63 * 3 pairs * 5 passes >= 512): two rounds, "
                                           "the second ending in a partial step; the fifth pass has 1 of 4 outputs"),
    "d140_n64": (140, 64, 2, 3, "rep", "3 blocks, 6 pairs, the last block 12 wide; split in 2 of exactly one round each"),
    "d300_n300": (300, 300, 2, 2, "all", "d > 256: 5 blocks, 15 pairs; split in 10 pieces of one round, the last of 12 centres"),
    "d300_n5": (300, 5, 2, 17, "last", "d > 256 with the centre range in one piece: every block pair stores both triangles itself"),
}


def variant_rows(k, kind):
    return {"all": None, "last": [k - 1], "rep": [1, 0, 1]}[kind]


_CASES = {}


def variant_case(name, kernel="multiquadric"):
    """model, queries and reference of one (shape, radial function): computed once, read-only"""
    key = (name, kernel)
    if key not in _CASES:
        d, n, m, k, kind, _ = VARIANTS[name]
        kid, a, b = kernel_ids(kernel, d)
        C, W, rng = random_model(d, n, k, 4100 + sorted(VARIANTS).index(name))
        X = np.ascontiguousarray(rng.random((m, d)))
        rows = variant_rows(k, kind)
        H_ref, S = reference_hessian(C, W, kid, a, b, X, rows)
        for arr in (C, W, X, H_ref, S):
            arr.setflags(write=False)
        _CASES[key] = SimpleNamespace(name=name, kernel=kernel, d=d, n=n, m=m, k=k, rows=rows, kid=kid, a=a, b=b, C=C, W=W, X=X, H_ref=H_ref, S=S)
    return _CASES[key]
