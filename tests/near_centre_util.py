"""Shared by tests/test_near_centre_reference.py and tests/test_gpu_near_centres.py (not a test module): queries and sites close to a
centre, an extended-precision reference of the evaluation in DIFFERENCE form, and the checker both files push their results through.

Every device path but the cross-Gram forms |x - c|^2 as |x|^2 + |c|^2 - 2 <x, c> on centred coordinates, which loses all figures of a
distance below ~1e-8 while the coordinates stay O(1).  Radial functions whose phi' (cubic, beta = 1) or phi' / rho (thin plate spline,
k = 1) is unbounded at 0 magnify that without limit; the smooth ones do not.  The cases here put queries at 0, 1e-12 .. 1e-2 from
centres at tile edges, for every evaluation-kernel variant (VARIANTS) and every family of radial function (KERNELS).

Bounds (`errors_over_bound`): the suite's own for the evaluation alone (test_eval_from_golden_coeffs_isolated_from_solve), per output
column with sw = max(1, max |w|):  |V - V_ref| <= 1e-12 sw n max(1, max |V_ref|),  |J - J_ref| <= 1e-11 sw n max(1, max |J_ref|)."""
import math
from types import SimpleNamespace

import numpy as np

from oracle import rbf_oracle as orc

LD = np.longdouble

# name: d, n, k  -- the smallest shapes that reach each evaluation kernel (launch_pass; a model of >= 4 centre tiles splits the centre
# range for a small query batch, eval_nsplit)
VARIANTS = {
    "d64_final": (10, 100, 2),
    "d64_split": (64, 300, 2),
    "d128_final": (100, 150, 3),
    "d128_split": (100, 300, 3),
    "d256_final": (140, 150, 2),
    "d256_split": (140, 300, 2),
    "d_gt_256": (300, 200, 2),
}
# name: kernel, shape parameter  -- (a, b) follow from rbf_oracle.kernel_params: the fast paths, the pow paths and the branchy ones
KERNELS = {
    "cubic1": ("cubic", 1.0),
    "cubic3": ("cubic", 3.0),
    "cubic5": ("cubic", 5.0),
    "tps1": ("thin_plate_spline", 1.0),
    "tps2": ("thin_plate_spline", 2.0),
    "gaussian": ("gaussian", 1.0),
    "multiquadric": ("multiquadric", 1.0),
    "inv_multiquadric": ("inv_multiquadric", 1.0),
}
DELTAS = (0.0, 1e-12, 1e-9, 3e-8, 1e-6, 1e-4, 1e-2)
N_FAR = 8
DEG = 1


def kernel_ids(kernel):
    name, sp = KERNELS[kernel]
    a, b = orc.kernel_params(name, sp)
    return orc.KERNEL_IDS[name], a, b


# ---- the reference: difference form in extended precision ----------------------------------------------------------------------
def _phi_psi_ld(kid, a, b, rho):
    """phi(rho) and psi(rho) = phi'(rho) / rho in np.longdouble; the rho = 0 term as rbf_oracle.dphi_over_rho defines it"""
    rho = np.asarray(rho, dtype=LD)
    one, two = LD(1), LD(2)
    a, b = LD(a), LD(b)
    zero = rho == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        if kid == 4:
            e = np.exp(-(a * rho) ** 2)
            return e, -two * a * a * e
        if kid == 2:
            sgn = LD((-1.0) ** math.ceil(float(b)))
            t = one + (a * rho) ** 2
            return sgn * t ** b, sgn * two * a * a * b * t ** (b - one)
        if kid == 1:
            t = one + (a * rho) ** 2
            return t ** (-b), -two * a * a * b * t ** (-b - one)
        if kid == 0:
            sgn = LD((-1.0) ** math.ceil(float(a) / 2.0))
            psi = sgn * a * rho ** (a - two)
            return sgn * rho ** a, (np.where(zero, LD(0), psi) if a < 2 else psi)
        if kid == 3:
            k = int(a)
            lg = np.log(rho)
            phi = LD((-1.0) ** (k + 1)) * rho ** (2 * k) * lg
            psi = LD((-1.0) ** (k + 1)) * rho ** (2 * k - 2) * (2 * k * lg + one)
            return np.where(zero, LD(0), phi), np.where(zero, LD(0), psi)
    raise ValueError(kid)


def _reference_eval_ld(C, W, Lam, kid, a, b, deg, X):
    C, W, X = np.asarray(C, dtype=LD), np.asarray(W, dtype=LD), np.asarray(X, dtype=LD)
    Lam = np.asarray(Lam, dtype=LD).reshape(-1, W.shape[1])
    m, d = X.shape
    k = W.shape[1]
    V, J = np.zeros((m, k), dtype=LD), np.zeros((m, k, d), dtype=LD)
    for p in range(m):
        diff = X[p][None, :] - C                                  # exact: both are doubles, the difference fits 64 bits where it matters
        rho = np.sqrt((diff * diff).sum(axis=1))
        phi, psi = _phi_psi_ld(kid, a, b, rho)
        V[p] = phi @ W
        J[p] = (W * psi[:, None]).T @ diff
        if deg >= 0:
            V[p] += Lam[0]
        if deg >= 1:
            V[p] += X[p] @ Lam[1:]
            J[p] += Lam[1:].T
    return V, J


def reference_eval_mp(C, W, Lam, kid, a, b, deg, X, digits=50):
    """the same in mpmath at `digits` digits; returns (V, J) as object arrays of mpf"""
    import mpmath as mp

    with mp.workdps(digits):
        f = np.frompyfunc(lambda v: mp.mpf(float(v)), 1, 1)
        C, W, X = f(np.asarray(C, dtype=np.float64)), f(np.asarray(W, dtype=np.float64)), f(np.asarray(X, dtype=np.float64))
        Lam = f(np.asarray(Lam, dtype=np.float64).reshape(-1, W.shape[1])) if deg >= 0 else None
        m, d = X.shape
        n, k = W.shape
        a_, b_ = mp.mpf(a), mp.mpf(b)

        def phi_psi(rho):
            if kid == 4:
                e = mp.exp(-(a_ * rho) ** 2)
                return e, -2 * a_ * a_ * e
            if kid == 2:
                sgn = (-1) ** math.ceil(b)
                t = 1 + (a_ * rho) ** 2
                return sgn * t ** b_, sgn * 2 * a_ * a_ * b_ * t ** (b_ - 1)
            if kid == 1:
                t = 1 + (a_ * rho) ** 2
                return t ** (-b_), -2 * a_ * a_ * b_ * t ** (-b_ - 1)
            if kid == 0:
                sgn = (-1) ** math.ceil(a / 2.0)
                if rho == 0:
                    return mp.mpf(0), mp.mpf(0)    # beta >= 3: the limit; beta = 1: no limit -> 0
                return sgn * rho ** a_, sgn * a_ * rho ** (a_ - 2)
            kk = int(a)
            if rho == 0:
                return mp.mpf(0), mp.mpf(0)
            lg, sgn = mp.log(rho), (-1) ** (kk + 1)
            return sgn * rho ** (2 * kk) * lg, sgn * rho ** (2 * kk - 2) * (2 * kk * lg + 1)

        V, J = np.empty((m, k), dtype=object), np.empty((m, k, d), dtype=object)
        for p in range(m):
            v = [Lam[0, l] if deg >= 0 else mp.mpf(0) for l in range(k)]
            g = [[Lam[1 + t, l] if deg >= 1 else mp.mpf(0) for t in range(d)] for l in range(k)]
            if deg >= 1:
                for l in range(k):
                    v[l] += mp.fsum(Lam[1 + t, l] * X[p, t] for t in range(d))
            for c in range(n):
                diff = [X[p, t] - C[c, t] for t in range(d)]
                phi, psi = phi_psi(mp.sqrt(mp.fsum(x * x for x in diff)))
                for l in range(k):
                    v[l] += W[c, l] * phi
                    wp = W[c, l] * psi
                    for t in range(d):
                        g[l][t] += wp * diff[t]
            for l in range(k):
                V[p, l] = v[l]
                for t in range(d):
                    J[p, l, t] = g[l][t]
        return V, J


def reference_eval(C, W, Lam, kid, a, b, deg, X):
    """values (m, k) and Jacobians (m, k, d) of the model in difference form, the formulas of oracle/rbf_oracle.py, as np.longdouble
    arrays: computed in np.longdouble where that is the x87 format (64-bit significand), in mpmath at 50 digits otherwise"""
    if np.finfo(LD).nmant >= 63:
        return _reference_eval_ld(C, W, Lam, kid, a, b, deg, X)
    V, J = reference_eval_mp(C, W, Lam, kid, a, b, deg, X, 50)
    return V.astype(np.float64).astype(LD), J.astype(np.float64).astype(LD)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
_CASES = {}


def near_centre_case(variant, kernel):
    """sites, coefficients and the 43 queries of one (evaluation-kernel variant, radial function): computed once, read-only.
    Queries: x = c + delta u for the centres 0, 63, 64, n - 1 (tile edges, the ragged last tile, both ends of a split centre range),
    the seven DELTAS and one random unit vector u per centre; for centre 0 also u = e_1 (only one coordinate differs, the padding
    agrees); 8 uniform points far from every centre.  `delta[i]` / `target[i]` describe query i (far points: nan / -1)."""
    key = (variant, kernel)
    if key in _CASES:
        return _CASES[key]
    d, n, k = VARIANTS[variant]
    kid, a, b = kernel_ids(kernel)
    rng = np.random.Generator(np.random.PCG64(20240 + sorted(VARIANTS).index(variant)))
    C = rng.random((n, d))
    targets = (0, 63, 64, n - 1)
    W = rng.standard_normal((n, k))
    W /= np.abs(W).max()
    for i, c in enumerate(targets):
        W[c] = [1.0 if (i + l) % 2 == 0 else -1.0 for l in range(k)]   # the near term cannot hide behind a small weight
    Lam = rng.standard_normal((d + 1, k))
    X, delta, target = [], [], []
    for c in targets:
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        for dl in DELTAS:
            X.append(C[c] + dl * u)
            delta.append(dl)
            target.append(c)
    e1 = np.zeros(d)
    e1[0] = 1.0
    for dl in DELTAS:
        X.append(C[0] + dl * e1)
        delta.append(dl)
        target.append(0)
    for _ in range(N_FAR):
        X.append(rng.random(d))
        delta.append(float("nan"))
        target.append(-1)
    X = np.ascontiguousarray(np.array(X))
    name, sp = KERNELS[kernel]
    case = SimpleNamespace(variant=variant, kernel=kernel, kernel_name=name, shape_parameter=sp, d=d, n=n, k=k, kid=kid, a=a, b=b, deg=DEG,
                           C=C, W=W, Lam=Lam, X=X, delta=np.array(delta), target=np.array(target), targets=targets)
    case.V_ref, case.J_ref = reference_eval(C, W, Lam, kid, a, b, DEG, X)     # of the fp64 x that is actually passed
    for arr in (C, W, Lam, X, case.delta, case.target, case.V_ref, case.J_ref):
        arr.setflags(write=False)
    _CASES[key] = case
    return case


def clustered_sites(d, n, radius, seed=0):
    """the late-iteration geometry: one site x0, n / 2 - 1 sites in the box x0 +- radius, n / 2 uniform sites in the unit cube"""
    rng = np.random.Generator(np.random.PCG64(7700 + 13 * d + n + seed))
    x0 = 0.25 + 0.5 * rng.random(d)
    near = x0 + radius * (2.0 * rng.random((n // 2 - 1, d)) - 1.0)
    far = rng.random((n - n // 2, d))
    return np.ascontiguousarray(np.vstack([x0[None, :], near, far]))


def cluster_values(C, k=2):
    """smooth training values at the sites, every column different"""
    s = C.sum(axis=1) / C.shape[1]
    return np.stack([np.sin((1.0 + 0.7 * j) * np.pi * s + 0.3 * j) + 0.1 * j for j in range(k)], axis=1)


def step_queries(x0, seed=0):
    """x0 and x0 + delta u for the non-zero DELTAS and one random unit vector u"""
    rng = np.random.Generator(np.random.PCG64(99 + seed))
    u = rng.standard_normal(x0.shape[0])
    u /= np.linalg.norm(u)
    return np.ascontiguousarray(np.array([x0 + dl * u for dl in DELTAS]))


# ---- the checker ---------------------------------------------------------------------------------------------------------------
V_BOUND, J_BOUND = 1e-12, 1e-11


def bounds(W, n, V_ref, J_ref):
    """per output column: (value bound, Jacobian bound) as absolute numbers"""
    sw = np.maximum(1.0, np.abs(np.asarray(W, dtype=np.float64)).max(axis=0))
    vmax = np.maximum(1.0, np.abs(V_ref).max(axis=0).astype(np.float64))
    jmax = np.maximum(1.0, np.abs(J_ref).max(axis=(0, 2)).astype(np.float64))
    return V_BOUND * sw * n * vmax, J_BOUND * sw * n * jmax


def errors_over_bound(W, n, V_ref, J_ref, V=None, J=None):
    """error / bound per query (the worst output column and coordinate of each): two arrays of m figures, < 1 passes; a result that is
    not finite counts as inf.  The difference is taken in extended precision against the reference as it stands."""
    bv, bj = bounds(W, n, V_ref, J_ref)
    m = V_ref.shape[0]
    ev, ej = np.zeros(m), np.zeros(m)
    if V is not None:
        e = np.abs(np.asarray(V, dtype=LD) - V_ref).astype(np.float64) / bv[None, :]
        ev = np.where(np.isfinite(e), e, np.inf).max(axis=1)
    if J is not None:
        e = np.abs(np.asarray(J, dtype=LD) - J_ref).astype(np.float64) / bj[None, :, None]
        ej = np.where(np.isfinite(e), e, np.inf).max(axis=(1, 2))
    return ev, ej


def by_delta(case, e):
    """the worst figure of the per-query array e for each delta, and for the far points"""
    out = {("%g" % dl): float(e[case.delta == dl].max()) for dl in DELTAS}
    out["far"] = float(e[case.target < 0].max())
    return out


def gemm_form_eval(case):
    """what the GEMM-form kernels compute, in NumPy: centred coordinates, s = max(|x|^2 + |c|^2 - 2 <x, c>, 0), the Jacobian as
    (sum a) x - sum a c with a = w psi.  The checker must reject this for the non-smooth radial functions."""
    mean = case.C.mean(axis=0)
    Cc, Xc = case.C - mean, case.X - mean
    s = np.maximum((Xc * Xc).sum(axis=1)[:, None] + (Cc * Cc).sum(axis=1)[None, :] - 2.0 * (Xc @ Cc.T), 0.0)
    rho = np.sqrt(s)
    V = orc.phi(case.kid, case.a, case.b, rho) @ case.W + orc.poly_matrix(case.X, case.deg) @ case.Lam
    A = orc.dphi_over_rho(case.kid, case.a, case.b, rho)
    J = np.empty((case.X.shape[0], case.k, case.d))
    for l in range(case.k):
        Al = A * case.W[None, :, l]
        J[:, l, :] = Al.sum(axis=1)[:, None] * Xc - Al @ Cc + case.Lam[1:, l][None, :]
    return V, J
