"""Shared by tests/test_round4_batch_host.py and tests/test_gpu_round4_batch.py (not a test module): test inputs for the many-start
round 4 (mrbf_round4_batch), the oracle's list per start with the margin of every decision, and a NumPy restatement of the walk.

The batched walk sums in another order than mrbf_round4's blocked walk and than the oracle's from-scratch determinants, so equal
lists can only be demanded where no decision sits on the threshold.  That is a condition on the INPUT, checked here on the CPU with
the oracle alone (`oracle_case`): every tau^2 of the oracle's walk, recomputed from scratch as a ratio of `_logdet_spd` determinants of
kernel matrices projected onto `_round4_basis`'s subspace, must lie outside [thr / 100, 100 thr] -- above 100 thr (accepted with margin), below
thr / 100, or not positive (rejected with margin; where the threshold itself is below rounding, as with the default theta, a tau^2
at rounding level is no clear decision either: `margin_violations`).  An input that misses this is unfit and is not used; no decision is dropped.

Inputs with rejections (`clustered_case`): the candidates are well separated cluster heads, each followed somewhere later in the
(shuffled) order by near copies at distance ~eps.  With theta in 0.1 .. 0.5 the threshold (theta^2)^2 is 1e-4 .. 6e-2: whichever member
of a cluster comes first has tau^2 far above it, every later one far below."""
import math

import numpy as np

from oracle import rbf_oracle as orc
from oracle import sampling_oracle as so

KERNELS = {"cubic": (0, 3.0, 0.0), "inv_multiquadric": (1, 1.0, 0.5), "multiquadric": (2, 1.0, 0.5), "thin_plate_spline": (3, 2.0, 0.0),
           "gaussian": (4, 1.0, 0.0)}


def poly_dim(d, deg):
    return 0 if deg < 0 else (1 if deg == 0 else d + 1)


def start_set(rng, d, n0, scale):
    """the centre and n0 - 1 sites around it, affinely independent by construction (centre + scaled unit vectors first)"""
    x = np.full(d, 0.5 * scale)
    S = [x]
    for i in range(min(d, n0 - 1)):
        e = np.zeros(d)
        e[i] = 0.35 * scale * (1.0 if i % 2 == 0 else -1.0)
        S.append(x + e + 0.02 * scale * rng.standard_normal(d))
    while len(S) < n0:
        S.append(rng.random(d) * scale)
    return np.array(S)


def random_case(seed, d, n0, mc, scale=1.0):
    """generic sites: with the default theta = 1e-7 (threshold 1e-28) every candidate is accepted until max_points"""
    rng = np.random.default_rng(seed)
    return start_set(rng, d, n0, scale), rng.random((mc, d)) * scale


def clustered_case(seed, d, n0, mc, scale=4.0, eps=1e-5, copies=2):
    """mc candidates in clusters of `copies` near-identical sites (shuffled order): about (copies - 1) / copies of the decisions are
    rejections when theta is large"""
    rng = np.random.default_rng(seed)
    C0 = start_set(rng, d, n0, scale)
    heads = rng.random(((mc + copies - 1) // copies, d)) * scale
    X = np.vstack([heads + (eps * scale * rng.standard_normal(heads.shape) if c else 0.0) for c in range(copies)])[:mc]
    return C0, X[rng.permutation(X.shape[0])]


def _basis_qr(Pi0, P_acc):
    """the subspace of `sampling_oracle._round4_basis` -- orthogonal to range([Pi0; P_acc]) and to the start set's own null-space
    directions -- from two complete QR factorisations instead of two SVDs (a tenth of the time at 257 rows); Pi0 has full column rank"""
    N0, q = Pi0.shape
    j = P_acc.shape[0]
    Q2 = np.linalg.qr(Pi0, mode="complete")[0][:, q:] if q > 0 else np.eye(N0)
    A = np.block([[Pi0, Q2], [P_acc, np.zeros((j, Q2.shape[1]))]])
    return np.linalg.qr(A, mode="complete")[0][:, N0:]


def margins(C0, Xc, kid, a, b, deg, theta, max_points):
    """the oracle's walk with tau^2 of EVERY decision from scratch, the way the oracle forms it -- the ratio of the `_logdet_spd`
    determinants of the kernel matrix projected onto the round-4 subspace with and without the candidate; nothing is carried from
    one decision to the next but the accepted list and the last determinant -> (accepted positions, [(position, tau^2 or None when
    the projected matrix is not positive definite)])"""
    C0, Xc = np.asarray(C0, dtype=np.float64), np.asarray(Xc, dtype=np.float64).reshape(-1, np.asarray(C0).shape[1])
    n0, d = C0.shape
    if max_points is None or max_points <= 0:
        max_points = (d + 1) * (d + 2) // 2
    thr = (theta ** 2) ** 2
    Pi0, Pc = orc.poly_matrix(C0, deg), orc.poly_matrix(Xc, deg) if Xc.shape[0] else np.zeros((0, poly_dim(d, deg)))
    S = np.vstack([C0, Xc])
    Phi_all = orc.phi(kid, a, b, orc.pairwise_dist(S, S))        # kernel values of every pair, once; each decision takes its rows
    Phi_all = 0.5 * (Phi_all + Phi_all.T)
    acc, taus, ld_cur = [], [], 0.0
    for pos in range(Xc.shape[0]):
        if n0 + len(acc) >= max_points:
            break
        rows = list(range(n0)) + [n0 + i for i in acc + [pos]]
        B = _basis_qr(Pi0, Pc[acc + [pos]])
        ld = so._logdet_spd(B.T @ Phi_all[np.ix_(rows, rows)] @ B)
        tau2 = None if ld is None else math.exp(ld - ld_cur)
        taus.append((pos, tau2))
        if tau2 is not None and tau2 > thr:
            acc.append(pos)
            ld_cur = ld
    return acc, taus


def kernel_scale(C0, Xc, kid, a, b):
    """the largest kernel value among the sites: what the rounding of the projected determinants is relative to"""
    S = np.vstack([np.asarray(C0, dtype=np.float64), np.asarray(Xc, dtype=np.float64).reshape(-1, np.asarray(C0).shape[1])])
    return max(1.0, float(np.abs(orc.phi(kid, a, b, orc.pairwise_dist(S, S))).max()))


def margin_violations(taus, theta, factor=100.0, noise=0.0):
    """decisions that fp64 alone does not place on one side of the threshold thr = (theta^2)^2: tau^2 -- or, with `noise` > 0, any value
    within `noise` of it -- inside [thr / factor, factor * thr].  `noise` is the absolute rounding level of the from-scratch tau^2
    (`oracle_case` takes 1000 eps times the largest kernel value: the backward error of a Cholesky factorisation of matrices of that
    size); a projected matrix that is not positive definite (None) stands for tau^2 = 0 +- noise.  With the default theta = 1e-7
    (thr = 1e-28) an exact copy of an accepted site is such a decision: its tau^2 is rounding noise of either sign."""
    thr = (theta ** 2) ** 2
    bad = []
    for pos, t in taus:
        v = 0.0 if t is None else t
        if v + noise >= thr / factor and v - noise <= factor * thr:
            bad.append((pos, t))
    return bad


_CACHE = {}


def oracle_case(key, C0, Xc, kernel, deg, theta, max_points, full_oracle=True):
    """the expected list of one start, computed once per `key`: the margin condition asserted on every decision, and (full_oracle) the
    list of oracle/sampling_oracle.py::rbf_round4 asserted equal to the walk's.  Returns (accepted, share of rejections)."""
    if key not in _CACHE:
        kid, a, b = KERNELS[kernel]
        acc, taus = margins(C0, Xc, kid, a, b, deg, theta, max_points)
        bad = margin_violations(taus, theta, noise=1000.0 * np.finfo(float).eps * kernel_scale(C0, Xc, kid, a, b))
        assert not bad, "unfit test input %r: decisions within a factor 100 of the threshold: %r" % (key, bad[:4])
        if full_oracle:
            want = so.rbf_round4(list(C0), list(np.asarray(Xc).reshape(-1, C0.shape[1])), kid, a, b, deg, theta_pivot_cholesky=theta,
                                 max_points=max_points)
            assert want == acc, key
        _CACHE[key] = (acc, (len(taus) - len(acc)) / max(len(taus), 1))
    return _CACHE[key]


def numpy_walk(C0, Xc, kid, a, b, deg, theta, max_points):
    """The batched kernel's arithmetic in NumPy (round4_small.hip): kappa = phi + lam.u + lam.u with u = Phi00 lam / 2 - p,
    H = I + P G0^-1 P', right-looking Cholesky of both over the accepted sites, tau^2 = s_K / s_H from the running diagonals."""
    C0, Xc = np.asarray(C0, dtype=np.float64), np.asarray(Xc, dtype=np.float64).reshape(-1, np.asarray(C0).shape[1])
    n0, d = C0.shape
    mc = Xc.shape[0]
    if max_points is None or max_points <= 0:
        max_points = (d + 1) * (d + 2) // 2
    cap = min(mc, max_points - n0)
    if cap <= 0:
        return []
    thr = (theta ** 2) ** 2
    q = poly_dim(d, deg)
    Pi0, P = orc.poly_matrix(C0, deg), orc.poly_matrix(Xc, deg)
    T = np.linalg.solve(Pi0.T @ Pi0, P.T) if q else np.zeros((0, mc))
    Lam = Pi0 @ T
    Pk = orc.phi(kid, a, b, orc.pairwise_dist(C0, Xc))
    U = 0.5 * orc.phi(kid, a, b, orc.pairwise_dist(C0, C0)) @ Lam - Pk
    Kc = orc.phi(kid, a, b, orc.pairwise_dist(Xc, Xc))
    dK = np.diag(Kc) + 2.0 * np.sum(Lam * U, axis=0)
    dH = 1.0 + np.sum(P.T * T, axis=0)
    RK, RH, acc = np.zeros((cap, mc)), np.zeros((cap, mc)), []
    for j in range(mc):
        if len(acc) >= cap:
            break
        sK, sH = dK[j], dH[j]
        with np.errstate(all="ignore"):
            tau2 = sK / sH
        if not (sH > 0 and sK > 0 and tau2 > thr and tau2 < 1e300):
            continue
        r = len(acc)
        col = Kc[j] + Lam[:, j] @ U + U[:, j] @ Lam
        v = (col - RK[:r, j] @ RK[:r]) / math.sqrt(sK)
        w = ((P[j] @ T if q else np.zeros(mc)) - RH[:r, j] @ RH[:r]) / math.sqrt(sH)
        v[: j + 1] = 0.0
        w[: j + 1] = 0.0
        RK[r], RH[r] = v, w
        dK -= v * v
        dH -= w * w
        acc.append(j)
    return acc
