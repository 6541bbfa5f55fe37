"""What the directed-search tests share (tests/test_ds_host.py, tests/test_gpu_ds.py, tests/golden/make_ds_host.py): the seeded QPs
of one shape, the checks of a returned solution, SLSQP on the same QP, and the stored host results of the GPU shapes."""
import os

import numpy as np

N_QP = 37
GPU_SHAPES = [(d, k) for d in (1, 2, 7, 63, 64, 65, 300) for k in (1, 2, 3, 5, 16)] + [(4096, 2)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ds_host.npz")
EPS = 2.0 ** -52


def make_qp(rng, d, k, p):
    """QP p of a batch: G (k x d), r (k) < 0, x, lb, ub (d).  p % 4: an interior site, half the coordinates on the lower bound, on the
    upper bound, on either; p % 5 == 3: a zero gradient row; p % 5 == 4: row 1 is row 0 doubled exactly; G and r scaled by 0.05, 1, 5;
    p % 7 in (3, 4) / (5, 6): r stretched by 3 sqrt(d) / by d, a target that the box keeps out of reach, so that bounds block and
    multipliers are dropped"""
    scale = (0.05, 1.0, 5.0)[p % 3]
    G = rng.standard_normal((k, d)) * scale
    r = -rng.uniform(0.05, 1.0, k) * scale * (1.0, 1.0, 1.0, 3.0 * np.sqrt(d), 3.0 * np.sqrt(d), float(d), float(d))[p % 7]
    lb, ub = np.zeros(d), np.ones(d)
    x = rng.uniform(0.1, 0.9, d)
    on = rng.random(d) < 0.5
    side = rng.random(d) < 0.5
    if p % 4 == 1:
        x[on] = 0.0
    elif p % 4 == 2:
        x[on] = 1.0
    elif p % 4 == 3:
        x[on] = np.where(side[on], 0.0, 1.0)
    if p % 5 == 3 and k >= 2:
        G[k - 1] = 0.0
    if p % 5 == 4 and k >= 2:
        G[1] = 2.0 * G[0]
    return G, r, x, lb, ub


def make_batch(d, k, n_qp=N_QP, seed=0):
    """the n_qp QPs of shape (d, k): G (n_qp x k x d), r (n_qp x k), X (n_qp x d), lb, ub (d)"""
    rng = np.random.default_rng(1000003 * seed + 1009 * d + k)
    qs = [make_qp(rng, d, k, p) for p in range(n_qp)]
    return (np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs]), np.stack([q[2] for q in qs]), qs[0][3], qs[0][4])


def value(G, r, d):
    return 0.5 * float(np.sum((G @ d - r) ** 2))


def slsqp(G, r, lo, hi):
    """(d, f) of SciPy's SLSQP on min 1/2 ||G d - r||^2, lo <= d <= hi, G d <= 0, from d = 0"""
    from scipy.optimize import minimize

    res = minimize(lambda v: value(G, r, v), np.zeros(G.shape[1]), jac=lambda v: G.T @ (G @ v - r), bounds=list(zip(lo, hi)),
                   constraints=[{"type": "ineq", "fun": lambda v: -(G @ v), "jac": lambda v: -G}], method="SLSQP",
                   options={"ftol": 1e-15, "maxiter": 1000})
    dd = np.clip(res.x, lo, hi)
    return dd, value(G, r, dd)


# The certificate's tolerance: the method accepts a multiplier within 1e-11 of the magnitudes it was formed from (DS_DUAL_TOL); mu and
# s = G' y carry the rounding of the k x k solves on top, cond(M) 2^-52 with cond(M) up to ~1e6 on these inputs (rows scaled alike,
# random columns): 1e-9 covers both.
KKT_TOL = 1e-9


def check_solution(G, r, lo, hi, d, z, omega, mu, tag=""):
    """the assertions of a status-OK solution: the box exactly, rows within 1e-13 sum_j |G_ij| (sd_lp.hip's FEAS_TOL and row scale),
    z and omega recomputed from d, and the KKT sign pattern of s = G' (z - r + mu) with complementarity"""
    assert np.all(d >= lo) and np.all(d <= hi), tag
    absG = np.abs(G)
    rowsum = absG.sum(axis=1)
    zz = G @ d
    assert np.all(zz <= 1e-13 * rowsum), (tag, zz, rowsum)
    n = d.size
    assert np.all(np.abs(z - zz) <= 4 * (n + 2) * EPS * (absG @ np.abs(d)) + 1e-300), (tag, z, zz)
    assert omega == max(0.0, -float(np.max(z))), (tag, omega, z)
    assert np.all(mu >= 0.0), (tag, mu)
    y = z - r + mu
    s = G.T @ y
    ysc = np.abs(z) + np.abs(r) + np.abs(mu)
    ssc = absG.T @ ysc
    free = (d > lo) & (d < hi)
    assert np.all(np.abs(s[free]) <= KKT_TOL * ssc[free]), (tag, "free", np.max(np.abs(s[free]) / ssc[free]))
    at_lo, at_hi = (d == lo) & (lo < hi), (d == hi) & (lo < hi)
    assert np.all(s[at_lo] >= -KKT_TOL * ssc[at_lo]), (tag, "lower")
    assert np.all(s[at_hi] <= KKT_TOL * ssc[at_hi]), (tag, "upper")
    assert np.all(np.abs(mu * z) <= KKT_TOL * ysc * ysc), (tag, "complementarity", mu, z)


# The margin of |z_dev - z_host|_i <= MARGIN (d + k) 2^-52 (sum_j |G_ij| + |r_i|): 8 x the largest ratio of the host method against
# itself with the columns of G permuted, which reorders its sums, on these same QPs (tests/golden/make_ds_host.py prints it and stores
# it as "worst_ratio": 3.603 at (d, k) = (7, 5), every other shape below 0.3; 8 x 3.603 = 28.82, rounded up).
MARGIN = 28.9


def z_bound(G, r):
    k, d = G.shape
    return MARGIN * (d + k) * EPS * (np.abs(G).sum(axis=1) + np.abs(r))


def load_golden():
    """the host method's z, omega, optimal value and iterations on make_batch(d, k) of every GPU shape, and the measured ratio of the
    host method against itself on permuted columns (tests/golden/make_ds_host.py)"""
    f = np.load(GOLDEN)
    return {k: f[k] for k in f.files}
