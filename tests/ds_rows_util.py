"""What the tests of directed search with constraint rows share (tests/test_ds_rows_host.py, tests/test_gpu_ds_rows.py,
tests/golden/make_ds_rows_host.py): the seeded QPs of one shape -- ds_util.make_qp plus constraint rows --, the checks of a returned
solution, and the stored host results of the GPU shapes."""
import os

import numpy as np

from tests import ds_util

N_QP = ds_util.N_QP
EPS = ds_util.EPS
ROW_SETS = [(1, 0, 1), (1, 1, 0), (2, 1, 1), (3, 0, 2), (2, 2, 3), (5, 3, 8), (1, 0, 15)]     # (k, m_eq, m_in)
CPU_SHAPES = [(d,) + rs for d in (1, 2, 3, 7, 30, 64, 65, 130) for rs in ROW_SETS if rs[1] <= d - 1]
GPU_SHAPES = [(d,) + rs for d in (1, 2, 7, 63, 64, 65, 300) for rs in ROW_SETS if rs[1] <= d - 1] + [(4096, 2, 1, 1)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ds_rows_host.npz")
FEAS_TOL = 1e-13


def make_qp(rng, d, k, m_eq, m_in, p):
    """QP p of a batch: ds_util.make_qp's G, r, x, lb, ub and rows A_eq (m_eq x d), A_in (m_in x d) with random entries scaled like G;
    b_eq = 0 (the start d = 0 satisfies the equalities), b_in a mix of 0 (active at the start) and positive slack"""
    G, r, x, lb, ub = ds_util.make_qp(rng, d, k, p)
    scale = (0.05, 1.0, 5.0)[p % 3]
    A_eq = rng.standard_normal((m_eq, d)) * scale
    A_in = rng.standard_normal((m_in, d)) * scale
    b_eq = np.zeros(m_eq)
    b_in = np.where(rng.random(m_in) < 0.5, 0.0, rng.uniform(0.05, 1.0, m_in) * scale)
    return G, r, x, lb, ub, A_eq, b_eq, A_in, b_in


def make_batch(d, k, m_eq, m_in, n_qp=N_QP, seed=0):
    """the n_qp QPs of one shape: G (n_qp x k x d), r, X, lb, ub (d), A_eq (n_qp x m_eq x d), b_eq, A_in (n_qp x m_in x d), b_in"""
    rng = np.random.default_rng(1000003 * seed + 1009 * d + 97 * k + 13 * m_eq + m_in)
    qs = [make_qp(rng, d, k, m_eq, m_in, p) for p in range(n_qp)]
    st = lambda i: np.stack([q[i] for q in qs])
    return st(0), st(1), st(2), qs[0][3], qs[0][4], st(5), st(6), st(7), st(8)


def key(d, k, m_eq, m_in):
    return "d%d_k%d_e%d_i%d" % (d, k, m_eq, m_in)


def value(G, r, d):
    return ds_util.value(G, r, d)


# The certificate's tolerance is ds_util.KKT_TOL (1e-9): measured on CPU_SHAPES x 10 QPs and GPU_SHAPES x 37 QPs, the host mirror's worst
# residual of any certificate line, relative to the magnitudes it was formed from, is printed by tests/golden/make_ds_rows_host.py and
# stays below it.
KKT_TOL = ds_util.KKT_TOL

# f <= f_SLSQP + SLSQP_TAU (1 + f): 2 x the host mirror's own worst excess over SLSQP on the stored batch (CPU_SHAPES x 10 QPs),
# measured by   python tests/golden/make_ds_rows_host.py --slsqp   (prints the worst excess per shape; SLSQP accepts rows within 1e-9,
# so its point may undercut the optimum by about that much).
SLSQP_TAU = 1.1e-9   # measured worst excess 5.21e-10 at (d; k, m_eq, m_in) = (30; 3, 0, 2); SLSQP failed on at most 1 of 10 QPs of a shape


def check_solution(G, r, lo, hi, A_eq, b_eq, A_in, b_in, d, c, omega, mu, tag="", kkt_tol=KKT_TOL, h=None):
    """the assertions of a status-OK solution: the box exactly, every row within FEAS_TOL (sum_j |W_ij| + |h_i|) of the (clamped)
    right-hand side h, c and omega recomputed from d, and the certificate -- s = W' y zero on free variables, >= 0 at the lower and
    <= 0 at the upper bound, mu >= 0 on objective and inequality rows, mu_i (h_i - c_i) = 0.  Returns the worst certificate residual
    relative to its scale."""
    k, m_eq = G.shape[0], A_eq.shape[0]
    W = np.vstack([G, A_eq, A_in])
    K, n = W.shape
    if h is None:
        h = np.concatenate([np.zeros(k), b_eq, b_in])
    absW = np.abs(W)
    rowsum = absW.sum(axis=1)
    is_eq = (np.arange(K) >= k) & (np.arange(K) < k + m_eq)
    assert np.all(d >= lo) and np.all(d <= hi), tag
    cc = W @ d
    miss = np.where(is_eq, np.abs(cc - h), cc - h)
    assert np.all(miss <= FEAS_TOL * (rowsum + np.abs(h))), (tag, miss, rowsum)
    assert np.all(np.abs(c - cc) <= 4 * (n + 2) * EPS * (absW @ np.abs(d)) + 1e-300), (tag, c, cc)
    assert omega == max(0.0, -float(np.max(c[:k]))), (tag, omega, c)
    rext = np.concatenate([r, np.zeros(K - k)])
    zext = np.where(np.arange(K) < k, c, 0.0)
    mscale = float(np.max(np.abs(r) + np.abs(c[:k])))     # the scale the method judges a multiplier's sign on
    assert np.all(mu[~is_eq] >= -kkt_tol * mscale), (tag, mu)
    y = zext - rext + mu
    s = W.T @ y
    ysc = np.abs(zext) + np.abs(rext) + np.abs(mu)
    ssc = absW.T @ ysc
    free = (d > lo) & (d < hi)
    at_lo, at_hi = (d == lo) & (lo < hi), (d == hi) & (lo < hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ssc > 0, s / ssc, 0.0)
    worst = max(float(np.max(-mu[~is_eq], initial=0.0)) / mscale, float(np.max(np.abs(rel[free]), initial=0.0)), float(np.max(-rel[at_lo], initial=0.0)), float(np.max(rel[at_hi], initial=0.0)))
    assert np.all(np.abs(s[free]) <= kkt_tol * ssc[free]), (tag, "free", worst)
    assert np.all(s[at_lo] >= -kkt_tol * ssc[at_lo]), (tag, "lower", worst)
    assert np.all(s[at_hi] <= kkt_tol * ssc[at_hi]), (tag, "upper", worst)
    # complementarity on the scale of the row: |mu_i| (|c_i| + |h_i| + rowsum_i) -- the slack of a row of S is rounding of that size
    cscale = (ysc + np.abs(mu)) * (np.abs(c) + np.abs(h) + rowsum)
    comp = np.abs(mu * (h - c))
    assert np.all(comp <= kkt_tol * cscale), (tag, "complementarity", mu, h - c)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = max(worst, float(np.max(np.where(cscale > 0, comp / cscale, 0.0), initial=0.0)))
    return worst


def z_bound(G, r, K, margin):
    """|z_dev - z_host|_i <= margin (d + K) 2^-52 (sum_j |G_ij| + |r_i|)"""
    d = G.shape[1]
    return margin * (d + K) * EPS * (np.abs(G).sum(axis=1) + np.abs(r))


def load_golden():
    """the host mirror's z, omega, optimal value, status and iterations on make_batch of every GPU shape, and "worst_ratio": the host
    mirror against itself on permuted columns (tests/golden/make_ds_rows_host.py)"""
    f = np.load(GOLDEN)
    return {k: f[k] for k in f.files}
