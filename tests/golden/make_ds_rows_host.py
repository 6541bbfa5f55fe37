"""Writes tests/golden/ds_rows_host.npz: the host mirror of the directed-search direction with constraint rows (morbit.jl_amd/descent.py,
_ds_active_set_rows) on the seeded QPs of every GPU shape (tests/ds_rows_util.py: GPU_SHAPES x N_QP), and the measurement behind the
device test's margin -- the host mirror against itself with the columns of W = [G; A_eq; A_in] (and the box with them) permuted, which
reorders every sum over the variables:
    ratio = max_i |z_a - z_b|_i / ((d + K) 2^-52 (sum_j |G_ij| + |r_i|)).
Asserts that no QP gives up and prints the worst certificate residual.  With --slsqp it writes nothing and prints, per CPU shape, the
host mirror's worst excess (f - f_SLSQP) / (1 + f) over SciPy's SLSQP on 10 QPs and how many QPs SLSQP failed on (the numbers behind
ds_rows_util.SLSQP_TAU).  Needs no GPU and no library.  Takes some minutes (the host mirror is plain Python):
    python tests/golden/make_ds_rows_host.py [--slsqp]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from morbit.jl_amd import descent  # noqa: E402
from tests import ds_rows_util as ru  # noqa: E402


def slsqp_excess():
    worst_all = -np.inf
    for d, k, m_eq, m_in in ru.CPU_SHAPES:
        G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(d, k, m_eq, m_in, n_qp=10)
        worst, skipped = -np.inf, 0
        for p in range(10):
            lo, hi = descent._sd_box(X[p], lb, ub)
            dd, _, _, _, s = descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p])
            assert s == 0, (d, k, m_eq, m_in, p, s)
            ds = descent._ds_slsqp(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p])
            if ds is None:
                skipped += 1
                continue
            f, fs = ru.value(G[p], r[p], dd), ru.value(G[p], r[p], ds)
            worst = max(worst, (f - fs) / (1 + f))
        worst_all = max(worst_all, worst)
        print("%-16s (f - f_SLSQP) / (1 + f) <= %.3g, SLSQP failed on %d of 10" % (ru.key(d, k, m_eq, m_in), worst, skipped), flush=True)
    print("worst excess %.3g -> SLSQP_TAU %.3g" % (worst_all, 2 * worst_all))


def main():
    out = {}
    worst, kkt = 0.0, 0.0
    for d, k, m_eq, m_in in ru.GPU_SHAPES:
        K = k + m_eq + m_in
        G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(d, k, m_eq, m_in)
        Z, om, val, ratio = np.zeros((ru.N_QP, k)), np.zeros(ru.N_QP), np.zeros(ru.N_QP), np.zeros(ru.N_QP)
        status, iters = [], []
        perm = np.random.default_rng(d * 31 + K).permutation(d)
        for p in range(ru.N_QP):
            lo, hi = descent._sd_box(X[p], lb, ub)
            st = {}
            dd, c, w, mu, s = descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p], st)
            _, c2, _, _, s2 = descent._ds_active_set_rows(G[p][:, perm], r[p], lo[perm], hi[perm], Ae[p][:, perm], be[p], Ai[p][:, perm], bi[p])
            assert s == 0 and s2 == 0, (d, k, m_eq, m_in, p, s, s2, st)    # zero give-ups
            kkt = max(kkt, ru.check_solution(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p], dd, c, w, mu, (d, k, m_eq, m_in, p)))
            Z[p], om[p], val[p] = c[:k], w, ru.value(G[p], r[p], dd)
            status.append(s), iters.append(st["iterations"])
            scale = (d + K) * ru.EPS * (np.abs(G[p]).sum(axis=1) + np.abs(r[p]))
            ratio[p] = float(np.max(np.abs(c[:k] - c2[:k]) / scale))
        kk = ru.key(d, k, m_eq, m_in)
        out[kk + "_z"], out[kk + "_omega"], out[kk + "_value"], out[kk + "_ratio"] = Z, om, val, ratio
        out[kk + "_iters"], out[kk + "_status"] = np.array(iters), np.array(status)
        worst = max(worst, float(ratio.max()))
        print("%-18s iterations <= %.2f (d + K), ratio <= %.3g" % (kk, max(iters) / (d + K), ratio.max()), flush=True)
    out["worst_ratio"] = np.array(worst)
    np.savez_compressed(ru.GOLDEN, **out)
    print("worst ratio %.3g -> margin %.3g; worst certificate residual %.3g" % (worst, 8 * worst, kkt))


if __name__ == "__main__":
    slsqp_excess() if "--slsqp" in sys.argv[1:] else main()
