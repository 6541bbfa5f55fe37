"""Writes tests/golden/ds_host.npz: the host method of the directed-search direction (morbit.jl_amd/descent.py, _ds_active_set) on
the seeded QPs of every GPU shape (tests/ds_util.py: GPU_SHAPES x N_QP), and the measurement behind the device test's margin -- the
host method against itself with the columns of G (and x with them) permuted, which reorders every sum over the variables:
    ratio = max_i |z_a - z_b|_i / ((d + k) 2^-52 (sum_j |G_ij| + |r_i|)).
Needs no GPU and no library.  Takes some minutes (the host method is plain Python):  python tests/golden/make_ds_host.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from morbit.jl_amd import descent  # noqa: E402
from tests import ds_util  # noqa: E402


def main():
    out = {}
    worst = 0.0
    for d, k in ds_util.GPU_SHAPES:
        G, r, X, lb, ub = ds_util.make_batch(d, k)
        Z, om, status, iters, ratio = np.zeros((ds_util.N_QP, k)), np.zeros(ds_util.N_QP), [], [], np.zeros(ds_util.N_QP)
        perm = np.random.default_rng(d * 31 + k).permutation(d)
        for p in range(ds_util.N_QP):
            lo, hi = descent._sd_box(X[p], lb, ub)
            st = {}
            _, z, w, _, s = descent._ds_active_set(G[p], r[p], lo, hi, st)
            _, z2, _, _, s2 = descent._ds_active_set(G[p][:, perm], r[p], lo[perm], hi[perm])
            assert s == 0 and s2 == 0, (d, k, p, s, s2)
            Z[p], om[p] = z, w
            status.append(s), iters.append(st["iterations"])
            scale = (d + k) * ds_util.EPS * (np.abs(G[p]).sum(axis=1) + np.abs(r[p]))
            ratio[p] = float(np.max(np.abs(z - z2) / scale))
        key = "d%d_k%d" % (d, k)
        out[key + "_z"], out[key + "_omega"], out[key + "_iters"], out[key + "_ratio"] = Z, om, np.array(iters), ratio
        worst = max(worst, float(ratio.max()))
        print("%-10s iterations <= %.2f (d + k), ratio <= %.3g" % (key, max(iters) / (d + k), ratio.max()), flush=True)
    out["worst_ratio"] = np.array(worst)
    np.savez_compressed(ds_util.GOLDEN, **out)
    print("worst ratio %.3g -> margin %.3g" % (worst, 8 * worst))


if __name__ == "__main__":
    main()
