"""Extended-precision truth for the one-launch LU (tests/test_gpu_small_lu.py)  ->  tests/golden/lu_truth.npz.

The fixture grid (rbf_golden.npz) has 21 cases on the LU path, all of them small.  This script adds saddle systems at the sizes where
the blocked LU of small_lu.hip changes what it does -- N = n + q in {2, 15, 16, 17, 33, 65, 129, 190}: below, at and above one
16-column panel, several panels, a padded last panel -- at d in {1, 3, 65} and for the kernel / tail pairs that take the LU path:
thin plate spline k = 2 with a linear tail, cubic 3 with a constant and with no tail, cubic 5 with a linear tail, multiquadric without
a tail; one case has n == q.  Sites are uniform in [-2, 2]^d, values two parabolas (+ a linear term), seeds fixed.

Each system  [Phi Pi; Pi' 0][w; lam] = [Y; 0]  is assembled from the fp64 sites / values taken as exact rationals and solved with mpmath
at 60 significant digits (pivoted LU), exactly as tests/golden/make_truth.py does; its radial functions and its hi + lo storage are
imported from there.  No code of the product or of the fp64 oracle is imported.  The tests only read the .npz.

Run:  python tests/golden/make_lu_truth.py
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_truth import DIGITS, flatten, hi_lo, solve_case  # noqa: E402

# name: (kernel id, a, b, polynomial degree)
PAIRS = {
    "tps2_deg1": (3, 2.0, 0.0, 1),
    "cubic3_deg0": (0, 3.0, 0.0, 0),
    "cubic3_degm1": (0, 3.0, 0.0, -1),
    "cubic5_deg1": (0, 5.0, 0.0, 1),
    "mq_degm1": (2, 1.0, 0.5, -1),
}
# (pair, d, N = n + q, k)
CASES = [
    ("cubic3_deg0", 1, 2, 1),      # n == q == 1
    ("mq_degm1", 1, 17, 2),
    ("cubic3_degm1", 1, 33, 2),
    ("tps2_deg1", 1, 65, 2),
    ("cubic3_degm1", 3, 15, 2),
    ("cubic3_deg0", 3, 16, 2),
    ("tps2_deg1", 3, 17, 3),
    ("cubic5_deg1", 3, 33, 2),
    ("mq_degm1", 3, 65, 2),
    ("tps2_deg1", 3, 129, 1),
    ("cubic3_deg0", 65, 129, 2),
    ("mq_degm1", 65, 129, 2),
    ("tps2_deg1", 65, 190, 2),
    ("cubic5_deg1", 65, 190, 1),
]


def case_data(pair, d, N, k):
    kid, a, b, deg = PAIRS[pair]
    q = 0 if deg < 0 else (1 if deg == 0 else d + 1)
    n = N - q
    assert n >= q, (pair, d, N)
    rng = np.random.default_rng(1000 * N + 10 * d + kid)
    C = rng.uniform(-2.0, 2.0, (n, d))
    Y = np.stack([np.sum((C - 1.0) ** 2, axis=1), np.sum((C + 1.0) ** 2, axis=1) + C[:, 0], np.sum(C, axis=1)], axis=1)[:, :k]
    return C, np.ascontiguousarray(Y), kid, a, b, deg


def main():
    mp.mp.dps = DIGITS
    arrays = {}
    for idx, (pair, d, N, k) in enumerate(CASES):
        C, Y, kid, a, b, deg = case_data(pair, d, N, k)
        n = C.shape[0]
        q = N - n
        W, Lam, _, _, resn = solve_case(C, Y, np.zeros((0, d)), kid, a, b, deg)
        pre = "c%03d_" % idx
        arrays[pre + "C"], arrays[pre + "Y"] = C, Y
        arrays[pre + "kernel"] = np.array([kid, a, b, deg], dtype=np.float64)
        for key, val, shape in (("W", W, (n, k)), ("Lam", Lam, (q, k))):
            arrays[pre + key + "_hi"], arrays[pre + key + "_lo"] = hi_lo(flatten(val), shape)
        print("%-14s d %3d N %3d n %3d k %d  (mp residual %.1e)" % (pair, d, N, n, k, float(resn)), flush=True)
    arrays["count"] = np.array([len(CASES)])
    np.savez_compressed(os.path.join(HERE, "lu_truth.npz"), **arrays)
    print("wrote %d cases" % len(CASES))


if __name__ == "__main__":
    main()
