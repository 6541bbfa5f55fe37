"""Writes tests/golden/normal_lp.{json,npz}: LPs of compute_normal_step (descent.jl:691-757) solved by HiGHS at feasibility /
optimality tolerances of 1e-10 (morbit.jl_amd/descent.py `_normal_step_lp`, the explicit LP with its 2d band rows).

Each case: x, lb, ub (d), A_eq / b_eq, A_ineq / b_ineq (rows in the step n), and HiGHS' status (MRBF_NS_*), alpha* and row
multipliers y.  Every array lies on a power-of-two grid (8-bit integers times a power of two; right-hand sides 16-bit), so it is
exact in fp64 and the tests solve exactly the LPs HiGHS solved here.  Families: alpha* = 0 (x satisfies every row); one violated
row with a box that does not bind (closed form alpha* = -b / ||c||_1); equality rows only; mixed equality / inequality rows
(linear and modelled alike are just rows here) with m up to 64 over d in {1, 2, 3, 12, 64, 128, 256, 1024, 4096}; x on or near
the box's boundary; x outside the box; infinite box sides; infeasible systems (contradictory rows, rows that need to leave the
box, an empty box); degenerate systems (duplicate rows, zero rows with b >= 0 and b < 0, ties).  Each feasible case also carries
a (kappa_delta, delta_max) pair on one side of alpha* / kappa_delta.  Run from the repository root:
python tests/golden/make_normal_lp.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from morbit.jl_amd import descent  # noqa: E402

KEYS = ("x", "lb", "ub", "A_eq", "b_eq", "A_ineq", "b_ineq")


def quant(v, bits=8):
    """v rounded to a power-of-two grid with (bits)-bit integer mantissas (infinities kept)"""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    top = float(np.max(np.abs(v[fin]))) if fin.any() else 0.0
    s = 1.0 if top == 0.0 else float(2.0 ** np.ceil(np.log2(top / (2 ** (bits - 1) - 1))))
    out = v.copy()
    out[fin] = np.round(v[fin] / s) * s
    return out


def box(rng, d):
    lb = -rng.random(d) * 2.0
    ub = rng.random(d) * 2.0
    x = lb + rng.random(d) * (ub - lb)
    v = quant(np.concatenate([x, lb, ub]))
    return v[:d], v[d:2 * d], v[2 * d:]


def rows(rng, d, m, sparse=False):
    A = rng.standard_normal((m, d))
    if sparse:
        A *= rng.random((m, d)) < 0.3
    return quant(A)


def case(tag, x, lb, ub, A_eq, b_eq, A_in, b_in, closed=None):
    d = x.size
    A_eq, A_in = np.asarray(A_eq, dtype=np.float64).reshape(-1, d), np.asarray(A_in, dtype=np.float64).reshape(-1, d)
    b_eq, b_in = quant(np.asarray(b_eq, dtype=np.float64), 16), quant(np.asarray(b_in, dtype=np.float64), 16)
    return {"tag": tag, "x": x, "lb": lb, "ub": ub, "A_eq": A_eq, "b_eq": b_eq, "A_ineq": A_in, "b_ineq": b_in, "closed": closed}


def main():
    rng = np.random.default_rng(20261015)
    cases = []
    z = lambda d: np.zeros((0, d))
    e = np.zeros(0)
    # alpha* = 0: every row holds at x (n = 0)
    for d, m in ((2, 1), (12, 4), (64, 8), (1024, 3)):
        x, lb, ub = box(rng, d)
        A = rows(rng, d, m)
        cases.append(case("alpha0", x, lb, ub, z(d), e, A, rng.random(m) + 0.25))
    # one violated row, the box far away: alpha* = -b / ||c||_1
    for d in (1, 2, 3, 12, 64, 256, 1024, 4096):
        x, lb, ub = quant(rng.random(d) - 0.5), np.full(d, -64.0), np.full(d, 64.0)
        c = rows(rng, d, 1)
        c[0, 0] = c[0, 0] or 1.0
        b = -quant(rng.random(1) + 0.5, 16)
        cases.append(case("closed", x, lb, ub, z(d), e, c, b, closed=float(-b[0] / np.abs(c).sum())))
    # equality rows only
    for d, m in ((2, 1), (3, 2), (12, 5), (64, 16), (256, 8)):
        x, lb, ub = box(rng, d)
        cases.append(case("eq_only", x, lb, ub, rows(rng, d, m), rng.standard_normal(m) * 0.1, z(d), e))
    # mixed rows (linear and modelled rows are both rows here)
    for d in (1, 2, 3, 12, 64, 128, 256, 1024, 4096):
        for m in sorted({1, 2, 4, 8, 16, 64}):
            if d >= 1024 and m not in ((1, 4) if d == 1024 else (2,)):
                continue
            for rep in range(2 if d <= 128 else 1):
                x, lb, ub = box(rng, d)
                meq = int(rng.integers(0, min(m, d) + 1)) // 2
                Ae, Ai = rows(rng, d, meq), rows(rng, d, m - meq, d > 64)
                n0 = (lb - x) + rng.random(d) * (ub - lb) if rep == 0 else np.zeros(d)   # rep 0: rows met by a point of the box
                cases.append(case("mixed", x, lb, ub, Ae, Ae @ n0 if rep == 0 else rng.standard_normal(meq) * 0.05, Ai,
                                  Ai @ n0 + rng.random(m - meq) * 0.1 if rep == 0 else rng.standard_normal(m - meq) * 0.2))
    # x on / near the boundary
    for d, m in ((2, 1), (12, 3), (64, 6)):
        x, lb, ub = box(rng, d)
        on = rng.random(d) < 0.5
        x = np.where(on, np.where(rng.random(d) < 0.5, lb, ub), x)
        cases.append(case("on_bound", x, lb, ub, z(d), e, rows(rng, d, m), -rng.random(m) * 0.2))
    # x outside the box
    for d, m in ((1, 1), (3, 2), (12, 4), (128, 8)):
        x, lb, ub = box(rng, d)
        x = x + quant(np.where(rng.random(d) < 0.5, 3.0, -3.0) * (rng.random(d) < 0.5))
        cases.append(case("outside", x, lb, ub, z(d), e, rows(rng, d, m), rng.standard_normal(m) * 0.2))
        cases.append(case("outside_free", x, lb, ub, z(d), e, rows(rng, d, m), rng.random(m) * 50 + 50))
    # infinite box sides
    for d, m in ((2, 1), (12, 4), (64, 8), (256, 3)):
        x, lb, ub = box(rng, d)
        lb[rng.random(d) < 0.4] = -np.inf
        ub[rng.random(d) < 0.4] = np.inf
        cases.append(case("inf_box", x, lb, ub, rows(rng, d, 1), rng.standard_normal(1) * 0.2, rows(rng, d, m), rng.standard_normal(m) * 0.5))
    x, lb, ub = box(rng, 4)
    cases.append(case("inf_box", x, np.full(4, -np.inf), np.full(4, np.inf), z(4), e, rows(rng, 4, 2), -np.ones(2)))
    # infeasible: contradictory rows, rows that need to leave the box, an empty box
    for d in (2, 12, 64):
        x, lb, ub = box(rng, d)
        c = rows(rng, d, 1)
        cases.append(case("infeasible_rows", x, lb, ub, z(d), e, np.vstack([c, -c]), np.array([-0.5, -0.5])))
        cases.append(case("infeasible_eq", x, lb, ub, np.vstack([c, c]), np.array([0.25, -0.25]), z(d), e))
        cases.append(case("infeasible_box", x, lb, ub, z(d), e, np.ones((1, d)), np.array([float(np.sum(lb - x)) - 1.0])))
    x, lb, ub = box(rng, 3)
    lb[1], ub[1] = 0.5, -0.5
    cases.append(case("empty_box", x, lb, ub, z(3), e, np.ones((1, 3)), np.array([1.0])))
    # degenerate: duplicate rows, zero rows with b >= 0 / b < 0, ties
    for d in (3, 12, 64):
        x, lb, ub = box(rng, d)
        A = rows(rng, d, 3)
        cases.append(case("duplicate_rows", x, lb, ub, z(d), e, np.vstack([A, A, 2 * A[:1]]), np.concatenate([[-0.3, 0.1, -0.2]] * 2 + [[-0.6]])))
        cases.append(case("zero_row", x, lb, ub, z(d), e, np.vstack([A, np.zeros((2, d))]), np.array([-0.3, 0.1, -0.2, 0.0, 0.5])))
        cases.append(case("zero_row_infeasible", x, lb, ub, z(d), e, np.vstack([A, np.zeros((1, d))]), np.array([-0.3, 0.1, -0.2, -0.5])))
        cases.append(case("ties", np.zeros(d), -np.ones(d), np.ones(d), z(d), e, np.vstack([np.ones((1, d)), -np.ones((1, d))]),
                          np.array([-0.5, 0.5])))
    # solve, attach (kappa_delta, delta_max) pairs
    out, arrays = [], {}
    for i, c in enumerate(cases):
        n, alpha, status, y = descent._normal_step_lp(c["x"], c["lb"], c["ub"], c["A_eq"], c["b_eq"], c["A_ineq"], c["b_ineq"])
        meta = {"idx": i, "tag": c["tag"], "d": int(c["x"].size), "m_eq": int(c["b_eq"].size), "m_ineq": int(c["b_ineq"].size),
                "status": int(status), "alpha": None if status else alpha, "closed": c["closed"]}
        if status == 0:
            kappa = float(2.0 ** int(rng.integers(-2, 3)))
            r = alpha / kappa
            meta["kappa_delta"] = kappa
            meta["delta_max"] = float(quant(np.array([r * (2.0 if i % 2 else 0.5) + (0.0 if r > 0 or i % 2 else -1.0)]), 16)[0])
            arrays["%d_y" % i] = y
        for k in KEYS:
            arrays["%d_%s" % (i, k)] = c[k].astype(np.float32)   # exact: every value is on an 8- / 16-bit grid
        out.append(meta)
    g = os.path.dirname(os.path.abspath(__file__))
    np.savez_compressed(os.path.join(g, "normal_lp.npz"), **arrays)
    with open(os.path.join(g, "normal_lp.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(len(out), "cases;", sum(1 for c in out if c["status"]), "infeasible")


def load(path_npz, path_json):
    """the cases as dicts: the manifest's fields plus fp64 arrays (y only where HiGHS found an optimum)"""
    meta = json.load(open(path_json))
    z = np.load(path_npz)
    out = []
    for c in meta:
        c = dict(c)
        for k in KEYS:
            c[k] = z["%d_%s" % (c["idx"], k)].astype(np.float64)
        c["y"] = z["%d_y" % c["idx"]] if c["status"] == 0 else None
        out.append(c)
    return out


if __name__ == "__main__":
    main()
