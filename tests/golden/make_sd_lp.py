"""Writes tests/golden/sd_lp.{json,npz}: direction LPs of _steepest_descent_direction (descent.jl:91-135) solved by HiGHS at
feasibility / optimality tolerances of 1e-10 (morbit.jl_amd/descent.py `_steepest_descent_direction`).

Each case: x, lb, ub (d), G (k x d, the rows g_i), A_eq / b_eq, A_ineq / b_ineq, normalize, and HiGHS' status (MRBF_SD_*) and
omega.  To keep the file small, x / lb / ub, G and the constraint matrices lie on a grid: every such array is q * s with q an int8
(int16 for G) array and s a power of two, both stored (keys <name>_q, <name>_s); q * s is exact in fp64, so the LPs the tests solve
are exactly the ones HiGHS solved here.  b_eq / b_ineq are stored as fp64.  Families: random boxes and gradients over d in {1, 2, 5, 12, 64, 256} x k in {1, 2, 3, 5, 8} x normalize on / off; x on lb
or ub (zero-width sides); l_j = u_j; duplicate and parallel gradient rows; a zero gradient row; all rows zero; critical points
(omega = 0); linear equality / inequality rows (b_ineq < 0 among them); rows that cannot be met; m = 64 rows; a few LPs at
d = 1024 and 4096.  Run from the repository root: python tests/golden/make_sd_lp.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from morbit.jl_amd import descent  # noqa: E402


QBITS = {"x": 8, "lb": 8, "ub": 8, "G": 16, "A_eq": 8, "A_ineq": 8}


def scale_of(v, bits):
    """the power of two s with |v| / s <= 2^(bits - 1) - 1"""
    top = float(np.max(np.abs(v))) if np.size(v) else 0.0
    return 1.0 if top == 0.0 else float(2.0 ** np.ceil(np.log2(top / (2 ** (bits - 1) - 1))))


def quant(v, bits=8):
    """v rounded to the grid of scale_of(v, bits): exactly representable as (int8 / int16) * power of two"""
    v = np.asarray(v, dtype=np.float64)
    s = scale_of(v, bits)
    return np.round(v / s) * s


def box(rng, d):
    lb = -rng.random(d) * 2.0
    ub = rng.random(d) * 2.0
    x = lb + rng.random(d) * (ub - lb)
    return quant_box(x, lb, ub)


def quant_box(x, lb, ub):
    """x, lb, ub on ONE grid, so that x == lb, x == ub, lb == ub survive"""
    s = scale_of(np.concatenate([x, lb, ub]), 8)
    return tuple(np.round(v / s) * s for v in (x, lb, ub))


def lin_rows(rng, d, x, lb, ub, meq, mineq, neg=False):
    lo, hi = descent._sd_box(x, lb, ub)
    d0 = lo + rng.random(d) * (hi - lo)          # a feasible direction: the rows can be met
    A_eq = quant(rng.standard_normal((meq, d)))
    b_eq = A_eq @ d0
    A_in = quant(rng.standard_normal((mineq, d)))
    b_in = A_in @ d0 + rng.random(mineq) * (0.0 if neg else 0.5)
    if neg and mineq:
        A_in[0] = np.abs(A_in[0])                # b < 0 with a feasible start of the box's interior
        b_in[0] = A_in[0] @ d0
    return A_eq, b_eq, A_in, b_in


def load(path_npz, path_json):
    """the cases as dicts with fp64 arrays (the tests' loader)"""
    arrs = np.load(path_npz)
    with open(path_json) as f:
        manifest = json.load(f)
    for c in manifest:
        for key, (kind, off, shape, sc) in c.pop("arrays").items():
            n = int(np.prod(shape))
            c[key] = arrs[kind][off:off + n].astype(np.float64).reshape(shape) * sc
    return manifest


def main():
    rng = np.random.default_rng(20261015)
    cases = []

    def add(tag, x, lb, ub, G, normalize, A_eq=None, b_eq=None, A_in=None, b_in=None):
        d = x.size
        x, lb, ub = quant_box(np.asarray(x, dtype=np.float64), np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64))
        G = quant(np.asarray(G, dtype=np.float64).reshape(-1, d), 16)
        A_eq = np.zeros((0, d)) if A_eq is None else np.asarray(A_eq, dtype=np.float64).reshape(-1, d)
        b_eq = np.zeros(0) if b_eq is None else np.asarray(b_eq, dtype=np.float64).ravel()
        A_in = np.zeros((0, d)) if A_in is None else np.asarray(A_in, dtype=np.float64).reshape(-1, d)
        b_in = np.zeros(0) if b_in is None else np.asarray(b_in, dtype=np.float64).ravel()
        dd, omega, status = descent._steepest_descent_direction(x, G, lb, ub, A_eq, b_eq, A_in, b_in, normalize, tol=1e-10,
                                                                want_status=True)
        cases.append(dict(tag=tag, x=x, lb=lb, ub=ub, G=G, A_eq=A_eq, b_eq=b_eq, A_ineq=A_in, b_ineq=b_in, normalize=bool(normalize),
                          status=int(status), omega=float(omega)))

    for d in (1, 2, 5, 12, 64, 256):
        for k in (1, 2, 3, 5, 8):
            for normalize in (True, False):
                x, lb, ub = box(rng, d)
                add("random", x, lb, ub, rng.standard_normal((k, d)) * 10.0 ** rng.uniform(-2, 2), normalize)
    for d in (2, 12, 64):
        for k in (2, 3):
            for normalize in (True, False):
                x, lb, ub = box(rng, d)
                x[::3] = lb[::3]
                x[1::3] = ub[1::3]
                add("x_on_bound", x, lb, ub, rng.standard_normal((k, d)), normalize)
                x, lb, ub = box(rng, d)
                lb[::2] = x[::2]
                ub[::2] = x[::2]
                add("l_eq_u", x, lb, ub, rng.standard_normal((k, d)), normalize)
                g = quant(rng.standard_normal((1, d)))
                add("duplicate_rows", *box(rng, d), np.vstack([g, g, 3.0 * g] + [rng.standard_normal((1, d))] * (k - 2)), normalize)
                Gz = rng.standard_normal((k, d))
                Gz[k - 1] = 0.0
                add("zero_row", *box(rng, d), Gz, normalize)
                add("all_zero", *box(rng, d), np.zeros((k, d)), normalize)
                g = quant(rng.standard_normal(d))
                add("critical", *box(rng, d), np.vstack([g, -2.0 * g] + [rng.standard_normal((1, d))] * (k - 2)), normalize)
    for d in (2, 5, 12, 64, 256):
        for (meq, mineq, neg) in ((1, 0, False), (0, 2, False), (2, 3, False), (0, 3, True), (1, 2, True)):
            if meq >= d:
                continue
            for normalize in (True, False):
                x, lb, ub = box(rng, d)
                k = int(rng.integers(1, 4))
                A_eq, b_eq, A_in, b_in = lin_rows(rng, d, x, lb, ub, meq, mineq, neg)
                add("linear", x, lb, ub, rng.standard_normal((k, d)), normalize, A_eq, b_eq, A_in, b_in)
    for d in (2, 12, 64):
        for normalize in (True, False):
            x, lb, ub = box(rng, d)
            a = np.ones((1, d))
            add("infeasible_eq", x, lb, ub, rng.standard_normal((2, d)), normalize, a, [3.0 * d])
            add("infeasible_ineq", x, lb, ub, rng.standard_normal((2, d)), normalize, None, None, np.vstack([a, -a]), [-1.0, -1.0])
            x, lb, ub = box(rng, d)
            lb[0] = x[0] + 1.5                  # x more than 1 below lb: the box max(-1, lb - x) .. min(1, ub - x) is empty
            ub[0] = lb[0] + 1.0
            add("empty_box", x, lb, ub, rng.standard_normal((2, d)), normalize)
    for d, k, meq, mineq in ((256, 8, 8, 48), (64, 4, 10, 50), (128, 64, 0, 0)):
        for normalize in (True, False):
            x, lb, ub = box(rng, d)
            A_eq, b_eq, A_in, b_in = lin_rows(rng, d, x, lb, ub, meq, mineq, False)
            add("m64", x, lb, ub, rng.standard_normal((k, d)), normalize, A_eq, b_eq, A_in, b_in)
    for d, k in ((1024, 2), (1024, 3), (4096, 2), (4096, 3)):
        x, lb, ub = box(rng, d)
        add("large", x, lb, ub, rng.standard_normal((k, d)), True)
    x, lb, ub = box(rng, 1024)
    A_eq, b_eq, A_in, b_in = lin_rows(rng, 1024, x, lb, ub, 2, 4, True)
    add("large_linear", x, lb, ub, rng.standard_normal((3, 1024)), False, A_eq, b_eq, A_in, b_in)

    # three flat arrays (int8, int16, fp64); the manifest holds every case's offsets, shapes and scales
    blobs = {"i8": [], "i16": [], "f64": []}
    fill = {"i8": 0, "i16": 0, "f64": 0}

    def put(kind, arr):
        off = fill[kind]
        blobs[kind].append(arr.ravel())
        fill[kind] += arr.size
        return [off, list(arr.shape)]

    manifest = []
    for i, c in enumerate(cases):
        entry = dict(idx=i, tag=c["tag"], d=int(c["x"].size), k=int(c["G"].shape[0]), m_eq=int(c["b_eq"].size),
                     m_ineq=int(c["b_ineq"].size), normalize=c["normalize"], status=c["status"],
                     omega=c["omega"] if np.isfinite(c["omega"]) else None, arrays={})
        for key in QBITS:
            v = np.asarray(c[key], dtype=np.float64)
            sc = scale_of(v, QBITS[key])
            q = v / sc
            assert np.array_equal(q, np.round(q)) and np.all(np.abs(q) < 2 ** (QBITS[key] - 1))
            kind = "i8" if QBITS[key] == 8 else "i16"
            entry["arrays"][key] = [kind] + put(kind, q.astype(np.int8 if kind == "i8" else np.int16)) + [sc]
        for key in ("b_eq", "b_ineq"):
            entry["arrays"][key] = ["f64"] + put("f64", np.asarray(c[key], dtype=np.float64)) + [1.0]
        manifest.append(entry)
    arrays = {kind: np.concatenate(v) if v else np.zeros(0) for kind, v in blobs.items()}
    g = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(g, "sd_lp.npz"), **arrays)
    with open(os.path.join(g, "sd_lp.json"), "w") as f:
        json.dump(manifest, f, separators=(",", ":"))
    print("%d LPs" % len(cases), {s: sum(c["status"] == s for c in cases) for s in (0, 1, 2)})


if __name__ == "__main__":
    main()
