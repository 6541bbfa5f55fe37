"""Every output of the Pascoletti-Serafini entry points on seeded cases, into one .npz: run once per build of the library, the two
files compared byte for byte (a refactor of the step's host part must not change an output bit).

    python tools/ps_identity_dump.py --lib path/to/libmrbf.so --out dump.npz

Cases come from the builders of tests/test_gpu_ps_batch.py and tests/test_gpu_ideal_point.py: (d, n, k) = (3, 40, 2), (65, 131, 2),
(129, 259, 3); the two-model container with modelled constraints and linear rows; a critical start beside others.  Calls: mrbf_ps_step,
mrbf_ps_step_problem, mrbf_ps_step_batch, mrbf_ideal_point_problem and mrbf_ideal_point_batch with 1 and 9 starts, a given and a NULL
direction, polish 0 and 40, and one chunked run (MRBF_PS_CHUNK_KB=1).  Stored: every output array, every info field except ms_total,
and a hash of each model's coefficients (a difference in the fit is told apart from a difference in the step)."""
import argparse
import ctypes
import hashlib
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(3, 40, 2), (65, 131, 2), (129, 259, 3)]
NS = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    os.environ.setdefault("MRBF_EXPERIMENTS", "1")      # the gate of MRBF_PS_CHUNK_KB

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib
    import tests.test_gpu_ideal_point as tip
    import tests.test_gpu_ps_batch as tps

    out = {}

    def put(tag, arrays, infos, fields):
        for name, a in arrays:
            out["%s/%s" % (tag, name)] = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
        for f in fields:
            col = np.array([i[f] for i in infos], dtype=np.float64 if f == "tau" else np.int64)
            out["%s/info.%s" % (tag, f)] = col.view(np.uint64) if f == "tau" else col

    def put_models(tag, rows):
        for p, row in enumerate(rows):
            for j, m in enumerate(row):
                h = hashlib.sha256(np.ascontiguousarray(m.weights).tobytes() + np.ascontiguousarray(m.poly).tobytes()).digest()
                out["%s/model.%d.%d" % (tag, p, j)] = np.frombuffer(h, dtype=np.uint8)

    def steps(tag, rows, roles, k, X_n, LB, UB, FX, R, seeds, polishes, lin=None, eq_tol=-1.0):
        """the PS step through the single call (a loop) and the batch, 1 start and all of them, r given and not"""
        d = X_n.shape[1]
        for ns in (1, len(rows)):
            for given in (False, True):
                for polish in polishes:
                    a = (rows[:ns], roles, k, X_n[:ns], LB[:ns], UB[:ns], FX[:ns], R[:ns] if given else None, tps._opts(d, polish), seeds[:ns])
                    t = "%s/ns%d/given%d/polish%d" % (tag, ns, given, polish)
                    for name, got in (("problem", tps.single_loop(*a, lin=lin, eq_tol=eq_tol)), ("batch", tps.batch(*a, lin=lin, eq_tol=eq_tol))):
                        put("%s/%s" % (t, name), zip(("x_trial", "mx_trial", "r_out"), got[:3]), got[3], tps.INFO_FIELDS)

    def ideals(tag, rows, roles, k, X_n, LB, UB, seeds, lin=None, eq_tol=-1.0):
        d = X_n.shape[1]
        for ns in (1, len(rows)):
            a = (rows[:ns], roles, k, X_n[:ns], LB[:ns], UB[:ns], 4 * 20 * (d + 1), seeds[:ns])
            for name, got in (("problem", tip.ideal_loop(*a, lin=lin, eq_tol=eq_tol)), ("batch", tip.ideal_batch(*a, lin=lin, eq_tol=eq_tol))):
                put("%s/ns%d/ideal_%s" % (tag, ns, name), zip(("ideal", "x_ideal", "mx"), got[:3]), got[3], tip.INFO_FIELDS)

    def one_model_step(tag, m, x_n, lb, ub, fx, r, opts):
        """mrbf_ps_step: the entry for one model whose outputs are the objectives in order"""
        ctx, P = m.ctx, _lib.as_ptr
        xt, mt, ro, info = np.empty(x_n.size), np.empty(fx.size), np.empty(fx.size), _lib.PsInfo()
        arrs = [np.ascontiguousarray(a) for a in (x_n, lb, ub, fx)]
        rc = ctx.lib.mrbf_ps_step(ctx.h, tps._handle(m), *[P(a) for a in arrs], P(None if r is None else np.ascontiguousarray(r)), ctypes.byref(opts),
                                  P(xt), P(mt), P(ro), ctypes.byref(info))
        assert rc == 0, (tag, rc)
        put(tag, (("x_trial", xt), ("mx_trial", mt), ("r_out", ro)), [info.asdict()], tps.INFO_FIELDS)

    for d, n, k in SHAPES:
        tag = "d%d_n%d_k%d" % (d, n, k)
        if k == 2:
            c = tps.case(d, n, NS)
            roles = [0, 1]
        else:       # the ideal-point builder has the objective count; the values at x_n are the models' own, as in the other builder
            c = dict(tip.case(d, n, k))
            roles = c["roles"]
            c["FX"] = np.stack([pkg.eval_models_at_sites(c["rows"][p][0], None, c["X_n"][p][None, :])[0] for p in range(NS)])
            c["R"] = np.random.default_rng(31 * d + k).uniform(0.5, 1.5, (NS, k))
        put_models(tag, c["rows"])
        steps(tag, c["rows"], roles, k, c["X_n"], c["LB"], c["UB"], c["FX"], c["R"], c["seeds"], (0, 40))
        ideals(tag, c["rows"], roles, k, c["X_n"], c["LB"], c["UB"], c["seeds"])
        for given in (False, True):
            one_model_step("%s/ps_step/given%d" % (tag, given), c["rows"][0][0], c["X_n"][0], c["LB"][0], c["UB"][0], c["FX"][0],
                           c["R"][0] if given else None, tps._opts(d, 40, c["seeds"][0]))
        if d == 3:      # a critical start beside others; the batch in chunks of one start
            R = c["R"].copy()
            R[1, 0] = 0.0
            R[3, 1] = -0.25
            a = (c["rows"], roles, k, c["X_n"], c["LB"], c["UB"], c["FX"], R, tps._opts(d), c["seeds"])
            for name, got in (("problem", tps.single_loop(*a)), ("batch", tps.batch(*a))):
                put("%s/critical/%s" % (tag, name), zip(("x_trial", "mx_trial", "r_out"), got[:3]), got[3], tps.INFO_FIELDS)
            os.environ["MRBF_PS_CHUNK_KB"] = "1"
            try:
                got = tps.batch(*(a[:7] + (None,) + a[8:]))
                put("%s/chunked/batch" % tag, zip(("x_trial", "mx_trial", "r_out"), got[:3]), got[3], tps.INFO_FIELDS)
                got = tip.ideal_batch(c["rows"], roles, k, c["X_n"], c["LB"], c["UB"], 4 * 20 * (d + 1), c["seeds"])
                put("%s/chunked/ideal_batch" % tag, zip(("ideal", "x_ideal", "mx"), got[:3]), got[3], tip.INFO_FIELDS)
            finally:
                del os.environ["MRBF_PS_CHUNK_KB"]

    c = tip._constrained_case()
    X_n = c["X_n"]
    FX = np.stack([np.sum((X_n - 0.3) ** 2, axis=1), np.sum((X_n - 0.7) ** 2, axis=1)], axis=1)
    R = np.full((len(c["rows"]), 2), 1.0)
    put_models("container", c["rows"])
    steps("container", c["rows"], c["roles"], 2, X_n, c["LB"], c["UB"], FX, R, c["seeds"], (0, 40), lin=c["lin"], eq_tol=0.02)
    ideals("container", c["rows"], c["roles"], 2, X_n, c["LB"], c["UB"], c["seeds"], lin=c["lin"], eq_tol=0.02)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    keys = sorted(out)
    # an .npz as np.savez writes it, but with a fixed time stamp per member: equal arrays give equal bytes
    with zipfile.ZipFile(args.out, "w", zipfile.ZIP_STORED) as z:
        for key in keys:
            with z.open(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as f:
                np.lib.format.write_array(f, out[key], allow_pickle=False)
    print("ps_identity_dump: %d arrays, %d bytes of data, library %s" % (len(keys), sum(out[key].nbytes for key in keys), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
