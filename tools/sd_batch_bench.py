"""Many-start steepest descent at the C4 shape (d = 128, n = 257, cubic, degree-1 tail, k = 2, default SteepestDescentConfig: 117 loops):
one mrbf_sd_iterate_batch call against the loop of n_starts x (mrbf_sd_criticality + mrbf_sd_step), for n_starts in {1, 8, 64}.

    python tools/sd_batch_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/sd_batch_bench.jsonl] [--reps 30]

Medians of `--reps` host-clock calls (and of the batch call's event time).  --lib times another build of the library (the parent
commit's, which has no batch entry: only the loop is timed there -- the single calls must not have become slower); one JSON line per
(label, n_starts) is appended to --out.  The batch's outputs are checked against the loop's (bit identity) before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sd_batch_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--starts", default="1,8,64")
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import ctypes

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg

    raw = ctypes.CDLL(_lib.LIB_PATH)
    has_batch = hasattr(raw, "mrbf_sd_iterate_batch")
    if not has_batch:       # an earlier build: bind what it has, time the loop only
        for name in ("mrbf_sd_iterate_batch", "mrbf_dispatch_sd_batch"):
            _lib.SIGNATURES.pop(name, None)
    d, n, k = 128, 257, 2
    starts = [int(s) for s in args.starts.split(",")]
    rng = np.random.default_rng(4)
    cfg = descent.SteepestDescentConfig()
    mcfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    scs = []
    for p in range(max(starts)):
        C = rng.uniform(-2.0, 2.0, (n, d))
        Y = np.stack([np.sum((C - 1.0) ** 2, axis=1), np.sum((C + 1.0) ** 2, axis=1)], axis=1)
        scs.append(sg.SurrogateContainer(objectives=[sg.RefSurrogate(pkg.update_model(mcfg, C, Y), [0, 1])]))
    plans = [sg.container_plan(sc) for sc in scs]
    X = rng.uniform(-1.0, 1.0, (max(starts), d))
    X_n = X + rng.uniform(-0.02, 0.02, X.shape)
    deltas = np.full(max(starts), 0.3)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)

    def loop(ns):
        out = []
        for p in range(ns):
            rc, om, dd, ci = descent.sd_criticality_device(plans[p], X[p], X_n[p], lb, ub, cfg.normalize)
            assert rc == 0, rc
            rc, xp, mxp, si = descent.sd_step_device(plans[p], cfg, X[p], X_n[p], 0.3, lb, ub, om, dd)
            assert rc == 0, rc
            out.append((dd, xp, mxp, ci["ms_total"] + si["ms_total"]))
        return out

    def batch(ns):
        rc, D, XP, MXP, recs, ms = descent.sd_iterate_batch_device(plans[:ns], cfg, X[:ns], X_n[:ns], deltas[:ns], lb, ub)
        assert rc == 0, rc
        return D, XP, MXP, recs, ms

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for ns in starts:
        ref = loop(ns)
        rec = {"tool": "sd_batch_bench", "label": args.label, "n_starts": ns, "d": d, "n": n, "k": k, "max_loops": cfg.max_loops,
               "reps": args.reps}
        if has_batch:
            D, XP, MXP, recs, _ = batch(ns)
            same = all(np.array_equal(D[p], ref[p][0]) and np.array_equal(XP[p], ref[p][1]) and np.array_equal(MXP[p], ref[p][2])
                       for p in range(ns))
            assert same, "the batch does not reproduce the chained single calls"
            rec["bit_identical"] = True
            host, ev = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r = batch(ns)
                host.append((time.perf_counter() - t0) * 1e3)
                ev.append(r[4])
            rec["batch_host_ms"] = float(np.median(host))
            rec["batch_event_ms"] = float(np.median(ev))
            rec["batch_host_ms_min_max"] = [float(np.min(host)), float(np.max(host))]
        host, ev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = loop(ns)
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(sum(x[3] for x in r))
        rec["loop_host_ms"] = float(np.median(host))
        rec["loop_event_ms"] = float(np.median(ev))
        rec["loop_host_ms_min_max"] = [float(np.min(host)), float(np.max(host))]
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
