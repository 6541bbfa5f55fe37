"""Many-start normal step at the C4 shape (d = 128, n = 257, cubic, degree-1 tail; one modelled inequality plus two linear rows): one
mrbf_normal_step_batch call against the loop of n_starts x mrbf_normal_step, for n_starts in {1, 8, 64}.

    python tools/normal_batch_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/normal_batch_bench.jsonl] [--reps 30]

Medians and ranges of `--reps` host-clock calls (every call ends in the library's own stream synchronisation), with the event time of
the same calls beside them.  --lib times another build of the library (the parent commit's, which has no batch entry: only the loop
is timed there -- the single call must not have become slower); one JSON line per (label, n_starts) is appended to --out.  The batch's
outputs are checked against the loop's (bit identity) before anything is timed; every shape is warmed up by that check."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_batch_bench.jsonl"))
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
    has_batch = hasattr(raw, "mrbf_normal_step_batch")
    if not has_batch:       # an earlier build: bind what it has, time the loop only
        for name in ("mrbf_normal_step_batch", "mrbf_dispatch_normal_batch"):
            _lib.SIGNATURES.pop(name, None)
    d, n = 128, 257
    starts = [int(s) for s in args.starts.split(",")]
    rng = np.random.default_rng(4)
    mcfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    scs = []
    for p in range(max(starts)):
        C = rng.uniform(-2.0, 2.0, (n, d))
        Y = C[:, :1] + 0.3 * np.sum(C ** 2, axis=1, keepdims=True) / d - 0.1
        scs.append(sg.SurrogateContainer(nl_ineq_constraints=[sg.RefSurrogate(pkg.update_model(mcfg, C, Y), [0])]))
    plans = [sg.container_plan(sc) for sc in scs]
    lin = (np.ones((1, d)) / d, np.array([0.05]), rng.standard_normal((1, d)) / np.sqrt(d), np.array([-0.2]))
    X = rng.uniform(-0.8, 0.8, (max(starts), d))
    deltas = np.full(max(starts), 0.3)
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)

    def loop(ns):
        out = []
        for p in range(ns):
            rc, nn, dl, info = descent.normal_step_device(plans[p], X[p], lb, ub, 0.3, lin)
            assert rc == 0, rc
            out.append((nn, info))
        return out

    def batch(ns):
        rc, N, X_n, recs, ms = descent.normal_step_batch_device(plans[:ns], X[:ns], lb, ub, deltas[:ns], lin)
        assert rc == 0, rc
        return N, X_n, recs, ms

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for ns in starts:
        ref = loop(ns)
        rec = {"tool": "normal_batch_bench", "label": args.label, "n_starts": ns, "d": d, "n": n, "rows": 3, "reps": args.reps,
               "iterations": [int(r[1]["iterations"]) for r in ref[:8]], "ok": int(sum(r[1]["status"] == _lib.NS_OK for r in ref))}
        if has_batch:
            N, X_n, recs, _ = batch(ns)
            same = all(np.array_equal(N[p], ref[p][0], equal_nan=True) and recs[p]["alpha"] == ref[p][1]["alpha"] and
                       recs[p]["iterations"] == ref[p][1]["iterations"] for p in range(ns))
            assert same, "the batch does not reproduce the single calls"
            rec["bit_identical"] = True
            host, ev = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r = batch(ns)
                host.append((time.perf_counter() - t0) * 1e3)
                ev.append(r[3])
            rec["batch_host_ms"] = float(np.median(host))
            rec["batch_event_ms"] = float(np.median(ev))
            rec["batch_host_ms_min_max"] = [float(np.min(host)), float(np.max(host))]
        host, ev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = loop(ns)
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(sum(x[1]["ms_total"] for x in r))
        rec["loop_host_ms"] = float(np.median(host))
        rec["loop_event_ms"] = float(np.median(ev))
        rec["loop_host_ms_min_max"] = [float(np.min(host)), float(np.max(host))]
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
