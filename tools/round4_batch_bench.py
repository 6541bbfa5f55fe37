"""Many-start round 4 at the many-start shape (d = 128, degree-1 tail, cubic kernel, n0 = 129 start sites, max_points = 257, 300 and
1400 candidates per start, host arrays as the bindings pass them): one mrbf_round4_batch call against the loop of n_starts x
mrbf_round4 (no state kept), for n_starts in {1, 8, 64}.

    python tools/round4_batch_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/round4_batch_bench.jsonl] [--reps 20]
    rocprofv3 --kernel-trace --stats -d DIR -o r4b --output-format csv -- python tools/round4_batch_bench.py --trace
    python tools/round4_batch_bench.py --summarise DIR/.../r4b_kernel_trace.csv --out profiles/round4_batch_kernel_stats.csv

Medians of `--reps` host-clock calls after a warm-up call, with the fastest and slowest beside them and the event time of the batched
chain (ms_total).  --lib times another build of the library (the parent commit's, which has no batch entry: only the loop is timed
there); one JSON line per (label, candidates, n_starts) is appended to --out.  The batch's lists are asserted equal to the loop's
before anything is timed.  --trace: one batch call at 8 and one at 64 starts (300 candidates) and nothing else, for a kernel trace;
--summarise turns that trace into launches per kernel and call.  One GPU process; run one label at a time."""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, N0, MAX_POINTS, DEG = 128, 129, 257, 1


def summarise(trace, out):
    """launches per kernel of the two batch calls of a --trace run: the dispatches in time order, split where the second call's first
    launch (the clearing of its output words, in front of r4s_ginv_kernel) begins"""
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    first = [i for i, n in enumerate(names) if "r4s_ginv_kernel" in n]
    assert len(first) == 2, "expected two batch calls in the trace, found %d" % len(first)
    head = first[0]                      # dispatches in front of the first ginv launch belong to the first call
    cut = first[1] - head
    calls = {8: names[:cut], 64: names[cut:]}
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["n_starts", "kernel", "launches"])
        for ns, ks in calls.items():
            seen = []
            for k in ks:
                if k not in seen:
                    seen.append(k)
            for k in seen:
                w.writerow([ns, k.split("(")[0], ks.count(k)])
            w.writerow([ns, "TOTAL", len(ks)])
    print(open(out).read())
    assert len(calls[8]) == len(calls[64]), "the launch count of a batch call depends on the number of starts"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--starts", default="1,8,64")
    ap.add_argument("--cands", default="300,1400")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.out or os.path.join(ROOT, "profiles", "round4_batch_kernel_stats.csv"))
    out = args.out or os.path.join(ROOT, "profiles", "round4_batch_bench.jsonl")
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

    has_batch = hasattr(ctypes.CDLL(_lib.LIB_PATH), "mrbf_round4_batch")
    if not has_batch:       # an earlier build: bind what it has, time the loop only
        for name in ("mrbf_round4_batch", "mrbf_dispatch_round4_batch"):
            _lib.SIGNATURES.pop(name, None)
    ctx = pkg.Context()
    lib = ctx.lib
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel="cubic", polynomial_degree=DEG))
    theta = 1e-7
    starts = [int(s) for s in args.starts.split(",")]
    cands = [int(s) for s in args.cands.split(",")]
    P = max(starts)
    rng = np.random.default_rng(4)
    x = np.full(D, 0.5)
    C0s = [np.vstack([x, x + 0.3 * np.eye(D) * np.where(np.arange(D) % 2 == 0, 1.0, -1.0) + 0.01 * rng.standard_normal((D, D))]) for _ in range(P)]
    Xall = [x + 0.6 * (rng.random((max(cands), D)) - 0.5) for _ in range(P)]
    acc = [np.zeros(MAX_POINTS - N0, dtype=np.int32) for _ in range(P)]

    def loop(ns, mc):
        got = []
        for p in range(ns):
            na = ctypes.c_int32()
            ctx.check(lib.mrbf_round4(ctx.h, N0, D, _lib.as_ptr(C0s[p]), mc, _lib.as_ptr(Xs[p]), kid, a, b, DEG, MAX_POINTS, theta, _lib.as_ptr(acc[p]),
                                      ctypes.byref(na), None))
            got.append(acc[p][: na.value].tolist())
        return got, 0.0

    def batch(ns, mc):
        jobs = (_lib.Round4Job * ns)()
        for p in range(ns):
            J = jobs[p]
            J.n0, J.mc, J.start_sites, J.cand_sites = N0, mc, C0s[p].ctypes.data, Xs[p].ctypes.data
            J.kernel_id, J.poly_deg, J.a, J.b, J.max_points, J.theta_pivot_cholesky, J.accepted_out = kid, DEG, a, b, MAX_POINTS, theta, acc[p].ctypes.data
        ms = ctypes.c_float()
        ctx.check(lib.mrbf_round4_batch(ctx.h, ns, D, jobs, ctypes.byref(ms)))
        assert all(J.rc == 0 for J in jobs)
        return [acc[p][: jobs[p].n_accepted].tolist() for p in range(ns)], ms.value

    def timed(f, ns, mc):
        f(ns, mc)                                     # warm-up
        host, ev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, e = f(ns, mc)
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(e)
        return float(np.median(host)), float(np.median(ev)), [float(np.min(host)), float(np.max(host))]

    if args.trace:
        Xs = [np.ascontiguousarray(X[:300]) for X in Xall]
        batch(8, 300)
        batch(64, 300)
        ctx.close()
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for mc in cands:
        Xs = [np.ascontiguousarray(X[:mc]) for X in Xall]
        for ns in starts:
            rec = {"tool": "round4_batch_bench", "label": args.label, "n_starts": ns, "candidates": mc, "d": D, "n0": N0, "max_points": MAX_POINTS,
                   "reps": args.reps}
            want, _ = loop(ns, mc)
            rec["accepted"] = [len(w) for w in want[:2]]
            if has_batch:
                got, _ = batch(ns, mc)
                assert got == want, "the batch's lists differ from the loop's"
                rec["identical_lists"] = True
                rec["batch_host_ms"], rec["batch_event_ms"], rec["batch_host_ms_min_max"] = timed(batch, ns, mc)
            rec["loop_host_ms"], _, rec["loop_host_ms_min_max"] = timed(loop, ns, mc)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
