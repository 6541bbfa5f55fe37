"""Many-start site selection at the C4 shape (d = 128, 300 and 1400 candidates per start, the filter's first pick taken on the host as
`collect()` does, d - 1 further picks wanted): one mrbf_affine_select_batch call against the loop of n_starts mrbf_affine_select calls,
for n_starts in {1, 8, 64}.

    python tools/affine_batch_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/affine_batch_bench.jsonl] [--reps 20]

Medians (and the spread: min, quartiles, max) of `--reps` host-clock calls, and the median of the batch call's event time.  --lib times
another build of the library (the parent commit's, which has no batch entry: only the loop is timed there); one JSON line per (label,
candidates, n_starts) is appended to --out.  The batch's outputs are checked against the loop's (bit identity) before anything is timed."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return {"median": float(q[2]), "min": float(q[0]), "q1": float(q[1]), "q3": float(q[3]), "max": float(q[4])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_batch_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--starts", default="1,8,64")
    ap.add_argument("--candidates", default="300,1400")
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, sampling

    raw = ctypes.CDLL(_lib.LIB_PATH)
    has_batch = hasattr(raw, "mrbf_affine_select_batch")
    if not has_batch:       # an earlier build: bind what it has, time the loop only
        for name in ("mrbf_affine_select_batch", "mrbf_dispatch_affine_batch"):
            _lib.SIGNATURES.pop(name, None)
    ctx = pkg.default_context()
    d, pivot = 128, 1e-3
    starts = [int(s) for s in args.starts.split(",")]
    i64p = ctypes.POINTER(ctypes.c_int64)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for mc in [int(s) for s in args.candidates.split(",")]:
        rng = np.random.default_rng(mc)
        S, Q0, picks, Z, npk = [], [], [], [], []
        for p in range(max(starts)):
            s = 0.1 * (2.0 * rng.random((mc, d)) - 1.0)
            i = int(np.argmax(np.abs(s).max(axis=1)))          # the first pick, on the host (sampling.AffinelyIndependentPointFilter.collect)
            qr = sampling._GrowingQR(d)
            qr.append(s[i].copy())
            s[i] = 0.0
            S.append(np.ascontiguousarray(s))
            Q0.append(np.asfortranarray(qr.Q))
            picks.append([np.empty(d, dtype=np.int64) for _ in range(2)])
            Z.append([np.empty(d * d) for _ in range(2)])
            npk.append(ctypes.c_int32(0))

        def loop(ns):
            for p in range(ns):
                ctx.check(ctx.lib.mrbf_affine_select(ctx.h, mc, d, _lib.as_ptr(S[p]), 1, _lib.as_ptr(Q0[p]), d - 1, pivot, 1,
                                                     picks[p][0].ctypes.data_as(i64p), ctypes.byref(npk[p]), _lib.as_ptr(Z[p][0])))

        jobs = (_lib.AffineJob * max(starts))() if has_batch else None
        if has_batch:
            for p in range(max(starts)):
                jobs[p].mc, jobs[p].j0, jobs[p].max_picks, jobs[p].pivot_val = mc, 1, d - 1, pivot
                jobs[p].shifted, jobs[p].Q0 = S[p].ctypes.data, Q0[p].ctypes.data
                jobs[p].picked_out, jobs[p].Z_out = picks[p][1].ctypes.data, Z[p][1].ctypes.data
        ms = ctypes.c_float(0.0)

        def batch(ns):
            ctx.check(ctx.lib.mrbf_affine_select_batch(ctx.h, ns, d, 1, jobs, ctypes.byref(ms)))
            return float(ms.value)

        for ns in starts:
            loop(ns)
            rec = {"tool": "affine_batch_bench", "label": args.label, "n_starts": ns, "d": d, "candidates": mc, "pivot": pivot,
                   "picks": [int(npk[p].value) for p in range(ns)][:4], "reps": args.reps}
            if has_batch:
                batch(ns)
                for p in range(ns):
                    n = npk[p].value
                    used = d * (d - 1 - n)
                    assert jobs[p].n_picked == n and np.array_equal(picks[p][0][:n], picks[p][1][:n]) and \
                        np.array_equal(Z[p][0][:used], Z[p][1][:used]), "the batch does not reproduce the single calls (start %d)" % p
                rec["bit_identical"] = True
                host, ev = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    e = batch(ns)
                    host.append((time.perf_counter() - t0) * 1e3)
                    ev.append(e)
                rec["batch_host_ms"] = spread(host)
                rec["batch_event_ms"] = float(np.median(ev))
            host = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                loop(ns)
                host.append((time.perf_counter() - t0) * 1e3)
            rec["loop_host_ms"] = spread(host)
            if has_batch:
                rec["batch_over_loop"] = rec["batch_host_ms"]["median"] / rec["loop_host_ms"]["median"]
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
