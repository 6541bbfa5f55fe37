"""Many-start directed search: one mrbf_ds_iterate_batch call against the per-start loop mrbf_ds_criticality -> host normalisation ->
mrbf_sd_step, at (d, k, n_starts) = (64, 2, 1), (128, 2, 64), (256, 3, 256); n = 257 centres per model (cubic, degree-1 tail, built
from coefficients: no fit), max_loops = 117, targets inside reach so that the QPs end after a few iterations on both sides.

    python tools/ds_batch_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/ds_batch_bench.jsonl] [--reps 20]
    python tools/ds_batch_bench.py --calls 5 --shape 1 [--starts 8]    # only that many batch calls of one shape: for a kernel trace

The batch call is timed by its event time (ms_total) on device-resident inputs and by the host clock; the loop by the host clock and
by the sum of its calls' event times; medians of --reps calls after 3 warm-up calls.  --lib times another build of the library (the
parent commit's, which has no batch entry: only the loop is timed there); one JSON line per (label, shape) is appended to --out.  The
batch's outputs are checked against the loop's (bit identity) before anything is timed.  The launch count of a batch call comes from
a kernel trace of two --calls runs: (dispatches with 15 calls - dispatches with 5 calls) / 10."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 2, 1), (128, 2, 64), (256, 3, 256)]
N_CENTRES = 257


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ds_batch_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--shape", type=int, default=-1)
    ap.add_argument("--starts", type=int, default=0, help="with --shape: another number of starts at that shape's (d, k)")
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import ctypes

    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import rbf_model as rm
    from morbit.jl_amd import surrogates as sg

    raw = ctypes.CDLL(_lib.LIB_PATH)
    has_batch = hasattr(raw, "mrbf_ds_iterate_batch")
    if not has_batch:       # an earlier build: bind what it has, time the loop only
        for name in ("mrbf_ds_iterate_batch", "mrbf_dispatch_ds_batch"):
            _lib.SIGNATURES.pop(name, None)
    cfg = descent.DirectedSearchConfig(reference_point=[0.0])
    assert cfg.max_loops == 117
    mcfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shapes = SHAPES if args.shape < 0 else [SHAPES[args.shape][:2] + (args.starts or SHAPES[args.shape][2],)]
    for d, k, ns in shapes:
        rng = np.random.default_rng(1000 * d + ns)
        scs = []
        for p in range(ns):
            C = rng.uniform(0.0, 1.0, (N_CENTRES, d))
            W = rng.standard_normal((N_CENTRES, k)) * 0.05 / N_CENTRES
            mod = rm.model_from_coeffs(mcfg, C, W, rng.standard_normal((d + 1, k)))
            scs.append(sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, list(range(k)))]))
        plans = [sg.container_plan(sc) for sc in scs]
        X_n = rng.uniform(0.1, 0.9, (ns, d))
        X = np.clip(X_n + rng.uniform(-0.02, 0.02, (ns, d)), 0.0, 1.0)
        deltas = np.full(ns, 0.3)
        lb, ub = np.zeros(d), np.ones(d)
        R = -rng.uniform(0.05, 1.0, (ns, k))            # a change of the values that a step of length <= 1 can make: inside reach

        def loop():
            out = []
            for p in range(ns):
                rc, om, dd, ci, mu = descent.ds_criticality_device(plans[p], X_n[p], lb, ub, R[p], want_mult=True)
                assert rc == 0, rc
                nrm = float(np.max(np.abs(dd))) if ci["status"] == _lib.DS_OK else 0.0
                om_s, d_s = (float(om), dd / nrm) if ci["status"] == _lib.DS_OK and nrm > 0 else (0.0, np.zeros(d))
                rc, xp, mxp, si = descent.sd_step_device(plans[p], cfg, X[p], X_n[p], 0.3, lb, ub, om_s, d_s)
                assert rc == 0, rc
                out.append((d_s, xp, mxp, mu, ci["ms_total"] + si["ms_total"], ci["iterations"]))
            return out

        dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
        dX, dX_n, ddel, dlb, dub, dR = dev(X), dev(X_n), dev(deltas), dev(lb), dev(ub), dev(R)
        outs = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in ((ns, d), (ns, d), (ns, k), (ns, k)))
        torch.cuda.synchronize()

        def batch():
            rc, D, XP, MXP, MU, recs, ms = descent.ds_iterate_batch_device(plans, cfg, dX, dX_n, ddel, dlb, dub, dR, out=outs)
            assert rc == 0, rc
            return D, XP, MXP, MU, recs, ms

        if args.calls:
            for _ in range(args.calls):
                batch()
            continue
        ref = loop()
        rec = {"tool": "ds_batch_bench", "label": args.label, "d": d, "k": k, "n_starts": ns, "n": N_CENTRES, "max_loops": cfg.max_loops,
               "reps": args.reps, "qp_iterations_max": int(max(r[5] for r in ref))}
        if has_batch:
            D, XP, MXP, MU, recs, _ = batch()
            got = [np.asarray(t.cpu()) for t in (D, XP, MXP, MU)]
            same = all(np.array_equal(got[i][p], ref[p][i]) for p in range(ns) for i in range(4))
            assert same, "the batch does not reproduce the chained single calls"
            rec["bit_identical"] = True
            rec["batch_qp_iterations_max"] = int(max(r["iterations"] for r in recs))
            for _ in range(3):
                batch()
            host, ev = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r = batch()
                host.append((time.perf_counter() - t0) * 1e3)
                ev.append(r[5])
            rec["batch_event_ms"] = float(np.median(ev))
            rec["batch_event_ms_min_max"] = [float(np.min(ev)), float(np.max(ev))]
            rec["batch_host_ms"] = float(np.median(host))
        for _ in range(3):
            loop()
        host, ev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = loop()
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(sum(x[4] for x in r))
        rec["loop_host_ms"] = float(np.median(host))
        rec["loop_host_ms_min_max"] = [float(np.min(host)), float(np.max(host))]
        rec["loop_event_ms"] = float(np.median(ev))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        for sc in scs:
            sc.lists["objective"][0].model.free()


if __name__ == "__main__":
    main()
