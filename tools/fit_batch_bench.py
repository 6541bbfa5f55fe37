"""Many-start model update at the C4 shape (n = 257, d = 128, cubic, degree-1 tail, k = 2, device-resident sites and values): one
mrbf_fit_batch call followed by freeing its models, against the loop of n_starts x (mrbf_fit + mrbf_free_model), for n_starts in
{1, 8, 64}.

    python tools/fit_batch_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/fit_batch_bench.jsonl] [--reps 30]

Medians of `--reps` host-clock calls with the event time beside them (the batch call's ms_total; the sum of info.ms_total over the
loop) and the spread (min, max) of the host-clock calls.  --lib times another build of the library (the parent commit's, which has no
batch entry: only the loop is timed there); one JSON line per (label, n_starts) is appended to --out.  The batch's weights are checked
against the loop's (bit identity) before anything is timed.  One GPU process; run one label at a time.

    python tools/fit_batch_bench.py --wide --n 645,907,1164,1684,2048 --starts 8,16,64 --out profiles/fit_batch_wide_bench.jsonl

--n times other site counts (the C4 rehearsal's model sizes beyond 512), --d another dimension (at most 128).  --wide raises the context's MRBF_OPT_SMALL_FIT_MAX_N to 2048
for the batch call, so that starts beyond 512 sites share its one launch; the loop of single fits runs at the option's default (the
launch chain), which is what the batch replaces.  The bit check then compares the batch with single fits under the raised option.  A
build without the option (--lib, the parent commit's) times the loop only."""
import argparse
import ctypes
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_batch_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--starts", default="1,8,64")
    ap.add_argument("--n", default="257")
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import torch  # noqa: F401  (before the library, as every driver here does)

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

    built = ctypes.CDLL(_lib.LIB_PATH)
    has_batch = hasattr(built, "mrbf_fit_batch")
    has_wide = hasattr(built, "mrbf_dispatch_fit_batch_max_n")
    for name in ("mrbf_fit_batch", "mrbf_dispatch_fit_batch", "mrbf_dispatch_fit_batch_max_n"):
        if not hasattr(built, name):       # an earlier build: bind what it has, time the loop only
            _lib.SIGNATURES.pop(name, None)
    if args.wide and not has_wide:
        has_batch = False
    ctx = pkg.Context()
    lib = ctx.lib
    for n in (int(v) for v in args.n.split(",")):
        bench_size(args, ctx, lib, n, has_batch)
    ctx.close()


def bench_size(args, ctx, lib, n, has_batch):
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

    d, k, deg = args.d, 2, 1
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel="cubic", polynomial_degree=deg))
    starts = [int(s) for s in args.starts.split(",")]
    P = max(starts)
    rng = np.random.default_rng(4)
    Cs, Ys, Ws, Ls = [], [], [], []
    for p in range(P):
        C = rng.uniform(-2.0, 2.0, (n, d))
        Y = np.stack([np.sum((C - 1.0) ** 2, axis=1), np.sum((C + 1.0) ** 2, axis=1)], axis=1)
        Cs.append(torch.tensor(C, dtype=torch.float64, device="cuda"))
        Ys.append(torch.tensor(Y, dtype=torch.float64, device="cuda"))
        Ws.append(torch.empty((n, k), dtype=torch.float64, device="cuda"))
        Ls.append(torch.empty((d + 1, k), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()

    def loop(ns):
        ev = 0.0
        for p in range(ns):
            h, info = _lib.c_vp(), _lib.FitInfo()
            ctx.check(lib.mrbf_fit(ctx.h, n, d, k, _lib.as_ptr(Cs[p]), _lib.as_ptr(Ys[p]), kid, a, b, deg, ctypes.byref(h), _lib.as_ptr(Ws[p]),
                                   _lib.as_ptr(Ls[p]), ctypes.byref(info)))
            ev += info.ms_total
            ctx.check(lib.mrbf_free_model(ctx.h, h))
        return ev

    def option(value):
        if args.wide and has_batch:
            ctx.set_option(_lib.OPT_SMALL_FIT_MAX_N, value)

    def batch(ns):
        option(2048)
        try:
            return batch_call(ns)
        finally:
            option(512)

    def batch_call(ns):
        jobs = (_lib.FitJob * ns)()
        for p in range(ns):
            J = jobs[p]
            J.n, J.d, J.k, J.kernel_id, J.poly_deg, J.a, J.b = n, d, k, kid, deg, a, b
            J.centres, J.values, J.weights_out, J.poly_out = _lib.as_ptr(Cs[p]), _lib.as_ptr(Ys[p]), _lib.as_ptr(Ws[p]), _lib.as_ptr(Ls[p])
        ms = ctypes.c_float()
        ctx.check(lib.mrbf_fit_batch(ctx.h, ns, jobs, ctypes.byref(ms)))
        for J in jobs:
            assert J.status == 0, J.status
            ctx.check(lib.mrbf_free_model(ctx.h, J.model))
        return ms.value

    def timed(f, ns):
        host, ev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            e = f(ns)
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(e)
        return float(np.median(host)), float(np.median(ev)), [float(np.min(host)), float(np.max(host))]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for ns in starts:
        rec = {"tool": "fit_batch_bench", "label": args.label, "n_starts": ns, "n": n, "d": d, "k": k, "reps": args.reps, "wide": bool(args.wide)}
        loop(ns)
        if has_batch:
            option(2048)     # (the reference of the bit check: single fits under the option value the batch runs with)
            loop(ns)
            option(512)
            ref = [W.cpu().numpy().copy() for W in Ws[:ns]]
            for W in Ws[:ns]:
                W.fill_(float("nan"))
            batch(ns)
            assert all(np.array_equal(Ws[p].cpu().numpy(), ref[p]) for p in range(ns)), "the batch does not reproduce the single fits"
            rec["bit_identical"] = True
            rec["batch_host_ms"], rec["batch_event_ms"], rec["batch_host_ms_min_max"] = timed(batch, ns)
        rec["loop_host_ms"], rec["loop_event_ms"], rec["loop_host_ms_min_max"] = timed(loop, ns)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
