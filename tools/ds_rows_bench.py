"""Time one mrbf_ds_direction_rows call (the direction QP of directed search with constraint rows) and, beside
it, one mrbf_sd_direction call (the steepest-descent direction LP) with the same rows and one mrbf_ds_direction call without rows.  Device-resident buffers of one
context whose stream is torch's current stream, so that a pair of torch events brackets the call; the host clock stands beside it.
The QPs: seeded Gaussian G, sites with half their coordinates on a bound, and per QP one of three targets r -- inside reach, 3 sqrt(d)
and d times that (tests/ds_rows_util.py: make_qp), so that the batch mixes QPs that end after a few iterations with QPs that walk the box.
Per shape: medians of `--calls` calls after a warm-up, fastest and slowest beside them, cells alternating between the three calls.  No
threshold is set: the rows call had not been measured before.  One JSON line per shape.

    python tools/ds_rows_bench.py [--out profiles/ds_rows_bench.jsonl] [--calls 20] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 2, 1, 1, 1), (128, 2, 2, 2, 64), (256, 3, 2, 4, 1024)]   # d, k, m_eq, m_in, n_qp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ds_rows_bench.jsonl"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib
    from tests import ds_rows_util as ru

    ctx = pkg.Context()
    ctx.check(ctx.lib.mrbf_set_stream(ctx.h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    p = _lib.as_ptr
    lines = []
    for d, k, me, mi, nq in SHAPES:
        K = k + me + mi
        G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(d, k, me, mi, n_qp=nq, seed=7)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        Gd, rd, Xd = dev(np.transpose(G, (0, 2, 1))), dev(r), dev(X)
        Aed, bed, Aid, bid = dev(Ae), dev(be), dev(Ai), dev(bi)
        LB, UB = dev(np.broadcast_to(lb, (nq, d))), dev(np.broadcast_to(ub, (nq, d)))
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
        D, Z, om, mu, st, it = f64(nq, d), f64(nq, k), f64(nq), f64(nq, k), i32(nq), i32(nq, 2)
        D2, om2, y2, st2, it2 = f64(nq, d), f64(nq), f64(nq, K), i32(nq), i32(nq, 2)
        D3, C3, om3, mu3, st3, it3 = f64(nq, d), f64(nq, K), f64(nq), f64(nq, K), i32(nq), i32(nq, 2)

        def rows():
            ctx.check(ctx.lib.mrbf_ds_direction_rows(ctx.h, nq, d, k, me, mi, p(Gd), p(rd), p(Xd), p(LB), p(UB), p(Aed), p(bed), p(Aid), p(bid),
                                                     p(D3), p(C3), p(om3), p(mu3), p(st3), p(it3)))

        def ds():
            ctx.check(ctx.lib.mrbf_ds_direction(ctx.h, nq, d, k, p(Gd), p(rd), p(Xd), p(LB), p(UB), p(D), p(Z), p(om), p(mu), p(st), p(it)))

        def sd():
            ctx.check(ctx.lib.mrbf_sd_direction(ctx.h, nq, d, k, me, mi, p(Gd), p(Xd), p(LB), p(UB), p(Aed), p(bed), p(Aid), p(bid), 1, p(D2), p(om2), p(y2),
                                                p(st2), p(it2)))

        for _ in range(args.warmup):
            rows(), ds(), sd()
        assert int((st != 0).sum()) == 0 and int((st2 != 0).sum()) == 0 and int((st3 != 0).sum()) == 0, (st, st2, st3)
        t = {"rows": [], "ds": [], "sd": []}
        e = {"rows": [], "ds": [], "sd": []}
        for _ in range(args.calls):
            for name, fn in (("rows", rows), ("ds", ds), ("sd", sd)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e3)
                e[name].append(float(e0.elapsed_time(e1)))
        med = lambda v: float(np.median(v))
        its, its2, its3 = it.cpu().numpy(), it2.cpu().numpy(), it3.cpu().numpy()
        ms = lambda n: dict(event_median=med(e[n]), event_fastest=min(e[n]), event_slowest=max(e[n]), host_median=med(t[n]))
        rec = dict(d=d, k=k, m_eq=me, m_in=mi, n_qp=nq, calls=args.calls, ds_direction_rows_ms=ms("rows"),
                   ds_rows_iterations=dict(median=float(np.median(its3[:, 0])), most=int(its3[:, 0].max()), dropped_most=int(its3[:, 1].max())),
                   ds_direction_ms=dict(event_median=med(e["ds"]), event_fastest=min(e["ds"]), event_slowest=max(e["ds"]), host_median=med(t["ds"])),
                   sd_direction_ms=dict(event_median=med(e["sd"]), event_fastest=min(e["sd"]), event_slowest=max(e["sd"]), host_median=med(t["sd"])),
                   ds_iterations=dict(median=float(np.median(its[:, 0])), most=int(its[:, 0].max()), dropped_most=int(its[:, 1].max())),
                   sd_iterations=dict(median=float(np.median(its2[:, 0])), most=int(its2[:, 0].max())))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
