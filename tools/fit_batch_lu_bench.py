"""Many-start model update on the LU path: thin plate spline k = 2 with a degree-1 tail (the kernel's order exceeds what the tail covers:
fit_model sends it to the LU of the saddle system), k = 2 outputs, device-resident sites and values.  One mrbf_fit_batch call under
MRBF_OPT_SMALL_LU = 1 followed by freeing its models, against the loop of n_starts x (mrbf_fit + mrbf_free_model) with the option off --
the rocSOLVER chain, which is the parent commit's path -- at (n, d) = (33, 16), (257, 128), (512, 128) and 1, 8, 16 and 64 starts.

    python tools/fit_batch_lu_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/fit_batch_lu_bench.jsonl] [--reps 30]
                                       [--shapes 33x16,257x128,512x128] [--starts 1,8,16,64]

Medians of `--reps` host-clock calls with the spread (min, max) beside them.  --lib times another build of the library: the parent
commit's has neither the option nor the dispatch symbol, so only the loop is timed there.  Before anything is timed the batch's
weights are checked against single fits under the option (bit identity).  One JSON line per (label, shape, n_starts) is appended to
--out.  One GPU process; run one label at a time and alternate the labels."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_batch_lu_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="33x16,257x128,512x128")
    ap.add_argument("--starts", default="1,8,16,64")
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import torch  # noqa: F401  (before the library, as every driver here does)

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

    built = ctypes.CDLL(_lib.LIB_PATH)
    has_lu = hasattr(built, "mrbf_dispatch_fit_batch_lu")
    for name in list(_lib.SIGNATURES):
        if not hasattr(built, name):       # an earlier build: bind what it has, time the loop only
            _lib.SIGNATURES.pop(name)
    ctx = pkg.Context()
    for shape in args.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        bench_shape(args, ctx, n, d, has_lu)
    ctx.close()


def bench_shape(args, ctx, n, d, has_lu):
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

    lib, k, deg = ctx.lib, 2, 1
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel="thin_plate_spline", polynomial_degree=deg))
    starts = [int(s) for s in args.starts.split(",")]
    rng = np.random.default_rng(4)
    Cs, Ys, Ws, Ls = [], [], [], []
    for p in range(max(starts)):
        C = rng.uniform(-2.0, 2.0, (n, d))
        Y = np.stack([np.sum((C - 1.0) ** 2, axis=1), np.sum((C + 1.0) ** 2, axis=1)], axis=1)
        Cs.append(torch.tensor(C, dtype=torch.float64, device="cuda"))
        Ys.append(torch.tensor(Y, dtype=torch.float64, device="cuda"))
        Ws.append(torch.empty((n, k), dtype=torch.float64, device="cuda"))
        Ls.append(torch.empty((d + 1, k), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()

    def option(value):
        if has_lu:
            ctx.set_option(_lib.OPT_SMALL_LU, value)

    def loop(ns):
        for p in range(ns):
            h, info = _lib.c_vp(), _lib.FitInfo()
            ctx.check(lib.mrbf_fit(ctx.h, n, d, k, _lib.as_ptr(Cs[p]), _lib.as_ptr(Ys[p]), kid, a, b, deg, ctypes.byref(h), _lib.as_ptr(Ws[p]),
                                   _lib.as_ptr(Ls[p]), ctypes.byref(info)))
            assert info.path == _lib.PATH_LU
            ctx.check(lib.mrbf_free_model(ctx.h, h))

    def batch(ns):
        option(1)
        try:
            jobs = (_lib.FitJob * ns)()
            for p in range(ns):
                J = jobs[p]
                J.n, J.d, J.k, J.kernel_id, J.poly_deg, J.a, J.b = n, d, k, kid, deg, a, b
                J.centres, J.values, J.weights_out, J.poly_out = _lib.as_ptr(Cs[p]), _lib.as_ptr(Ys[p]), _lib.as_ptr(Ws[p]), _lib.as_ptr(Ls[p])
            ctx.check(lib.mrbf_fit_batch(ctx.h, ns, jobs, None))
            for J in jobs:
                assert J.status == 0 and J.info.path == _lib.PATH_LU, (J.status, J.info.path)
                ctx.check(lib.mrbf_free_model(ctx.h, J.model))
        finally:
            option(0)

    def timed(f, ns):
        host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            f(ns)
            host.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(host)), [float(np.min(host)), float(np.max(host))]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for ns in starts:
        rec = {"tool": "fit_batch_lu_bench", "label": args.label, "n_starts": ns, "n": n, "d": d, "k": k, "reps": args.reps}
        loop(ns)
        if has_lu:
            option(1)        # (the reference of the bit check: single fits under the option the batch runs with)
            loop(ns)
            option(0)
            ref = [W.cpu().numpy().copy() for W in Ws[:ns]]
            for W in Ws[:ns]:
                W.fill_(float("nan"))
            batch(ns)
            assert all(np.array_equal(Ws[p].cpu().numpy(), ref[p]) for p in range(ns)), "the batch does not reproduce the single fits"
            rec["bit_identical"] = True
            rec["batch_host_ms"], rec["batch_host_ms_min_max"] = timed(batch, ns)
        rec["loop_host_ms"], rec["loop_host_ms_min_max"] = timed(loop, ns)
        if has_lu:
            rec["batch_over_loop"] = rec["batch_host_ms"] / rec["loop_host_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
