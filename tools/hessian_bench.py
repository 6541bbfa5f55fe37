"""Time mrbf_eval_hessian against what a user had to do before it: central differences of mrbf_eval Jacobians, 2 d displaced queries
per point (DESIGN.md "Model Hessians").  Both routes run on device-resident buffers of one context in one session; the displaced
queries are built once, outside the timed region, so the difference route is charged its evaluation and the subtraction only.
The outputs are compared before anything is timed.  Per shape: medians of `--calls` host-clock calls after a warm-up, fastest and
slowest beside them, the hipEvent time of the library call, cells alternating between the two routes.  Admission rule of
dispatch.hip: the direct call should take at most 0.8 of the difference route's median.  One JSON line per shape.

    python tools/hessian_bench.py [--out profiles/hessian_bench.jsonl] [--calls 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64_MFMA = 78.6e12   # MI355X fp64 matrix peak, flop/s
ADMISSION = 0.8

# name, kernel, shape parameter, d, n, k, m
SHAPES = [
    ("C3 model, m = 256", "multiquadric", float("nan"), 64, 8192, 2, 256),
    ("C4 model, m = 64", "cubic", float("nan"), 128, 257, 2, 64),
    ("d = 256, n = 1024, m = 16", "multiquadric", float("nan"), 256, 1024, 2, 16),
    ("C3 model, m = 1 (split path)", "multiquadric", float("nan"), 64, 8192, 2, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hessian_bench.jsonl"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    import morbit.jl_amd as pkg

    ctx = pkg.Context()
    h = 1e-4
    lines = []
    for name, kernel, sp, d, n, k, m in SHAPES:
        rng = np.random.default_rng(d + n)
        cfg = pkg.RbfConfig(kernel=kernel, shape_parameter=sp, polynomial_degree=1)
        C, W, Lam = rng.random((n, d)), rng.standard_normal((n, k)) / n, rng.standard_normal((d + 1, k))
        mod = pkg.model_from_coeffs(cfg, C, W, Lam, ctx=ctx)
        X = 0.25 + 0.5 * rng.random((m, d))
        Xd = torch.from_numpy(X).cuda()
        Hd = torch.full((m, k, d, d), float("nan"), dtype=torch.float64, device="cuda")
        steps = (h * torch.eye(d, dtype=torch.float64, device="cuda"))[None]
        Xpm = torch.cat([Xd[:, None, :] + steps, Xd[:, None, :] - steps], dim=1).reshape(2 * m * d, d).contiguous()
        two_h = (Xpm.view(m, 2, d, d)[:, 0] - Xpm.view(m, 2, d, d)[:, 1]).diagonal(dim1=1, dim2=2).contiguous()   # the steps actually taken
        Jd = torch.empty((2 * m * d, d, k), dtype=torch.float64, device="cuda")      # per point a k x d column-major block
        hinfo, einfo = {}, {}

        def direct():
            mod.hessian_sites(Xd, out=Hd, info=hinfo)
            return Hd

        def differences():
            mod.eval_sites(Xpm, want_values=False, want_jac=True, out_jac=Jd, info=einfo)
            J = Jd.view(m, 2, d, d, k)                                                 # point, sign, displaced j, coordinate i, output
            fd = ((J[:, 0] - J[:, 1]) / two_h[:, :, None, None]).permute(0, 3, 2, 1)   # [p, l, i, j]
            torch.cuda.synchronize()
            return fd

        # ---- the outputs first
        Hh, Fh = direct().cpu().numpy(), differences().cpu().numpy()
        scale = np.abs(Hh).max()
        agree = float(np.abs(Hh - Fh).max() / scale)
        assert np.isfinite(Hh).all() and agree < 1e-5, (name, agree)
        assert np.array_equal(Hh, np.swapaxes(Hh, 2, 3))
        # ---- then the clock: warm-up, then alternating cells
        for _ in range(args.warmup):
            direct(), differences()
        t_dir, t_fd, e_dir, e_fd = [], [], [], []
        for _ in range(args.calls):
            for fn, ts, es, info in ((direct, t_dir, e_dir, hinfo), (differences, t_fd, e_fd, einfo)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
                es.append(float(info["ms_total"]))
        flops = 2.0 * n * k * d * (d + 16) / 2.0 * m
        med = lambda v: float(np.median(v))
        rec = dict(shape=name, kernel=kernel, d=d, n=n, k=k, m=m, calls=args.calls, nsplit=int(hinfo["nsplit"]),
                   direct_ms=dict(median=med(t_dir), fastest=min(t_dir), slowest=max(t_dir), event_median=med(e_dir)),
                   differences_ms=dict(median=med(t_fd), fastest=min(t_fd), slowest=max(t_fd), event_median=med(e_fd), queries=2 * m * d),
                   ratio=med(t_dir) / med(t_fd), admitted=bool(med(t_dir) <= ADMISSION * med(t_fd)),
                   max_rel_difference_of_the_routes=agree,
                   mfma_fraction=flops / (med(e_dir) * 1e-3) / PEAK_F64_MFMA, upper_triangle_flops=flops)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        mod.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
