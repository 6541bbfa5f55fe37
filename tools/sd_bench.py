"""Steepest-descent criticality: device against the host pattern (needs the GPU).

1. one get_criticality(::SteepestDescentConfig) per call at d = 2 / 12 / 64 / 128 / 256 and k = 2 / 3: mrbf_sd_criticality (device
   Jacobians + the LP on the device, one read-back) against the host pattern (the Jacobian by mrbf_eval, then HiGHS on the host);
2. mrbf_sd_direction for 1, 64 and 4096 LPs at d = 64 / 256 (k = 3, box only), inputs and outputs resident on the device, against
   HiGHS per LP (the host time of the batch is the measured per-LP median times the count).
Times: host clock around calls that end in a stream synchronisation; median of --reps calls after --warmup.  One JSON line per row.
    python tools/sd_bench.py [--reps 30] [--out profiles/sd_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import morbit.jl_amd as pkg  # noqa: E402
from morbit.jl_amd import _lib, descent  # noqa: E402
from morbit.jl_amd import surrogates as sg  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def objectives(k):
    def f(X):
        X = np.atleast_2d(X)
        shifts = np.linspace(-1.0, 1.0, k)
        return np.stack([np.sum((X - s) ** 2, axis=1) for s in shifts], axis=1)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "sd_bench needs the GPU"
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    rng = np.random.default_rng(1)
    cfg = descent.SteepestDescentConfig()
    for d in (2, 12, 64, 128, 256):
        for k in (2, 3):
            f = objectives(k)
            C = rng.uniform(-2.0, 2.0, (2 * d + 20, d))
            mod = pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, f(C))
            sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, list(range(k)))])
            plan = sg.container_plan(sc)
            lb, ub = np.full(d, -2.0), np.full(d, 2.0)
            x = rng.uniform(-1.5, 1.5, d)
            info = {}

            def device():
                rc, om, dd, inf = descent.sd_criticality_device(plan, x, x, lb, ub, cfg.normalize)
                assert rc == 0
                info.update(inf, omega_dev=om)

            def host():
                J = mod.eval_sites(x[None, :], want_values=False, want_jac=True)[1][0]
                info["omega_host"] = descent._steepest_descent_direction(x, J, lb, ub, normalize=cfg.normalize)[1]

            dm, d10, d90 = median_ms(device, args.reps, args.warmup)
            hm, h10, h90 = median_ms(host, args.reps, args.warmup)
            emit(dict(what="sd_criticality", d=d, k=k, device_ms=dm, device_p10=d10, device_p90=d90, device_event_ms=info["ms_total"],
                      host_pattern_ms=hm, host_p10=h10, host_p90=h90, iterations=info["iterations"], bound_flips=info["bound_flips"],
                      omega_diff=abs(info["omega_dev"] - info["omega_host"])))
            mod.free()
    ctx = _lib.default_context()
    for d in (64, 256):
        k = 3
        for n_lp in (1, 64, 4096):
            lb = -rng.random((n_lp, d)) * 2
            ub = rng.random((n_lp, d)) * 2
            x = lb + rng.random((n_lp, d)) * (ub - lb)
            G = rng.standard_normal((n_lp, d, k))          # per LP k x d column-major
            dev = {key: torch.from_numpy(np.ascontiguousarray(v)).cuda() for key, v in dict(G=G, x=x, lb=lb, ub=ub).items()}
            D = torch.empty((n_lp, d), dtype=torch.float64, device="cuda")
            om = torch.empty(n_lp, dtype=torch.float64, device="cuda")
            st = torch.empty(n_lp, dtype=torch.int32, device="cuda")
            it = torch.empty((n_lp, 2), dtype=torch.int32, device="cuda")
            p = _lib.as_ptr

            def device():
                ctx.check(ctx.lib.mrbf_sd_direction(ctx.h, n_lp, d, k, 0, 0, p(dev["G"]), p(dev["x"]), p(dev["lb"]), p(dev["ub"]),
                                                    None, None, None, None, 1, p(D), p(om), None, p(st), p(it)))
                torch.cuda.synchronize()

            dm, d10, d90 = median_ms(device, max(5, args.reps // (1 if n_lp < 4096 else 3)), 2)
            sample = list(range(min(n_lp, 20)))

            def host_one(i=[0]):
                j = sample[i[0] % len(sample)]
                i[0] += 1
                descent._steepest_descent_direction(x[j], G[j].T, lb[j], ub[j])

            hm, _, _ = median_ms(host_one, 20, 3)
            its = it.cpu().numpy()
            emit(dict(what="sd_direction", d=d, k=k, n_lp=n_lp, device_ms=dm, device_p10=d10, device_p90=d90, device_us_per_lp=1e3 * dm / n_lp,
                      host_ms_per_lp=hm, host_ms_batch_extrapolated=hm * n_lp, all_ok=bool((st.cpu().numpy() == 0).all()),
                      iterations_median=float(np.median(its[:, 0])), iterations_max=int(its[:, 0].max()),
                      flips_median=float(np.median(its[:, 1]))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
