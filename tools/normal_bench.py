"""The normal step: device against the host pattern (needs the GPU).

1. one compute_normal_step per call at d = 2 / 12 / 64 / 128 / 256 with one modelled equality, one modelled inequality and two
   linear inequality rows: mrbf_normal_step (values / Jacobians + the LP on the device, one read-back) against the host pattern
   (values and Jacobians by mrbf_eval, then HiGHS on the host);
2. mrbf_normal_direction for 64 and 4096 LPs at d = 2 / 12 / 64 / 256 (4 inequality rows met by a point of the box), inputs and
   outputs resident on the device, against HiGHS per LP (the host time of the batch is the measured per-LP median times the count);
3. the same for 1 and 64 LPs of 64 rows (16 equalities, 48 inequalities) at d = 64 / 256: the largest M and the most iterations.
Times: host clock around calls that end in a stream synchronisation; median of --reps calls after --warmup.  One JSON line per row.
    python tools/normal_bench.py [--reps 30] [--out profiles/normal_bench.jsonl]
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


def constraints(d):
    def f(X):
        X = np.atleast_2d(X)
        return np.concatenate([X[:, :1] + 0.3 * np.sum(X ** 2, axis=1, keepdims=True) / d - 0.1, X[:, -1:] - 0.2], axis=1)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "normal_bench needs the GPU"
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    rng = np.random.default_rng(1)
    for d in (2, 12, 64, 128, 256):
        C = rng.uniform(-2.0, 2.0, (2 * d + 20, d))
        con = pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, constraints(d)(C))
        sc = sg.SurrogateContainer(nl_eq_constraints=[sg.RefSurrogate(con, [1])], nl_ineq_constraints=[sg.RefSurrogate(con, [0])])
        plan = sg.container_plan(sc)
        lin = (None, None, rng.standard_normal((2, d)) / np.sqrt(d), np.array([0.1, -0.2]))
        lb, ub = np.full(d, -2.0), np.full(d, 2.0)
        x = rng.uniform(-1.5, 1.5, d)
        info = {}

        def device():
            rc, n, dl, inf = descent.normal_step_device(plan, x, lb, ub, 0.5, lin)
            assert rc == 0
            info.update(inf)

        def host():
            A_eq, b_eq, A_in, b_in = descent._ns_host_rows(sc, None, x, lin)
            info["alpha_host"] = descent._normal_step_lp(x, lb, ub, A_eq, b_eq, A_in, b_in)[1]

        dm, d10, d90 = median_ms(device, args.reps, args.warmup)
        hm, h10, h90 = median_ms(host, args.reps, args.warmup)
        emit(dict(what="normal_step", d=d, rows=4, device_ms=dm, device_p10=d10, device_p90=d90, device_event_ms=info["ms_total"],
                  host_pattern_ms=hm, host_p10=h10, host_p90=h90, iterations=info["iterations"], status=info["status"],
                  alpha_diff=abs(info["alpha"] - info["alpha_host"])))
        con.free()
    ctx = _lib.default_context()
    m = 4
    for d in (2, 12, 64, 256):
        for n_lp in (64, 4096):
            lb = -rng.random((n_lp, d)) * 2
            ub = rng.random((n_lp, d)) * 2
            x = lb + rng.random((n_lp, d)) * (ub - lb)
            A = rng.standard_normal((n_lp, m, d))
            n0 = (lb - x) + rng.random((n_lp, d)) * (ub - lb)
            b = np.einsum("lij,lj->li", A, n0) + rng.random((n_lp, m)) * 0.1
            dev = {key: torch.from_numpy(np.ascontiguousarray(v)).cuda() for key, v in dict(x=x, lb=lb, ub=ub, A=A, b=b).items()}
            N = torch.empty((n_lp, d), dtype=torch.float64, device="cuda")
            al = torch.empty(n_lp, dtype=torch.float64, device="cuda")
            st = torch.empty(n_lp, dtype=torch.int32, device="cuda")
            it = torch.empty((n_lp, 2), dtype=torch.int32, device="cuda")
            p = _lib.as_ptr

            def device():
                ctx.check(ctx.lib.mrbf_normal_direction(ctx.h, n_lp, d, 0, m, p(dev["x"]), p(dev["lb"]), p(dev["ub"]), None, None,
                                                        p(dev["A"]), p(dev["b"]), p(N), p(al), None, p(st), p(it)))
                torch.cuda.synchronize()

            dm, d10, d90 = median_ms(device, max(5, args.reps // (1 if n_lp < 4096 else 3)), 2)
            sample = list(range(min(n_lp, 20)))

            def host_one(i=[0]):
                j = sample[i[0] % len(sample)]
                i[0] += 1
                descent._normal_step_lp(x[j], lb[j], ub[j], A_ineq=A[j], b_ineq=b[j])

            hm, _, _ = median_ms(host_one, 20, 3)
            its = it.cpu().numpy()
            emit(dict(what="normal_direction", d=d, m=m, n_lp=n_lp, device_ms=dm, device_p10=d10, device_p90=d90,
                      device_us_per_lp=1e3 * dm / n_lp, host_ms_per_lp=hm, host_ms_batch_extrapolated=hm * n_lp,
                      all_ok=bool((st.cpu().numpy() == 0).all()), iterations_median=float(np.median(its[:, 0])),
                      iterations_max=int(its[:, 0].max())))
    # 64 rows (16 equalities, 48 inequalities met by a point of the box): the largest M, the most iterations
    for d in (64, 256):
        meq, mi = 16, 48
        for n_lp in (1, 64):
            lb = -rng.random((n_lp, d)) * 2
            ub = rng.random((n_lp, d)) * 2
            x = lb + rng.random((n_lp, d)) * (ub - lb)
            A = rng.standard_normal((n_lp, meq + mi, d))
            n0 = (lb - x) + rng.random((n_lp, d)) * (ub - lb)
            b = np.einsum("lij,lj->li", A, n0)
            b[:, meq:] += rng.random((n_lp, mi)) * 0.1
            dev = {key: torch.from_numpy(np.ascontiguousarray(v)).cuda()
                   for key, v in dict(x=x, lb=lb, ub=ub, Ae=A[:, :meq], be=b[:, :meq], Ai=A[:, meq:], bi=b[:, meq:]).items()}
            N = torch.empty((n_lp, d), dtype=torch.float64, device="cuda")
            al = torch.empty(n_lp, dtype=torch.float64, device="cuda")
            st = torch.empty(n_lp, dtype=torch.int32, device="cuda")
            it = torch.empty((n_lp, 2), dtype=torch.int32, device="cuda")
            p = _lib.as_ptr

            def device():
                ctx.check(ctx.lib.mrbf_normal_direction(ctx.h, n_lp, d, meq, mi, p(dev["x"]), p(dev["lb"]), p(dev["ub"]), p(dev["Ae"]),
                                                        p(dev["be"]), p(dev["Ai"]), p(dev["bi"]), p(N), p(al), None, p(st), p(it)))
                torch.cuda.synchronize()

            dm, d10, d90 = median_ms(device, 5, 1)

            def host_one(i=[0]):
                j = i[0] % min(n_lp, 5)
                i[0] += 1
                descent._normal_step_lp(x[j], lb[j], ub[j], A[j, :meq], b[j, :meq], A[j, meq:], b[j, meq:])

            hm, _, _ = median_ms(host_one, 5, 1)
            its = it.cpu().numpy()
            emit(dict(what="normal_direction", d=d, m=meq + mi, n_lp=n_lp, device_ms=dm, device_p10=d10, device_p90=d90,
                      device_us_per_lp=1e3 * dm / n_lp, host_ms_per_lp=hm, host_ms_batch_extrapolated=hm * n_lp,
                      all_ok=bool((st.cpu().numpy() == 0).all()), iterations_median=float(np.median(its[:, 0])),
                      iterations_max=int(its[:, 0].max()), us_per_iteration_one_lp=(1e3 * dm / max(1, int(its[0, 0]))) if n_lp == 1 else None))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
