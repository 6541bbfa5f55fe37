"""Local ideal points on the device: one mrbf_ideal_point_batch call against the loop of mrbf_ideal_point_problem calls, against the host
search directed search runs today, and `ds_iterate_many` end to end with either -- at the C4 shape (d = 128, n = 257 centres per model,
cubic, degree-1 tail, k = 2, built from coefficients: no fit), default budgets (500 (d + 1) evaluations per objective), boxes of
half-width 1.1 x 0.1 around x_n, n_starts in {1, 2, 8, 64}.

    python tools/ideal_point_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/ideal_point_bench.jsonl] [--reps 20]

One JSON line per (label, n_starts) is appended to --out, then one line for the host search and one per end-to-end count:
  * batch / loop: medians of --reps calls after 3 warm-up calls, by the host clock (the loop has no one event time), with fastest and
    slowest; the batch's event time beside it.  Contract B (every output of the batch equals the single call's, bit for bit) is asserted
    before anything is timed.
  * host search: `compute_local_ideal_point` as `descent._ds_image_direction` calls it, once on each of --host-starts starts, reported
    per start; its ideal values beside the device search's for the same starts (information only: different random processes).
  * end to end: `descent.ds_iterate_many` in the default configuration (the host search per start, then one mrbf_ds_iterate_batch call)
    and with ideal_point="device" (two device calls), at --e2e-starts starts; medians of --e2e-reps calls after one warm-up.
--lib times another build of the library (the parent commit's, which has no ideal-point entry: only the default configuration's end
to end and the host search are timed there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, K, N_CENTRES = 128, 2, 257
STARTS = [1, 2, 8, 64]
NEW_SYMBOLS = ("mrbf_ideal_point_problem", "mrbf_ideal_point_batch", "mrbf_dispatch_ideal", "mrbf_dispatch_ideal_batch")


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [float(np.min(t)), float(np.max(t))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ideal_point_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-starts", type=int, default=3)
    ap.add_argument("--e2e-starts", type=int, nargs="*", default=[8])
    ap.add_argument("--e2e-reps", type=int, default=3)
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import ctypes

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import pascoletti_serafini as ps
    from morbit.jl_amd import rbf_model as rm
    from morbit.jl_amd import surrogates as sg

    raw = ctypes.CDLL(_lib.LIB_PATH)
    has_ideal = hasattr(raw, "mrbf_ideal_point_batch")
    if not has_ideal:       # an earlier build: bind what it has
        for name in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    mcfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    ns_max = max(STARTS + args.e2e_starts)
    rng = np.random.default_rng(128257)
    scs = []
    for p in range(ns_max):
        C = rng.uniform(0.0, 1.0, (N_CENTRES, D))
        W = rng.standard_normal((N_CENTRES, K)) * 0.05 / N_CENTRES
        mod = rm.model_from_coeffs(mcfg, C, W, rng.standard_normal((D + 1, K)))
        scs.append(sg.SurrogateContainer(objectives=[sg.RefSurrogate(mod, list(range(K)))]))
    plans = [sg.container_plan(sc) for sc in scs]
    X_n = rng.uniform(0.2, 0.8, (ns_max, D))
    deltas = np.full(ns_max, 0.1)
    lb, ub = np.zeros(D), np.ones(D)
    cfg_host = descent.DirectedSearchConfig()
    cfg_dev = descent.DirectedSearchConfig(ideal_point="device") if has_ideal else None
    half = cfg_host.reference_trust_region_factor * 0.1
    LB, UB = X_n - half, X_n + half
    seeds = list(range(100, 100 + ns_max))
    FX_n = np.stack([pkg.eval_models_at_sites(plans[p]["models"][0], None, X_n[p][None, :])[0] for p in range(ns_max)])
    base = {"tool": "ideal_point_bench", "label": args.label, "d": D, "k": K, "n": N_CENTRES, "max_ideal_evals": 500 * (D + 1)}

    dev_ideal = None
    if has_ideal:
        for ns in STARTS:
            def batch():
                out = ps.ideal_points_batch_device(cfg_dev, plans[:ns], X_n[:ns], LB[:ns], UB[:ns], seeds=seeds[:ns])
                assert out[0] == 0, out[0]
                return out

            def loop():
                outs = [ps.ideal_point_problem_device(cfg_dev, plans[p], X_n[p], LB[p], UB[p], seed=seeds[p]) for p in range(ns)]
                assert all(o[0] == 0 for o in outs)
                return outs

            b, l = batch(), loop()
            bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
            for p in range(ns):             # contract B before anything is timed
                assert all(np.array_equal(bits(b[i][p]), bits(l[p][i])) for i in (1, 2, 3)), ("contract B", ns, p)
                assert all(b[4][p][f] == l[p][4][f] for f in ("evals_ideal", "generations", "found", "refined")), ("contract B", ns, p)
            if ns == max(STARTS):
                dev_ideal = b[1].copy()
            ev = []
            t_batch, mm_batch = timed(lambda: ev.append(batch()[5]), args.reps, 3)
            t_loop, mm_loop = timed(loop, args.reps, 3)
            emit(dict(base, kind="batch_vs_loop", n_starts=ns, reps=args.reps, bit_identical=True, batch_host_ms=t_batch,
                      batch_host_ms_min_max=mm_batch, batch_event_ms=float(np.median(ev[3:])), loop_host_ms=t_loop,
                      loop_host_ms_min_max=mm_loop, batch_over_loop=t_batch / t_loop,
                      evals_ideal_per_start=float(np.mean([i["evals_ideal"] for i in b[4]])),
                      generations_per_start=float(np.mean([i["generations"] for i in b[4]]))))

    # today's host search, as _ds_image_direction calls it (one start after the other)
    host_ms, host_ideal, host_stats = [], [], []
    for p in range(args.host_starts):
        st = {}
        t0 = time.perf_counter()
        r = descent._ds_image_direction(cfg_host, scs[p], None, X_n[p], X_n[p], FX_n[p], 0.1, lb, ub, np.random.default_rng(seeds[p]), st)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        host_ideal.append((r + FX_n[p]).tolist())
        host_stats.append([st.get("ideal_point_calls"), st.get("ideal_point_evals")])
    emit(dict(base, kind="host_search", starts=args.host_starts, host_ms_per_start=float(np.median(host_ms)),
              host_ms_min_max=[float(np.min(host_ms)), float(np.max(host_ms))], calls_and_evals=host_stats, host_ideal=host_ideal,
              device_ideal=None if dev_ideal is None else dev_ideal[:args.host_starts].tolist(), m_x_n=FX_n[:args.host_starts].tolist()))

    # directed search end to end
    for ns in args.e2e_starts:
        rec = dict(base, kind="ds_iterate_many", n_starts=ns, reps=args.e2e_reps)
        for name, cfg in (("default", cfg_host), ("device", cfg_dev)):
            if cfg is None:
                continue
            stats = {}

            def run():
                return descent.ds_iterate_many(cfg, scs[:ns], None, X_n[:ns], X_n[:ns], FX_n[:ns], deltas[:ns], lb, ub, stats=stats,
                                               rng=np.random.default_rng(0), **({"seeds": seeds[:ns]} if name == "device" else {}))

            t, mm = timed(run, args.e2e_reps if name == "default" else args.reps, 1 if name == "default" else 3)
            assert stats["path"] == "batch", stats["path"]
            rec["%s_ms" % name], rec["%s_ms_min_max" % name] = t, mm
            rec["%s_ideal_point_path" % name] = stats.get("ideal_point_path")
            rec["%s_omega_mean" % name] = float(np.mean([r["omega"] for r in stats["records"]]))
        emit(rec)
    for sc in scs:
        sc.lists["objective"][0].model.free()


if __name__ == "__main__":
    main()
