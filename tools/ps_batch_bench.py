"""Many-start Pascoletti-Serafini step at the C4 shape (d = 128, n = 257, cubic, degree-1 tail, k = 2, one model per start): one
mrbf_ps_step_batch call against the loop of n_starts x mrbf_ps_step_problem, for n_starts in {1, 2, 8, 64}, with the paper benchmark's
budgets (examples/large_scale_benchmarks.jl:215-219: a reference point, 50 (d + 1) evaluations of the global method, 100 (d + 1) of the
polish) and with the defaults (ideal-point phase, 500 (d + 1) evaluations each).

    python tools/ps_batch_bench.py [--label new] [--lib path/to/libmrbf.so] [--out profiles/ps_batch_bench.jsonl] [--reps 20]
                                   [--starts 1,2,8,64] [--budgets benchmark,default] [--once]

Median and range of `--reps` host-clock calls (and the event time).  --lib times another build of the library (the parent commit's,
which has no batch entry: only the loop is timed there -- the single call must not have become slower); one JSON line per (label,
budgets, n_starts) is appended to --out.  The batch's outputs are checked against the loop's (bit identity) before anything is timed.
--once: one batch call per row and nothing else (for a kernel trace: the launch count per generation)."""
import argparse
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps_batch_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--starts", default="1,2,8,64")
    ap.add_argument("--budgets", default="benchmark,default")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.lib:
        os.environ["MRBF_LIB"] = os.path.abspath(args.lib)
    import ctypes

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib
    from morbit.jl_amd import pascoletti_serafini as ps
    from morbit.jl_amd import surrogates as sg

    raw = ctypes.CDLL(_lib.LIB_PATH)
    has_batch = hasattr(raw, "mrbf_ps_step_batch")
    if not has_batch:       # an earlier build: bind what it has, time the loop only
        for name in ("mrbf_ps_step_batch", "mrbf_dispatch_ps_batch"):
            _lib.SIGNATURES.pop(name, None)
    d, n, k = 128, 257, 2
    starts = [int(s) for s in args.starts.split(",")]
    rng = np.random.default_rng(4)
    mcfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    mods = []
    for p in range(max(starts)):
        C = rng.uniform(0.0, 1.0, (n, d))
        Y = np.stack([np.sum((C - 0.3) ** 2, axis=1), np.sum((C - 0.7) ** 2, axis=1)], axis=1)
        mods.append(pkg.update_model(mcfg, C, Y))
    plans = [sg.container_plan(sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])])) for m in mods]
    X_n = 0.5 + rng.uniform(-0.1, 0.1, (max(starts), d))
    # the "true" values at x_n are the models' own: 2 d + 1 random sites do not pin the functions down at d = 128, and with the
    # functions' values r = fx - ideal comes out non-positive (every start critical: no PS phase to time)
    FX = np.stack([pkg.eval_models_at_sites(mods[p], None, X_n[p][None, :])[0] for p in range(max(starts))])
    LB, UB = X_n - 0.1, X_n + 0.1
    seeds = [100 + p for p in range(max(starts))]
    cfgs = {"benchmark": ps.PascolettiSerafiniConfig(reference_point=[-1.0, -1.0], max_ps_problem_evals=50 * (d + 1),
                                                     max_ps_polish_evals=100 * (d + 1), ps_polish_algo="LD_MMA"),
            "default": ps.PascolettiSerafiniConfig()}

    def loop(cfg, ns):
        out = []
        for p in range(ns):
            st = {}
            rc, res = ps._ps_step_problem(cfg, plans[p]["models"], plans[p]["roles"], k, X_n[p], X_n[p], FX[p], LB[p], UB[p], seed=seeds[p], stats=st)
            assert rc == 0, rc
            out.append((res, st))
        return out

    def batch(cfg, ns):
        dirs = [ps._get_global_dir(cfg, FX[p]) for p in range(ns)]
        R = None if dirs[0] is None else np.stack(dirs)
        rc, xt, mt, ro, infos, ms = ps.ps_step_batch_device(cfg, plans[:ns], X_n[:ns], FX[:ns], LB[:ns], UB[:ns], R=R, seeds=seeds[:ns])
        assert rc == 0, rc
        return xt, mt, ro, infos, ms

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for bname in args.budgets.split(","):
        cfg = cfgs[bname]
        for ns in starts:
            rec = {"tool": "ps_batch_bench", "label": args.label, "budgets": bname, "n_starts": ns, "d": d, "n": n, "k": k, "reps": args.reps}
            if args.once:
                xt, mt, ro, infos, ms = batch(cfg, ns)
                gens = [i["generations"] for i in infos]
                rec.update(batch_event_ms=ms, generations_min_max=[min(gens), max(gens)], status=sorted(set(i["status"] for i in infos)))
                print(json.dumps(rec), flush=True)
                continue
            ref = loop(cfg, ns)
            if has_batch:
                xt, mt, ro, infos, _ = batch(cfg, ns)
                for p in range(ns):
                    res, st = ref[p]
                    assert infos[p]["status"] == st["status"] and np.float64(infos[p]["tau"]).view(np.uint64) == np.float64(st["tau"]).view(np.uint64), p
                    assert all(infos[p][f] == st[f] for f in ("generations", "evals_ideal", "evals_ps", "evals_polish")), p
                    assert np.array_equal(ro[p].view(np.uint64), st["r"].view(np.uint64)), p
                    if st["status"] == _lib.PS_OK:
                        assert np.array_equal(xt[p].view(np.uint64), res[1][0].view(np.uint64)), p
                        assert np.array_equal(mt[p].view(np.uint64), res[1][1].view(np.uint64)), p
                rec["bit_identical"] = True
                rec["generations"] = int(np.max([i["generations"] for i in infos]))
                rec["status"] = sorted(set(i["status"] for i in infos))
                host, ev = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    r = batch(cfg, ns)
                    host.append((time.perf_counter() - t0) * 1e3)
                    ev.append(r[4])
                rec["batch_host_ms"] = float(np.median(host))
                rec["batch_event_ms"] = float(np.median(ev))
                rec["batch_host_ms_min_max"] = [float(np.min(host)), float(np.max(host))]
            host, ev = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r = loop(cfg, ns)
                host.append((time.perf_counter() - t0) * 1e3)
                ev.append(sum(st["ms_total"] for _, st in r))
            rec["loop_host_ms"] = float(np.median(host))
            rec["loop_event_ms"] = float(np.median(ev))
            rec["loop_host_ms_min_max"] = [float(np.min(host)), float(np.max(host))]
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
