"""The database traffic of one many-start iteration at the C4 shape (64 starts, d = 128, k = 2): round 3 with n_new new sites per start,
eval_missing! of those sites, and the append of one trial point per start -- through the batched calls (mrbf_db_round3_batch,
mrbf_db_set_values_batch, mrbf_db_append_batch: three calls, three synchronisations) and the way a caller did it before them (the host
mirror of round 3 on the filter's Z, then mrbf_db_append, mrbf_db_set_values and mrbf_db_append once per start: 3 x n_starts calls,
each with its own synchronisation), alternating, in one process.  Both paths start from the filter's Z as a host array (that is what
find_suitable_points_many returns by default).

    python tools/round3_batch_bench.py [--reps 7] [--starts 64] [--d 128] [--out profiles/round3_batch_bench.jsonl]

Every repetition runs on fresh databases of --n-db rows (created outside the timed region).  The two paths' databases are compared
(equality of bits) before anything is timed.  Written to --out, one JSON line per n_new in {16, d}: host clock around each path and
each of its three stages (minimum and median of --reps), the hipEvent time of the round-3 chain alone, and the number of library calls
(= synchronisations) of each path.  One GPU process."""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--starts", type=int, default=64)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n-db", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round3_batch_bench.jsonl"))
    args = ap.parse_args()
    import morbit.jl_amd as pkg
    from morbit.jl_amd import database, sampling

    ctx = pkg.Context()
    ns, d, k, n_db = args.starts, args.d, 2, args.n_db
    rng = np.random.default_rng(17)
    base = [(rng.uniform(0.0, 1.0, (n_db, d)), rng.uniform(-1.0, 1.0, (n_db, k))) for _ in range(ns)]
    xs = [np.full(d, 0.5) + rng.integers(-2, 3, d) / 64.0 for _ in range(ns)]
    lb1, ub1 = [x - 0.25 for x in xs], [x + 0.25 for x in xs]
    piv = 0.25 / 4
    f = lambda X: np.stack([np.sum((X - 1.0) ** 2, axis=1), np.sum((X + 1.0) ** 2, axis=1)], axis=1)
    trial = [x + 0.125 * rng.uniform(-1, 1, d) for x in xs]
    trial_v = [f(t[None, :]) for t in trial]
    out = []
    for n_new in sorted({min(16, d), d}):
        # the filter's final Z of every start: d x n_new with inf-normalised orthogonal columns, taken last column first
        Zs = []
        for p in range(ns):
            Q = np.linalg.qr(rng.normal(size=(d, n_new)))[0]
            Zs.append(np.ascontiguousarray((Q / np.abs(Q).max(axis=0)).T))       # rows are directions: the memory of the column-major Z

        def fresh():
            dbs = [database.DeviceDatabase(d, k, ctx=ctx, capacity=n_db) for _ in range(ns)]
            for db, (S, V) in zip(dbs, base):
                db.append(S, V)
            return dbs

        def batched(dbs, t, ev=None):
            st = {}
            t0 = time.perf_counter()
            res = sampling.rbf_round3_append(dbs, lb1, ub1, xs, piv, Zs, 10 ** 9, n_new, True, False, reversed_order=True, ctx=ctx, stats=st)
            t1 = time.perf_counter()
            database.set_values_many(dbs, [r.indices for r in res], [f(r.new_points) for r in res], ctx=ctx)
            t2 = time.perf_counter()
            database.append_many(dbs, [v[None, :] for v in trial], trial_v, ctx=ctx)
            t3 = time.perf_counter()
            assert st["path"] == "device" and not any(r.rebuilt for r in res)
            t.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            if ev is not None:
                ev.append(st["ms_total"])

        def per_start(dbs, t):
            t0 = time.perf_counter()
            res = sampling.rbf_round3_many(lb1, ub1, xs, piv, Zs, 10 ** 9, n_new, True, False, reversed_order=True)
            firsts = [db.append(r.new_points) for db, r in zip(dbs, res)]
            t1 = time.perf_counter()
            for db, r, first in zip(dbs, res, firsts):
                db.set_values(np.arange(first, first + r.new_points.shape[0]), f(r.new_points))
            t2 = time.perf_counter()
            for db, v, y in zip(dbs, trial, trial_v):
                db.append(v[None, :], y)
            t3 = time.perf_counter()
            t.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))

        def free(dbs):
            for db in dbs:
                db.free()

        # ---- the two paths agree (also the warm-up)
        a, b = fresh(), fresh()
        batched(a, []), per_start(b, [])
        for da, db_ in zip(a, b):
            (Sa, Va), (Sb, Vb) = da.read(), db_.read()
            assert len(da) == len(db_) == n_db + n_new + 1
            assert np.array_equal(Sa.view(np.uint64), Sb.view(np.uint64)) and np.array_equal(Va.view(np.uint64), Vb.view(np.uint64)), "the paths disagree"
        free(a), free(b)
        tb, tp, ev = [], [], []
        for _ in range(args.reps):                                  # alternating
            dbs = fresh()
            batched(dbs, tb, ev)
            free(dbs)
            dbs = fresh()
            per_start(dbs, tp)
            free(dbs)
        stat = lambda t, i: {"min": float(np.min([x[i] for x in t])), "median": float(np.median([x[i] for x in t]))}
        names = ("all", "round3", "set_values", "append_trial")
        out.append({"tool": "round3_batch_bench", "n_starts": ns, "d": d, "k": k, "n_db": n_db, "n_new": n_new, "reps": args.reps,
                    "batched_ms": {nm: stat(tb, i) for i, nm in enumerate(names)}, "per_start_ms": {nm: stat(tp, i) for i, nm in enumerate(names)},
                    "round3_event_ms": {"min": float(np.min(ev)), "median": float(np.median(ev))},
                    "library_calls": {"batched": 3, "per_start": 3 * ns}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fo:
        for r in out:
            line = json.dumps(r)
            print(line, flush=True)
            fo.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
