"""One model-update round of a many-start run at the C4 shape (d = 128, 64 starts, n_db = 1400, boxes holding most of the database,
cubic kernel with a degree-1 tail, k = 2, models of 257 sites): filter round 1, then round 4, then the fit -- through the drivers
(find_suitable_points_many, rbf_round4_many) on NumPy arrays with update_models_many (every site uploaded per call: the code as it
was before the resident database) and on resident databases with update_models_resident, alternating, in one process.

    python tools/db_batch_bench.py [--reps 7] [--starts 64] [--n-db 1400] [--out profiles/db_batch_bench.jsonl]

Written to --out, one JSON line each:
  round      host clock around a whole round (it ends synchronised), minimum and median of --reps, per path and per stage;
  calls      the three batched calls alone on the same inputs as host arrays and as device views: what a call costs beyond its
             kernels when its inputs are uploaded from pageable memory -- the upload's share of the host-array round;
  scan       mrbf_db_box_batch alone: event time of launches + read-back, GB/s of database bytes read once (n_db x d x 8 per start)
             and of all traffic (the rows again in the compaction, the two views written);
  gather     mrbf_db_gather_batch alone on the 257-row training sets: event time and GB/s (rows read + rows written).
The two paths' picks, accepted lists and weights are compared (equality) before anything is timed.  One GPU process."""
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
    ap.add_argument("--n-db", type=int, default=1400)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_batch_bench.jsonl"))
    args = ap.parse_args()
    import morbit.jl_amd as pkg
    from morbit.jl_amd import database, sampling
    from morbit.jl_amd import rbf_model as rm

    ctx = pkg.Context()
    ns, n_db, d, k = args.starts, args.n_db, args.d, 2
    cfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1, max_model_points=2 * d + 1)
    rng = np.random.default_rng(11)
    host, vals, dbs = [], [], []
    for p in range(ns):
        S = rng.uniform(-1.0, 1.0, (n_db, d))
        S[0] = 0.0
        S[5::10] *= 1.5                                   # a tenth of the rows outside the box
        V = np.stack([np.sum((S - 1.0) ** 2, axis=1), np.sum((S + 1.0) ** 2, axis=1)], axis=1)
        host.append(S), vals.append(V)
        dbs.append(database.DeviceDatabase(d, k, ctx=ctx, capacity=n_db))
        dbs[-1].append(S, V)
    xs, x_idx = [S[0].copy() for S in host], [0] * ns
    lb, ub = [x - 1.0 for x in xs], [x + 1.0 for x in xs]
    piv = 1e-3

    def round_host(t):
        t0 = time.perf_counter()
        r1 = sampling.find_suitable_points_many(host, lb, ub, xs, x_idx, piv, ctx=ctx)
        t1 = time.perf_counter()
        found = [[x_idx[p]] + r1[p][0] for p in range(ns)]
        acc = sampling.rbf_round4_many(host, lb, ub, xs, 1.0, found, cfg, ctx=ctx)
        t2 = time.perf_counter()
        train = [found[p] + acc[p] for p in range(ns)]
        mods = rm.update_models_many(cfg, [host[p][train[p]] for p in range(ns)], [vals[p][train[p]] for p in range(ns)], 1.0, ctx=ctx)
        t3 = time.perf_counter()
        t.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        return r1, acc, train, mods

    def round_resident(t):
        t0 = time.perf_counter()
        r1 = sampling.find_suitable_points_many(dbs, lb, ub, xs, x_idx, piv, ctx=ctx)
        t1 = time.perf_counter()
        found = [[x_idx[p]] + r1[p][0] for p in range(ns)]
        acc = sampling.rbf_round4_many(dbs, lb, ub, xs, 1.0, found, cfg, ctx=ctx)
        t2 = time.perf_counter()
        train = [found[p] + acc[p] for p in range(ns)]
        mods = rm.update_models_resident(cfg, dbs, train, 1.0, ctx=ctx)
        t3 = time.perf_counter()
        t.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        return r1, acc, train, mods

    def free(mods):
        for m in mods:
            m.free()

    # ---- the two paths agree (also the warm-up of every shape)
    a, b = round_host([]), round_resident([])
    assert [r[0] for r in a[0]] == [r[0] for r in b[0]] and a[1] == b[1], "the paths disagree"
    assert all(np.array_equal(ma.weights, mb.weights) for ma, mb in zip(a[3], b[3])), "the paths' models disagree"
    train = a[2]
    sizes = {"picks": int(np.mean([len(r[0]) for r in a[0]])), "candidates": int(np.mean([len(r[2]) for r in a[0]])),
             "accepted": int(np.mean([len(x) for x in a[1]])), "model_sites": int(np.mean([len(t) for t in train]))}
    free(a[3]), free(b[3])
    th, tr = [], []
    for _ in range(args.reps):                         # alternating
        free(round_host(th)[3])
        free(round_resident(tr)[3])
    stat = lambda t, i: {"min": float(np.min([x[i] for x in t])), "median": float(np.median([x[i] for x in t]))}
    names = ("round", "filter", "round4", "fit")
    rec = {"tool": "db_batch_bench", "what": "round", "n_starts": ns, "n_db": n_db, "d": d, "k": k, "reps": args.reps, **sizes,
           "host_ms": {nm: stat(th, i) for i, nm in enumerate(names)}, "resident_ms": {nm: stat(tr, i) for i, nm in enumerate(names)}}
    out = [rec]

    # ---- the three batched calls alone: host arrays against device views of the same bytes
    def best(f):
        f()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
            if isinstance(r, list):
                free(r)
        return float(np.min(ts)), float(np.median(ts))

    found = [train[p][: d + 1] for p in range(ns)]
    boxes = database.box_many(dbs, lb, ub, xs, [[0]] * ns, ctx=ctx)
    items_v, items_h = [], []
    for p, B in enumerate(boxes):
        qr = sampling._GrowingQR(d)
        qr.append(B.first_row)
        items_v.append((B.shifted, qr, d - 1, piv))
        items_h.append((np.asarray(B.shifted), qr, d - 1, piv))
    calls = {"affine_host": best(lambda: sampling.affine_select_batch_device(items_h, d, ctx=ctx)[0]),
             "affine_views": best(lambda: sampling.affine_select_batch_device(items_v, d, ctx=ctx)[0])}
    boxes4 = database.box_many(dbs, lb, ub, xs, found, zero_first_pick=False, ctx=ctx)
    starts = database.gather_many(dbs, found, ctx=ctx)
    r4_v = [(cfg, g.sites, B.sites, 1.0) for g, B in zip(starts, boxes4)]
    r4_h = [(cfg, np.asarray(g.sites), np.asarray(B.sites), 1.0) for g, B in zip(starts, boxes4)]
    calls["round4_host"] = best(lambda: sampling.rbf_round4_batch_device(r4_h, d, ctx=ctx)[0])
    calls["round4_views"] = best(lambda: sampling.rbf_round4_batch_device(r4_v, d, ctx=ctx)[0])
    sets = database.gather_many(dbs, train, ctx=ctx)
    fit_h = ([np.asarray(g.sites) for g in sets], [np.asarray(g.values) for g in sets])
    calls["fit_host"] = best(lambda: rm.update_models_many(cfg, fit_h[0], fit_h[1], 1.0, ctx=ctx))
    calls["fit_views"] = best(lambda: rm.update_models_many(cfg, [g.sites for g in sets], [g.values for g in sets], 1.0, ctx=ctx))
    upload = sum(calls[s + "_host"][0] - calls[s + "_views"][0] for s in ("affine", "round4", "fit"))
    out.append({"tool": "db_batch_bench", "what": "calls", "n_starts": ns, "min_median_ms": calls, "upload_ms": upload,
                "upload_share_of_host_round": upload / rec["host_ms"]["round"]["min"],
                "bytes_uploaded_MB": {"affine": sum(it[0].shape[0] for it in items_h) * d * 8e-6,
                                      "round4": sum(x[1].shape[0] + x[2].shape[0] for x in r4_h) * d * 8e-6,
                                      "fit": sum(s.shape[0] for s in fit_h[0]) * (d + k) * 8e-6}})

    # ---- the scan and the gather alone
    def event_ms(f):
        ms = []
        for _ in range(args.reps + 1):
            st = {}
            f(st)
            ms.append(st["ms_total"])
        return float(np.min(ms[1:])), float(np.median(ms[1:]))

    mc = sum(B.mc for B in boxes)
    scan = event_ms(lambda st: database.box_many(dbs, lb, ub, xs, [[0]] * ns, ctx=ctx, stats=st))
    db_bytes = ns * n_db * d * 8
    all_bytes = db_bytes + 3 * mc * d * 8          # the candidates' rows read again by the compaction, two views written
    out.append({"tool": "db_batch_bench", "what": "scan", "n_starts": ns, "n_db": n_db, "d": d, "candidates": mc, "event_ms_min_median": scan,
                "GBps_database_read_once": db_bytes / scan[0] * 1e-6, "GBps_all_traffic": all_bytes / scan[0] * 1e-6})
    gat = event_ms(lambda st: database.gather_many(dbs, train, ctx=ctx, stats=st))
    g_bytes = 2 * sum(len(t) for t in train) * (d + k) * 8
    out.append({"tool": "db_batch_bench", "what": "gather", "n_starts": ns, "rows": sum(len(t) for t in train), "event_ms_min_median": gat,
                "GBps_read_plus_written": g_bytes / gat[0] * 1e-6})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in out:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    for db in dbs:
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
