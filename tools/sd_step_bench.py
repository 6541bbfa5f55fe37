"""Times one mrbf_sd_step call (the whole steepest-descent step: sigma, trial points, their values, the Armijo stop) against
(a) the host mirror descent.compute_descent_step_sd (sigma on the host, one batched sweep per objective model) and
(b) a sequential per-site loop that stands in for HipRbf.jl's fallback to Morbit's `_backtrack`: one single-site evaluation per
    objective model and loop iteration, as descent.jl:150-185 makes them.
Containers with 1, 2 and 3 objective models, d = 2, 12, 64, 256, each sigma branch, few and many loops.  Every timing is the median
of 30 host-clock calls that each end in a stream synchronisation; the device call's hipEvent time (info.ms_total) is reported too.
Writes profiles/sd_step_bench.jsonl (one line per case).  Run on the GPU: python tools/sd_step_bench.py [out.jsonl]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import morbit.jl_amd as pkg  # noqa: E402
from morbit.jl_amd import descent  # noqa: E402
from morbit.jl_amd import surrogates as sg  # noqa: E402

REPS = 30


def fit(f, d, rng, kernel):
    C = rng.uniform(-2.0, 2.0, (max(40, 2 * d + 20), d))
    Y = np.atleast_2d(f(C)).reshape(C.shape[0], -1)
    return pkg.update_model(pkg.RbfConfig(kernel=kernel, polynomial_degree=1), C, Y)


def objectives(d, n_models, rng):
    fa = lambda X: np.sum((X - 1.0) ** 2, axis=1)
    fb = lambda X: np.sum((X + 1.0) ** 2, axis=1)
    fc = lambda X: np.sum(X ** 2, axis=1) + X[:, 0]
    if n_models == 1:
        m = fit(lambda X: np.stack([fa(X), fb(X)], axis=1), d, rng, "multiquadric")
        return [sg.RefSurrogate(m, [0, 1])]
    ms = [fit(fa, d, rng, "cubic"), fit(fb, d, rng, "multiquadric"), fit(fc, d, rng, "gaussian")][:n_models]
    return [sg.RefSurrogate(m, [0]) for m in ms]


def per_site_step(cfg, sc, x, x_n, delta, lb, ub, omega, d, lin):
    """the reference's sequential loop: sigma on the host, then one single-site container evaluation per iteration"""
    sigma, _ = descent._sd_stepsize(x, x_n, delta, lb, ub, d, lin, None)
    if not sigma > cfg.min_stepsize:
        return 0, x_n, sg.eval_container_objectives_at_scaled_site(sc, None, x_n), 0, 0
    mx = sg.eval_container_objectives_at_scaled_site(sc, None, x_n)
    step = sigma
    xp = x_n + step * d
    mxp = sg.eval_container_objectives_at_scaled_site(sc, None, xp)
    i = 0
    while i < cfg.max_loops:
        if descent._armijo_condition(cfg.strict_backtracking, mx, mxp, step, omega, cfg.armijo_const_rhs):
            break
        if step <= cfg.min_stepsize:
            break
        step *= cfg.armijo_const_shrink
        xp = x_n + step * d
        mxp = sg.eval_container_objectives_at_scaled_site(sc, None, xp)
        i += 1
    return omega, xp, mxp, float(np.max(np.abs(step * d))), i


def median_ms(fn):
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main(out_path):
    rows = []
    cfg = descent.SteepestDescentConfig()
    for n_models in (1, 2, 3):
        for d in (2, 12, 64, 256):
            rng = np.random.default_rng(7 * d + n_models)
            sc = sg.SurrogateContainer(objectives=objectives(d, n_models, rng))
            plan = sg.container_plan(sc)
            lb, ub = np.full(d, -2.0), np.full(d, 2.0)
            x = rng.uniform(-0.5, 0.5, d)
            G = sg.eval_container_objectives_jacobian_at_scaled_site(sc, None, x)
            dd = -G.sum(axis=0)
            dd /= np.max(np.abs(dd))
            omega = 0.5 * max(1e-3, float(np.min(-(G @ dd))))
            lin = (np.zeros((0, d)), np.zeros(0), (dd / np.linalg.norm(dd))[None, :], np.array([x @ dd / np.linalg.norm(dd) + 0.6]))
            # -(sum of the gradients) is a common descent direction for some containers only (few loops); an ascent direction
            # runs the loop to min_stepsize (many loops).  The regime is recorded from the measured loop count.
            cases = [("delta", 0.3, dd), ("one", 3.0, 0.5 * dd), ("intersect", 3.0, dd), ("delta", 0.3, -dd)]
            for branch, delta, direction in cases:
                args = (cfg, sc, None, x, x, delta, lb, ub, omega, direction, lin)
                rc, _, _, info = descent.sd_step_device(plan, cfg, x, x, delta, lb, ub, omega, direction, lin)
                assert rc == 0 and info["branch_name"] == branch, (branch, info)
                ref = descent.compute_descent_step_sd(*args)
                seq = per_site_step(cfg, sc, x, x, delta, lb, ub, omega, direction, lin)
                assert np.array_equal(seq[1], ref[1]), "the per-site loop must stop where the mirror does"
                ev = []

                def dev():
                    ev.append(descent.sd_step_device(plan, cfg, x, x, delta, lb, ub, omega, direction, lin)[3]["ms_total"])

                t_dev = median_ms(dev)
                t_host = median_ms(lambda: descent.compute_descent_step_sd(*args))
                t_seq = median_ms(lambda: per_site_step(cfg, sc, x, x, delta, lb, ub, omega, direction, lin))
                row = dict(models=n_models, d=d, branch=branch, regime="few" if info["loops"] <= 5 else "many", loops=int(info["loops"]), sigma=float(info["sigma"]),
                           device_ms=round(t_dev, 4), device_event_ms=round(float(np.median(ev)), 4), host_mirror_ms=round(t_host, 4),
                           per_site_ms=round(t_seq, 4), per_site_ms_per_iteration=round(t_seq / (seq[4] + 2), 4),
                           host_wins=bool(min(t_host, t_seq) < t_dev))
                rows.append(row)
                print(json.dumps(row), flush=True)
    with open(out_path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sd_step_bench.jsonl"))
