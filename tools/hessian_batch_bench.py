"""Many-start model Hessians: one mrbf_eval_hessian_batch call of this build against the loop of mrbf_eval_hessian on a build of the
parent commit, at the shapes of DESIGN.md section 19's table -- the C4 model (d = 128, n = 257, k = 2, cubic with a degree-1 tail)
at m = 1 and m = 16 sites per start for 2, 4, 8, 16 and 64 starts, the C3 model (d = 64, n = 8192, multiquadric) and a d = 256,
n = 1024 model at m = 1 for 8 and 64 starts; all outputs, device-resident buffers.

    python tools/hessian_batch_bench.py --parent path/to/parent/libmrbf.so [--out profiles/hessian_batch_bench.jsonl] [--reps 30]

Both libraries live in this one process, each with a context of its own, and the cells alternate: parent loop, batch, this build's
loop, parent loop again, cell by cell.  Medians of `--reps` host-clock calls after 5 warm-ups, with their spread (min, max); the batch
call's event time beside them.  The models are mrbf_model_from_coeffs of the same random coefficients in both libraries.  Before
anything is timed two things are asserted, bit for bit: the batch's outputs equal the parent loop's, and this build's single call equals
the parent's single call (the kernel bodies moved into shared device functions; their arithmetic must not have).  A cell is admitted
where the batch takes at most 0.8 of the parent loop's median (mrbf_dispatch_hessian_batch_min_jobs).  Without
--parent the loop of this build stands in (label "self").  One JSON line per cell is appended to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (label, kernel, polynomial degree, d, n, k, m, jobs)
CELLS = ([("C4", "cubic", 1, 128, 257, 2, 1, ns) for ns in (2, 4, 8, 16, 64)] + [("C4", "cubic", 1, 128, 257, 2, 16, ns) for ns in (2, 4, 8, 16, 64)] +
         [("C3", "multiquadric", 1, 64, 8192, 2, 1, ns) for ns in (8, 64)] + [("d256", "multiquadric", 1, 256, 1024, 2, 1, ns) for ns in (8, 64)])
WARMUPS = 5


class Side:
    """one build of the library with a context of its own"""

    def __init__(self, path):
        from morbit.jl_amd import _lib

        self.lib = ctypes.CDLL(path)
        for name in ("mrbf_init", "mrbf_shutdown", "mrbf_last_error", "mrbf_model_from_coeffs", "mrbf_eval_hessian", "mrbf_free_model"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.h = _lib.c_vp()
        self.check(self.lib.mrbf_init(-1, ctypes.byref(self.h)))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("rc %d: %s" % (rc, (self.lib.mrbf_last_error(self.h) or b"").decode()))

    def model(self, C, W, L, kid, a, b, deg):
        from morbit.jl_amd import _lib

        h = _lib.c_vp()
        n, d = C.shape
        self.check(self.lib.mrbf_model_from_coeffs(self.h, n, d, W.shape[1], _lib.as_ptr(C), _lib.as_ptr(W), _lib.as_ptr(L), kid, a, b, deg, ctypes.byref(h)))
        return h

    def loop(self, models, Xs, Hs):
        from morbit.jl_amd import _lib

        for h, X, H in zip(models, Xs, Hs):
            self.check(self.lib.mrbf_eval_hessian(self.h, h, X.shape[0], _lib.as_ptr(X), 0, None, _lib.as_ptr(H), None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hessian_batch_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

    ctx = pkg.Context()
    new = Side(_lib.LIB_PATH)
    old = Side(os.path.abspath(args.parent)) if args.parent else new

    def timed(f):
        host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            f()
            host.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(host)), [float(np.min(host)), float(np.max(host))]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for label, kernel, deg, d, n, k, m, ns in CELLS:
        cfg = pkg.RbfConfig(kernel=kernel, polynomial_degree=deg)
        kid, a, b = pkg.rbf_model._get_kernel_params(1.0, cfg)
        rng = np.random.default_rng(20)
        coeffs = [(rng.uniform(-2.0, 2.0, (n, d)), rng.standard_normal((n, k)) / n, rng.standard_normal((d + 1, k))) for _ in range(ns)]
        dev = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
        Xs = [torch.tensor(rng.uniform(-2.0, 2.0, (m, d)), dtype=torch.float64, device="cuda") for _ in range(ns)]
        Ho, Hn, Hs = ([dev(m, k, d, d) for _ in range(ns)] for _ in range(3))
        old_models = [old.model(C, W, L, kid, a, b, deg) for C, W, L in coeffs]
        new_models = [new.model(C, W, L, kid, a, b, deg) for C, W, L in coeffs] if new is not old else old_models
        mine = [pkg.rbf_model.model_from_coeffs(cfg, C, W, L, ctx=ctx) for C, W, L in coeffs]
        jobs = (_lib.HessJob * ns)()
        for p in range(ns):
            jobs[p].model, jobs[p].m, jobs[p].X = mine[p].model.value, m, Xs[p].data_ptr()
            jobs[p].rows, jobs[p].n_rows, jobs[p].hess_out = None, 0, Hn[p].data_ptr()
        info = _lib.HessBatchInfo()

        def batch():
            ctx.check(ctx.lib.mrbf_eval_hessian_batch(ctx.h, ns, jobs, ctypes.byref(info)))

        parent_loop = lambda: old.loop(old_models, Xs, Ho)
        self_loop = lambda: new.loop(new_models, Xs, Hs)
        # bit identity before anything is timed: the batch against the parent's loop, this build's single call against the parent's
        parent_loop()
        batch()
        self_loop()
        torch.cuda.synchronize()
        assert not any(torch.isnan(H).any().item() for H in Hn + Ho + Hs), "a result was not written"
        assert all(torch.equal(Ho[p], Hn[p]) for p in range(ns)), "the batch does not reproduce the parent's loop of single calls"
        assert all(torch.equal(Ho[p], Hs[p]) for p in range(ns)), "this build's single call does not reproduce the parent's single call"
        rec = {"tool": "hessian_batch_bench", "parent": "parent" if args.parent else "self", "model": label, "kernel": kernel, "jobs": ns, "d": d,
               "n": n, "k": k, "m": m, "reps": args.reps, "batch_equals_parent_loop": True, "single_equals_parent_single": True,
               "nsplit": int(jobs[0].nsplit), "groups": int(info.groups), "chunks": int(info.chunks)}
        for _ in range(WARMUPS):
            parent_loop(), batch(), self_loop()
        rec["parent_loop_host_ms"], rec["parent_loop_host_ms_min_max"] = timed(parent_loop)
        rec["batch_host_ms"], rec["batch_host_ms_min_max"] = timed(batch)
        rec["batch_event_ms"] = float(info.ms_total)
        rec["self_loop_host_ms"], rec["self_loop_host_ms_min_max"] = timed(self_loop)
        rec["parent_loop_host_ms_again"], _ = timed(parent_loop)      # the spread between two passes of the same thing
        rec["ratio"] = rec["batch_host_ms"] / rec["parent_loop_host_ms"]
        rec["admitted"] = rec["ratio"] <= 0.8
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        for h in old_models:
            old.check(old.lib.mrbf_free_model(old.h, h))
        if new is not old:
            for h in new_models:
                new.check(new.lib.mrbf_free_model(new.h, h))
        for mod in mine:
            mod.free()
    ctx.close()


if __name__ == "__main__":
    main()
