"""Many-start evaluation at the C4 shape (d = 128, n = 257, k = 2, cubic with a degree-1 tail, device-resident buffers): one
mrbf_eval_batch call of this build against the loop of mrbf_eval on a build of the parent commit, for 8, 16 and 64 jobs, each with
m = 6450 values + Jacobians (the C4 evaluation) and with m = 2 values only (the acceptance test), and one d = 3, n = 20 row.

    python tools/eval_batch_bench.py --parent path/to/parent/libmrbf.so [--out profiles/eval_batch_bench.jsonl] [--reps 30]

Both libraries live in this one process, each with a context of its own, and the cells alternate: parent loop, batch, this build's
loop, cell by cell.  Medians of `--reps` host-clock calls with their spread (min, max); the batch call's event time beside them.  The
models are mrbf_model_from_coeffs of the same random coefficients in both libraries, and the batch's outputs are compared with the
parent loop's bit for bit before anything is timed.  A cell is admitted where the batch takes at most 0.8 of the parent loop's median
(mrbf_dispatch_eval_batch_min_jobs).  Without --parent the loop of this build stands in (label "self").  One JSON
line per cell is appended to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (d, n, k, m, want_jac, jobs)
CELLS = [(128, 257, 2, 6450, True, ns) for ns in (8, 16, 64)] + [(128, 257, 2, 2, False, ns) for ns in (8, 16, 64)] + [(3, 20, 2, 2, False, 64)]


class Side:
    """one build of the library with a context of its own"""

    def __init__(self, path):
        from morbit.jl_amd import _lib

        self.lib = ctypes.CDLL(path)
        for name in ("mrbf_init", "mrbf_shutdown", "mrbf_last_error", "mrbf_model_from_coeffs", "mrbf_eval", "mrbf_free_model"):
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

    def loop(self, models, Xs, Vs, Js):
        from morbit.jl_amd import _lib

        for h, X, V, J in zip(models, Xs, Vs, Js):
            self.check(self.lib.mrbf_eval(self.h, h, X.shape[0], _lib.as_ptr(X), _lib.as_ptr(V), _lib.as_ptr(J), None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_batch_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

    ctx = pkg.Context()
    new = Side(_lib.LIB_PATH)
    old = Side(os.path.abspath(args.parent)) if args.parent else new
    deg = 1
    kid, a, b = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel="cubic", polynomial_degree=deg))

    def timed(f):
        host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            f()
            host.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(host)), [float(np.min(host)), float(np.max(host))]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for d, n, k, m, want_jac, ns in CELLS:
        rng = np.random.default_rng(18)
        coeffs = [(rng.uniform(-2.0, 2.0, (n, d)), rng.standard_normal((n, k)) / n, rng.standard_normal((d + 1, k))) for _ in range(ns)]
        dev = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
        Xs = [torch.tensor(rng.uniform(-2.0, 2.0, (m, d)), dtype=torch.float64, device="cuda") for _ in range(ns)]
        Vo, Vn = [dev(m, k) for _ in range(ns)], [dev(m, k) for _ in range(ns)]
        Jo = [dev(m, d, k) if want_jac else None for _ in range(ns)]
        Jn = [dev(m, d, k) if want_jac else None for _ in range(ns)]
        old_models = [old.model(C, W, L, kid, a, b, deg) for C, W, L in coeffs]
        new_models = [new.model(C, W, L, kid, a, b, deg) for C, W, L in coeffs] if new is not old else old_models
        mine = [pkg.rbf_model.model_from_coeffs(pkg.RbfConfig(kernel="cubic", polynomial_degree=deg), C, W, L, ctx=ctx) for C, W, L in coeffs]
        jobs = (_lib.EvalJob * ns)()
        for p in range(ns):
            jobs[p].model, jobs[p].m, jobs[p].X = mine[p].model.value, m, Xs[p].data_ptr()
            jobs[p].vals_out, jobs[p].jac_out = Vn[p].data_ptr(), (Jn[p].data_ptr() if want_jac else None)
        ms = ctypes.c_float()

        def batch():
            ctx.check(ctx.lib.mrbf_eval_batch(ctx.h, ns, jobs, ctypes.byref(ms)))

        parent_loop = lambda: old.loop(old_models, Xs, Vo, Jo)
        self_loop = lambda: new.loop(new_models, Xs, Vo, Jo)
        # bit identity before anything is timed
        parent_loop()
        batch()
        torch.cuda.synchronize()
        same = all(torch.equal(Vo[p], Vn[p]) and (not want_jac or torch.equal(Jo[p], Jn[p])) for p in range(ns))
        assert same and not any(torch.isnan(V).any().item() for V in Vn), "the batch does not reproduce the parent's loop of single calls"
        rec = {"tool": "eval_batch_bench", "parent": "parent" if args.parent else "self", "jobs": ns, "d": d, "n": n, "k": k, "m": m,
               "jacobians": want_jac, "reps": args.reps, "bit_identical": True}
        for _ in range(3):
            parent_loop(), batch()
        rec["parent_loop_host_ms"], rec["parent_loop_host_ms_min_max"] = timed(parent_loop)
        rec["batch_host_ms"], rec["batch_host_ms_min_max"] = timed(batch)
        rec["batch_event_ms"] = float(ms.value)
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
