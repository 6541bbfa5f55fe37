"""Many-start / many-problem mode: independent RBF build+solve+eval problems sharded over GPUs.

The reference parallelises exactly this way, on CPU threads: `Threads.@threads` over the rows of the
benchmark table (/root/reference/examples/large_scale_benchmarks.jl:253), Halton start points (:102-109).
Here: one process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI), problems dealt
round-robin, NO data-path collective (no problem is split across GPUs); one all_gather of small
fixed-size result records at the end of the batch (latency-bound, tens of KB).
"""
import numpy as np

RECORD_FIELDS = ("problem_id", "status", "path", "rel_residual", "checksum_w", "checksum_vals", "ms_fit", "ms_eval")
RECORD_LEN = len(RECORD_FIELDS)


def shard_indices(n_problems, rank, world_size):
    """round-robin: problem p runs on rank p % world_size"""
    return list(range(rank, n_problems, world_size))


def gpu_solve_problem(problem, ctx=None):
    """fit + eval of one problem dict on this rank's GPU through the C ABI -> record (list of floats)"""
    from . import rbf_model as rm

    cfg = problem["cfg"]
    mod = rm.update_model(cfg, problem["sites"], problem["values"], problem.get("delta", 1.0), ctx=ctx)
    info = {}
    vals = jac = None
    if problem.get("X") is not None and len(problem["X"]):
        vals, jac = mod.eval_sites(problem["X"], want_values=True, want_jac=problem.get("want_jac", True), info=info)
    rec = [float(problem["id"]), 0.0, float(mod.info["path"]), float(mod.info["rel_residual"]),
           float(np.sum(mod.weights)), float(np.sum(vals)) if vals is not None else 0.0,
           float(mod.info["ms_total"]), float(info.get("ms_total", 0.0))]
    mod.free()
    return rec


def gpu_solve_shard_keep_models(problems, ctx=None, stats=None, eval_min_jobs=None):
    """fit + eval of a shard of problem dicts with the models KEPT: one `update_models_many` call fits all of them (mrbf_fit_batch where
    the decision table allows it), then one `eval_models_many` call evaluates all of them (mrbf_eval_batch where the decision table and
    its threshold say so, else one mrbf_eval per problem: the same bits either way).  Returns (records, models): a record per problem as
    `gpu_solve_problem` writes it (a failed fit: its status and NaNs, model None; the evaluation time of a problem that shared the one
    call is that call's), and the resident models in problem order -- what a many-start driver hands to `descent.sd_iterate_many`
    (wrapped in its containers) before it frees them.  stats["wide"]: how many problems with more than 512 sites shared the batch's
    launch (`update_models_many` asks mrbf_dispatch_fit_batch_max_n); stats["eval"]: `eval_models_many`'s own stats (eval_min_jobs: its
    `min_jobs`)."""
    from . import rbf_model as rm

    stats = stats if stats is not None else {}
    mods = rm.update_models_many([p["cfg"] for p in problems], [p["sites"] for p in problems], [p["values"] for p in problems],
                                 [p.get("delta", 1.0) for p in problems], ctx=ctx, stats=stats)
    todo = [i for i, (problem, mod) in enumerate(zip(problems, mods)) if mod is not None and problem.get("X") is not None and len(problem["X"])]
    est = {}
    got = rm.eval_models_many([mods[i] for i in todo], [problems[i]["X"] for i in todo], want_values=True,
                              want_jac=[problems[i].get("want_jac", True) for i in todo], stats=est, min_jobs=eval_min_jobs)
    stats["eval"] = est
    ms_eval = dict(zip(todo, est["ms_jobs"]))
    vals_of = {i: g[0] for i, g in zip(todo, got)}
    recs = []
    for i, (problem, mod, status) in enumerate(zip(problems, mods, stats["status"])):
        if mod is None:
            recs.append([float(problem["id"]), float(status) if status != 0 else -999.0] + [float("nan")] * (RECORD_LEN - 2))
            continue
        vals = vals_of.get(i)
        recs.append([float(problem["id"]), 0.0, float(mod.info["path"]), float(mod.info["rel_residual"]), float(np.sum(mod.weights)),
                     float(np.sum(vals)) if vals is not None else 0.0, float(mod.info["ms_total"]), float(ms_eval.get(i, 0.0))])
    return np.asarray(recs, dtype=np.float64).reshape(-1, RECORD_LEN), mods


def run_local_keep_models(problems, rank, world_size, ctx=None, stats=None):
    """this rank's shard through `gpu_solve_shard_keep_models`: (n_local x RECORD_LEN table, models of the shard in shard order)"""
    return gpu_solve_shard_keep_models([problems[p] for p in shard_indices(len(problems), rank, world_size)], ctx=ctx, stats=stats)


def run_local(problems, rank, world_size, solve=gpu_solve_problem, **kw):
    """solve this rank's shard; returns an (n_local x RECORD_LEN) float64 array"""
    recs = []
    for p in shard_indices(len(problems), rank, world_size):
        try:
            recs.append(solve(problems[p], **kw))
        except Exception as e:  # a failed factorisation must surface as a status, never take the batch down
            code = float(getattr(e, "code", -999))
            recs.append([float(problems[p]["id"]), code if code != 0 else -999.0] + [float("nan")] * (RECORD_LEN - 2))
    return np.asarray(recs, dtype=np.float64).reshape(-1, RECORD_LEN)


def gather_records(local, n_problems, device="cpu", group=None):
    """all_gather the per-rank record tables -> (n_problems x RECORD_LEN) table ordered by problem id on every rank.
    Works on any initialised torch.distributed backend (nccl on GPUs, gloo on CPU)."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        table = local
    else:
        world = dist.get_world_size(group)
        cap = (n_problems + world - 1) // world
        buf = torch.full((cap, RECORD_LEN), float("nan"), dtype=torch.float64, device=device)
        if len(local):
            buf[: len(local)] = torch.as_tensor(local, dtype=torch.float64, device=device)
        out = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(out, buf, group=group)
        table = torch.cat(out).cpu().numpy()
        table = table[~np.isnan(table[:, 0])]
    order = np.argsort(table[:, 0], kind="stable")
    return table[order]


def run_manystart(problems, rank=0, world_size=1, device="cpu", solve=gpu_solve_problem, group=None, **kw):
    local = run_local(problems, rank, world_size, solve=solve, **kw)
    return gather_records(local, len(problems), device=device, group=group)
