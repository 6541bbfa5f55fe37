"""CPU rehearsal of bench.py's own launcher (no GPU): `python bench.py --gpus 2` must start two ranks itself, shard the problems
p % world, gather the records of the many-start workloads and print ONE JSON line that says n_gpus = 2 -- never a 1-GPU number
for an N-GPU request (ADVICE bench.py:124).  Also: `--steps` / `ms_per_step`, and `--dump-outputs` (its sampling on
the CPU; what it writes, against the oracle, on the GPU)."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def _run(*flags, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=300, env=e)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, lines


def test_bench_spawns_its_own_ranks_dry_run():
    r, lines = _run("--gpus", "2", "--dry-run", "--config", "C4", "--steps", "2", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["dry_run"] is True and out["value"] is None
    assert out["config"]["problems_per_step"] == 64 and out["scaling"] == "strong"
    assert out["records"] == {"gathered": 64, "failed": 0, "worst_rel_residual": 0.0}
    assert len(out["rank_seconds"]) == 2


def test_bench_default_workload_is_c3_weak_scaling():
    r, lines = _run("--gpus", "2", "--dry-run", "--steps", "1", "--warmup", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["problems_per_step"] == 2
    assert out["config"]["n"] == 8192 and out["config"]["d"] == 64 and out["config"]["m"] == 10000


def test_bench_refuses_a_mismatched_world():
    # under an external launcher with the wrong rank count the script must fail, not report a smaller job
    r, lines = _run("--gpus", "4", "--dry-run", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and not lines
    assert "WORLD_SIZE" in (r.stderr + r.stdout)


def test_bench_needs_a_gpu_for_real_runs():
    import torch

    if torch.cuda.is_available():
        return
    r, lines = _run("--steps", "1", "--warmup", "0")
    assert r.returncode != 0 and not lines
    assert "GPU" in r.stderr


def test_bench_times_exactly_the_requested_steps():
    r, lines = _run("--dry-run", "--steps", "7", "--warmup", "0", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 7 and out["warmup"] == 0
    assert out["dry_run_cycles"] == 7                 # one problem per step: the timed region ran exactly 7 steps
    # ms_per_step is the timed region over the steps (the dry worker sleeps 1 ms per cycle)
    assert abs(out["ms_per_step"] - 1e3 * out["rank_seconds"][0] / 7) <= 1e-9 * out["ms_per_step"]
    assert out["ms_per_step"] >= 1.0
    # a many-start step is the whole batch; the warm-up steps are not counted
    r, lines = _run("--dry-run", "--config", "C4", "--problems", "5", "--steps", "3", "--warmup", "2",
                    env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["dry_run_cycles"] == 3 * 5 and out["ms_per_step"] >= 5.0


def test_bench_refuses_steps_it_cannot_time():
    for flags in (("--steps", "0"), ("--warmup", "-1"), ("--dump-outputs", "unused_dir")):
        r, lines = _run("--dry-run", *flags, env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
        assert r.returncode != 0 and not lines, flags


def _load_bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_dump_outputs_writes_everything_under_the_share():
    """A dump under its budget is the arrays as they are, fp64, one file per problem and array"""
    import tempfile

    import numpy as np
    import torch

    bench = _load_bench()
    rng = np.random.default_rng(0)
    V, J, W = rng.random((50, 2)), rng.random((50, 3, 2)), torch.from_numpy(rng.random((20, 2)))
    with tempfile.TemporaryDirectory() as tmp:
        info = bench.dump_outputs(tmp, {4: [("queries", {"values": V, "jacobians": J}), ("sites", {"weights": W})]}, 1)
        assert info["files"] == 3 and info["sampled"] == {}
        assert sorted(os.listdir(tmp)) == ["p004_jacobians.npy", "p004_values.npy", "p004_weights.npy"]
        for name, a in (("values", V), ("jacobians", J), ("weights", W.numpy())):
            got = np.load(os.path.join(tmp, "p004_%s.npy" % name))
            assert got.dtype == np.float64 and np.array_equal(got, a)


def test_dump_outputs_samples_fixed_rows_within_64mb():
    """C4-sized outputs (64 problems of 6450 x 128 x 2 Jacobians, 845 MB in all) are sampled: every problem stays within its share of
    64 MB, the rows kept are the same in every run and for every array of a group, and they are rows of the output, unchanged"""
    import tempfile

    import numpy as np
    import torch

    bench = _load_bench()
    P, m, d, k, n = 64, 6450, 128, 2, 257
    rows = torch.arange(m, dtype=torch.float64)
    V = rows[:, None].expand(m, k).contiguous()
    J = rows[:, None, None].expand(m, d, k).contiguous()
    W = torch.arange(n, dtype=torch.float64)[:, None].expand(n, k).contiguous()
    outputs = {p: [("queries", {"values": V + p, "jacobians": J + p}), ("sites", {"weights": W})] for p in (0, 63)}
    got = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as tmp:
            info = bench.dump_outputs(tmp, outputs, P)
            sizes = {f: os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp)}
            assert info["bytes"] == sum(sizes.values()) and info["files"] == 6
            for p in (0, 63):
                assert sum(s for f, s in sizes.items() if f.startswith("p%03d_" % p)) <= bench.DUMP_LIMIT_BYTES // P
            got.append({f: np.load(os.path.join(tmp, f)) for f in sizes})
    assert got[0].keys() == got[1].keys() and all(np.array_equal(got[0][f], got[1][f]) for f in got[0])
    for p in (0, 63):
        vals, jacs, w = (got[0]["p%03d_%s.npy" % (p, x)] for x in ("values", "jacobians", "weights"))
        keep = vals.shape[0]
        assert 0 < keep < m and info["sampled"][str(p)]["queries"] == [keep, m]
        idx = bench.dump_sample_rows(p, 0, m, keep)
        assert np.array_equal(vals[:, 0], idx + p) and np.array_equal(jacs[:, 5, 1], idx + p) and jacs.shape == (keep, d, k)
        assert np.all(np.diff(w[:, 0]) > 0) and set(w[:, 0]) <= set(range(n))
    assert not np.array_equal(got[0]["p000_values.npy"][:, 0], got[0]["p063_values.npy"][:, 0] - 63)  # problems sample their own rows


@pytest.mark.gpu
@pytest.mark.parametrize("config,extra", [("C2", ()), ("C4", ()), ("C4", ("--no-batch", "--workers", "1"))],
                         ids=["C2", "C4-batched", "C4-one-worker-two-problems"])
def test_bench_dump_outputs_are_what_the_path_computed(config, extra, tmp_path):
    """bench.py --dump-outputs on the GPU: the files hold the last timed step's outputs -- every problem checked against the oracle's
    fit of the same seeded problem -- and a second run with the same arguments writes the same numbers.  The third case puts both
    problems on one worker of the per-problem path (its own buffers for the second one)."""
    import numpy as np

    from morbit.jl_amd import workloads as wl
    from oracle import rbf_oracle as orc

    dirs = [tmp_path / "a", tmp_path / "b"]
    for dd in dirs:
        r, lines = _run("--config", config, "--problems", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-callers",
                        "--dump-outputs", str(dd), *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 2 and out["dump_outputs"]["sampled"] == {} and out["dump_outputs"]["bytes"] <= 64 * 10 ** 6
        assert out["config"]["batched"] == (config == "C4" and not extra)
        assert out["config"]["contexts_per_gpu"] == 1
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert names == (["p000_tail.npy", "p000_weights.npy"] if config == "C2" else
                     ["p%03d_%s.npy" % (p, x) for p in (0, 1) for x in ("jacobians", "values", "weights")])
    for f in names:
        a, b = np.load(dirs[0] / f), np.load(dirs[1] / f)
        assert a.dtype == np.float64 and np.isfinite(a).all()
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), f
    import morbit.jl_amd as pkg

    cfg = wl.CONFIGS[config]
    kid, a_, b_ = pkg.rbf_model._get_kernel_params(1.0, pkg.RbfConfig(kernel=cfg["kernel"], polynomial_degree=cfg["deg"]))
    rel = lambda x, y: np.abs(x - y).max() / max(1.0, np.abs(y).max())
    for p in ((0,) if config == "C2" else (0, 1)):
        C, Y, X = wl.problem(config, p)
        W = np.load(dirs[0] / ("p%03d_weights.npy" % p))
        if config == "C2":
            # build+solve only: the weights and tail coefficients interpolate the data at the sites
            L = np.load(dirs[0] / "p000_tail.npy")
            assert W.shape == (2048, 1) and L.shape == (33, 1)
            assert rel(orc.OracleModel(C, W, L, kid, a_, b_, cfg["deg"]).values(C), Y) < 1e-8
        else:
            ref = orc.fit(C, Y, kid, a_, b_, cfg["deg"])   # cond ~ 2e3 (tests/test_gpu_configs.py::test_c4_many_start_batch)
            assert rel(W, ref.w) < 1e-10, p
            assert rel(np.load(dirs[0] / ("p%03d_values.npy" % p)), ref.values(X)) < 1e-8, p
            assert rel(np.load(dirs[0] / ("p%03d_jacobians.npy" % p)), np.transpose(ref.jacs(X), (0, 2, 1))) < 1e-8, p
