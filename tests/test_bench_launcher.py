"""bench.py's own multi-rank launcher (`--gpus N` without torchrun) and its CPU-baseline leg, on the CPU:
the launcher path runs with the gloo backend over the TEST-ONLY host build of the engine (`--engine host`)."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*args, timeout=300):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                         timeout=timeout, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout  # one JSON line, from rank 0 only
    return json.loads(lines[0])


def test_launcher_two_ranks_host_engine():
    sys.path.insert(0, os.path.join(REPO, "tests", "hostsim"))
    import driver

    driver.build()
    B, K, W = 8, 5, 2
    line = _run_bench("--engine", "host", "--gpus", "2", "--steps", str(K), "--warmup", str(W), "--envs", str(B),
                      "--preroll", "60", "--no-cpu-baseline")
    assert line["n_gpus"] == 2 and line["steps"] == K and line["warmup"] == W
    # lockstep with auto-reset: every env of both ranks takes exactly K timed decisions, summed over ranks
    assert line["decisions"] == 2 * B * K
    assert line["config"]["parallelism"] == "env-sharded x2"
    assert line["frozen_envs"] == 0 and line["roofline"] is None
    # the process group held both ranks, and what each rank measured adds up to the reported total
    assert line["ranks_seen"] == 2
    assert sorted(r["rank"] for r in line["per_rank"]) == [0, 1]
    assert sum(r["decisions"] for r in line["per_rank"]) == line["decisions"]
    assert all(r["decisions"] == B * K for r in line["per_rank"])
    assert max(r["elapsed_s"] for r in line["per_rank"]) <= line["ms_per_step"] * K / 1e3 + 1e-9


def test_launcher_one_rank_reports_ranks_seen():
    sys.path.insert(0, os.path.join(REPO, "tests", "hostsim"))
    import driver

    driver.build()
    line = _run_bench("--engine", "host", "--steps", "3", "--warmup", "1", "--envs", "4", "--preroll", "20",
                      "--no-cpu-baseline")
    assert line["n_gpus"] == 1 and line["ranks_seen"] == 1
    assert [r["rank"] for r in line["per_rank"]] == [0] and line["per_rank"][0]["decisions"] == line["decisions"]


def test_dump_outputs_host_engine(tmp_path):
    """`--dump-outputs DIR`: float32 / float64 .npy files of the final observations, identical from run to run, and
    the line names them; `--full` is accepted (the host engine never runs the CPU baseline)."""
    import numpy as np

    sys.path.insert(0, os.path.join(REPO, "tests", "hostsim"))
    import driver

    driver.build()
    B, K = 6, 4
    args = ("--engine", "host", "--steps", str(K), "--warmup", "1", "--envs", str(B), "--preroll", "30")
    a = _run_bench(*args, "--dump-outputs", str(tmp_path / "a"))
    b = _run_bench(*args, "--full", "--dump-outputs", str(tmp_path / "b"))
    assert a["steps"] == K and a["ms_per_step"] > 0 and a["cpu_baseline"] is None and b["cpu_baseline"] is None
    assert a["outputs"]["arrays"] == b["outputs"]["arrays"] and a["outputs"]["comparable"]
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == a["outputs"]["arrays"] and {"counts", "nodes", "wall_time", "acc", "env_index"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and x.shape[0] == B, n
        assert np.array_equal(x, y) and np.isfinite(x).all(), n
        total += x.nbytes
    assert total == a["outputs"]["bytes"] <= 64 << 20
    # the dump is the run's own state: the decisions of the current episodes are in it
    from spark_sched_sim import _abi

    assert np.load(tmp_path / "a" / "counts.npy")[:, _abi.OC_DECISIONS].sum() > 0


@pytest.mark.gpu
def test_dump_outputs_budget_rollout_is_reproducible(gpu_device, tmp_path):
    """The default (shared-budget, preemptible) timed path with `--dump-outputs`: the split of the budget over the envs
    varies from run to run, the dump does not. Every env ends at 8 x (warmup + steps) decisions after its pre-roll
    (the launches' per-env cap), with no step pending and no error, and two runs write the same arrays bit for bit."""
    import numpy as np

    from spark_sched_sim import _abi

    B, K, W, P = 96, 12, 3, 200
    args = ("--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs", str(B), "--preroll", str(P))
    a = _run_bench(*args, "--dump-outputs", str(tmp_path / "a"))
    b = _run_bench(*args, "--dump-outputs", str(tmp_path / "b"))
    assert a["cpu_baseline"] is None and a["outputs"]["comparable"] and a["config"]["work_sharing"].startswith("shared")
    for n in a["outputs"]["arrays"]:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y) and np.isfinite(x).all(), n
    # a job still running has no completion time: written as -1, never as inf; a completed one has a real time
    tc, st = np.load(tmp_path / "a" / "job_t_completed.npy"), np.load(tmp_path / "a" / "job_state.npy")
    assert ((tc >= 0) == (st == 2)).all() and (st != 2).any()
    pre =np.random.default_rng([0, 0, 7]).integers(0, P, B)  # bench.py's pre-roll draw (seed 0, rank 0)
    acc, counts = np.load(tmp_path / "a" / "acc.npy"), np.load(tmp_path / "a" / "counts.npy")
    assert np.array_equal(acc[:, _abi.ACC_DECISIONS], pre + 8 * (W + K))
    assert not counts[:, _abi.OC_ERR].any()


@pytest.mark.parametrize("workload", ["tpch", "decima"])
def test_cpu_baseline_worker(workload):
    import bench

    dec, wall, _, _ = bench._cpu_worker((workload, 3, 1.0, 0.5, 0))
    assert dec > 0 and wall >= 1.0
    assert bench.usable_cpus() >= 1 and isinstance(bench.cpu_model(), str)
