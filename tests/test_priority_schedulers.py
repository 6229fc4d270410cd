"""Shortest-job-first schedulers (SJF / SJF-CP) on the CPU: the host scheduler on hand-made observations, then the
device policy code through the test-only host build (both views: the obs arena's `policy(kind)` and the hot
block's fused rollout, which the host build also checks against each other at every decision) against the oracle
driven by the host scheduler (cases_priority.py). The gfx950 kernels run the same cases in test_gpu_priority.py."""

import numpy as np
import pytest

import cases_priority as P
from spark_sched_sim import _abi
from spark_sched_sim.engine import GraphInstance
from spark_sched_sim.schedulers import (POLICY_KINDS, RoundRobinScheduler, ShortestJobFirstScheduler, host_scheduler,
                                        make_scheduler)


def _obs(nodes, edges, dag_ptr, committable=3):
    """A reference-format observation: nodes = (remaining tasks, most recent duration, schedulable) per row."""
    links = np.array(edges, dtype=np.int64).reshape(-1, 2)
    return {"dag_batch": GraphInstance(np.array(nodes, dtype=np.float32).reshape(-1, 3),
                                       np.zeros(len(links), dtype=np.int64), links),
            "dag_ptr": list(dag_ptr), "num_committable_execs": committable, "source_job_idx": len(dag_ptr) - 1,
            "exec_supplies": [0] * (len(dag_ptr) - 1)}


def _act(obs, critical_path):
    a, info = ShortestJobFirstScheduler(10, critical_path=critical_path).schedule(obs)
    assert info == {}
    return int(a["stage_idx"]), int(a["num_exec"])


@pytest.mark.parametrize("cp", [False, True])
def test_work_tie_goes_to_the_earlier_job(cp):
    # work 50, 10, 10 (2 x 5 and 1 x 10), 10: jobs 1, 2 and 3 tie, job 1 is served (its row 1 has rank 1)
    obs = _obs([(5, 10, 1), (2, 5, 1), (1, 10, 1), (10, 1, 1)], [], [0, 1, 2, 3, 4], committable=4)
    assert _act(obs, cp) == (1, 4)


@pytest.mark.parametrize("cp", [False, True])
def test_shortest_job_without_schedulable_stage_is_skipped(cp):
    # job 0 (work 1) has nothing schedulable; job 2 (work 6 = 2 + 4) beats job 1 (work 8); its rows 2, 3 have ranks 1, -
    obs = _obs([(1, 1, 0), (4, 2, 1), (2, 1, 1), (4, 1, 0)], [(2, 3)], [0, 1, 2, 4])
    assert _act(obs, cp) == (1, 3)


def test_critical_path_choice_differs_from_find_stage():
    # one job: rows 0 and 1 are frontier and schedulable, row 1 leads to the long row 2 (cp 1 + 100), row 0 to nothing
    obs = _obs([(1, 1, 1), (1, 1, 1), (10, 10, 0)], [(1, 2)], [0, 3])
    assert _act(obs, False) == (0, 3)  # find_stage: the first frontier row
    assert _act(obs, True) == (1, 3)
    # the rank is among ALL schedulable rows: a schedulable row of a longer job in front shifts it
    obs = _obs([(20, 9, 1), (1, 1, 1), (1, 1, 1), (10, 10, 0)], [(2, 3)], [0, 1, 4])
    assert _act(obs, True) == (2, 3)
    # a chain: cp adds up along the longest path (row 0: 1 + max(2 + 3, 4)), the non-frontier row 2 is schedulable
    obs = _obs([(1, 1, 0), (1, 2, 0), (1, 3, 1), (1, 4, 1)], [(0, 1), (0, 3), (1, 2)], [0, 4])
    assert _act(obs, True) == (1, 3)  # row 3 (cp 4) over row 2 (cp 3): rank 1


def test_critical_path_tie_goes_to_the_lowest_row():
    # row 0: 2 + 3 through its child row 2; row 1: 5 on its own
    obs = _obs([(1, 2, 1), (1, 5, 1), (1, 3, 0)], [(0, 2)], [0, 3])
    assert _act(obs, True) == (0, 3)
    obs = _obs([(1, 5, 0), (1, 2, 1), (1, 5, 1), (1, 3, 0)], [(1, 3)], [0, 4])
    assert _act(obs, True) == (0, 3)  # rows 1 and 2 tie at 5: row 1, rank 0


@pytest.mark.parametrize("cp", [False, True])
def test_no_candidate(cp):
    assert _act(_obs([(1, 1, 0), (2, 2, 0)], [], [0, 1, 2]), cp) == (-1, 3)
    assert _act(_obs([], [], [0]), cp) == (-1, 3)


def test_names_and_factories():
    s = make_scheduler({"agent_cls": "ShortestJobFirstScheduler", "num_executors": 7, "critical_path": True})
    assert isinstance(s, ShortestJobFirstScheduler) and s.name == "SJF-CP" and s.num_executors == 7
    assert ShortestJobFirstScheduler(3).name == "SJF"
    for bad in ("NoSuchScheduler", "make_scheduler", "POLICY_KINDS"):
        with pytest.raises(AssertionError):
            make_scheduler({"agent_cls": bad})
    assert POLICY_KINDS == {"fair": _abi.SSIM_POLICY_FAIR, "fifo": _abi.SSIM_POLICY_FIFO,
                            "random": _abi.SSIM_POLICY_RANDOM, "sjf": 4, "sjf-cp": 5}
    assert (_abi.SSIM_POLICY_SJF, _abi.SSIM_POLICY_SJF_CP) == (4, 5)
    assert [host_scheduler(n, 10).name for n in POLICY_KINDS] == ["Fair", "FIFO", "Random", "SJF", "SJF-CP"]
    assert isinstance(host_scheduler("fifo", 10), RoundRobinScheduler)
    with pytest.raises(ValueError):
        host_scheduler("lifo", 10)


def test_examples_accepts_the_new_names(capsys):
    from spark_sched_sim import examples

    with pytest.raises(SystemExit):
        examples.main(["--sched", "lifo"])
    err = capsys.readouterr().err
    assert "sjf-cp" in err and "sjf" in err.replace("sjf-cp", "")


@pytest.fixture(scope="module", params=[False, True], ids=["hbm", "lds"])
def make(request):
    """As test_hostsim_parity.py: `lds` emulates the device's LDS residency on a poisoned working copy."""
    from hostsim.driver import HostEngine

    def _make(cfg, B, ds, trace_cap):
        return HostEngine(cfg, B, ds, trace_cap=trace_cap, resident=request.param)

    return _make


@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_policy_lockstep_default(make, dataset, env_cfg, name):
    P.case_policy_lockstep(make, dataset, env_cfg, name, False, P.DEFAULT_SEEDS)


@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_policy_lockstep_overloaded(make, dataset, env_cfg, name):
    P.case_policy_lockstep(make, dataset, env_cfg, name, True, P.OVERLOADED_SEEDS[:2])


@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_fused_rollout_default(make, dataset, env_cfg, name):
    P.case_fused_rollout(make, dataset, env_cfg, name, False, P.DEFAULT_SEEDS)


@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_fused_rollout_overloaded(make, dataset, env_cfg, name):
    P.case_fused_rollout(make, dataset, env_cfg, name, True, P.OVERLOADED_SEEDS)


@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_wide_jobs(make, env_cfg, name):
    P.case_wide_jobs(make, env_cfg, name)


@pytest.mark.parametrize("name", ["sjf", "sjf-cp", "fair"])
def test_evaluate_policy(dataset, env_cfg, name):
    from hostsim.driver import HostEngine

    out = P.case_evaluate(name, env_cfg, dataset, P.DEFAULT_SEEDS,
                          engine_factory=lambda cfg, B, ds: HostEngine(cfg, B, ds))
    assert out["launches"] >= 4 and (out["completed_jobs"] == env_cfg["job_arrival_cap"]).all()


def test_evaluate_policy_arguments(dataset, env_cfg):
    from hostsim.driver import HostEngine
    from spark_sched_sim.evaluate import evaluate_policy, policy_kind

    assert policy_kind("sjf-cp") == policy_kind(5) == _abi.SSIM_POLICY_SJF_CP
    for bad in ("lifo", 6, 0):
        with pytest.raises(ValueError):
            policy_kind(bad)
    with pytest.raises(RuntimeError, match="still running after 1 launches"):
        evaluate_policy(env_cfg, "sjf", [77], dataset=dataset, max_launches=1, steps_per_launch=10,
                        engine_factory=lambda cfg, B, ds: HostEngine(cfg, B, ds))


def test_run_episode_sjf_matches_oracle(dataset, env_cfg):
    """The facade episode of `examples.py --sched sjf` (one step per call, the host scheduler choosing)."""
    from spark_sched_sim.examples import run_episode

    from hostsim.driver import HostEngine

    got = run_episode(env_cfg, host_scheduler("sjf", env_cfg["num_executors"]), seed=77, dataset=dataset,
                      _engine_factory=lambda cfg, ds: HostEngine(cfg, 1, ds))
    assert np.isclose(got, P.oracle_episode(env_cfg, "sjf", 77).avg_job_duration, rtol=1e-12)
