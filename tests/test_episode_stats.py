"""Per-env episode statistics (ssim_episode_stats, csrc/sparksched.hip k_episode_stats; the host build's serial loop)
against evaluate.avg_job_durations, and evaluate_policy on top of them: the heuristic kinds unchanged, the "decima" kind
(greedy and sampled persistent rollouts of a DecimaScheduler) against the oracle env replaying its action log."""

import numpy as np
import pytest
import torch

from spark_sched_sim import _abi
from spark_sched_sim.evaluate import avg_job_durations, evaluate_policy, job_table_stats, stats_avg_job_durations

TPCH = dict(job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
J50 = dict(TPCH, num_executors=10, job_arrival_cap=50)
J200 = dict(TPCH, num_executors=50, job_arrival_cap=200, job_arrival_rate=1.0e-4)


def check_stats(eng, what):
    """episode_stats() against the job tables: the counts and the wall time exact, the mean to 1e-12 relative (nan for an
    env with no arrived job in both)."""
    stats = np.asarray(eng.episode_stats())
    ta, tc, st = (np.asarray(x) for x in eng.job_times_np())
    wall = np.asarray(eng.host_views()["wall_time"], dtype=np.float64)
    assert stats.shape == (eng.num_envs, 4) and stats.dtype == np.float64, what
    assert stats[:, 1].tolist() == (st > 0).sum(axis=1).tolist(), what
    assert stats[:, 2].tolist() == (st == 2).sum(axis=1).tolist(), what
    assert stats[:, 3].tolist() == wall.tolist(), what
    np.testing.assert_allclose(job_table_stats(eng), stats, rtol=1e-12, atol=0.0, err_msg=what)
    want, got = avg_job_durations(eng), stats_avg_job_durations(stats)
    assert np.array_equal(np.isnan(want), np.isnan(got)), what
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0.0, err_msg=what)
    return stats


@pytest.mark.parametrize("cfg", [J50, J200], ids=["j50", "j200"])
def test_episode_stats_host(dataset, cfg):
    """The host build: a freshly reset env before any decision, running envs (jobs active and pending: the duration of an
    unfinished job runs to the wall time), and, at J = 50, terminated envs."""
    from host_episode_stats import StatsHostEngine

    B = 3
    eng = StatsHostEngine(cfg, B, dataset)
    eng.reset(seeds=[5, 6, 7])
    fresh = check_stats(eng, "after reset")
    assert (fresh[:, 2] == 0).all() and (fresh[:, 3] == 0).all()
    eng.rollout(_abi.SSIM_POLICY_FAIR, 0, 150)
    running = check_stats(eng, "running")
    assert (running[:, 1] > running[:, 2]).all() and (running[:, 2] > 0).all()
    assert (running[:, 1] < cfg["job_arrival_cap"]).all()
    if cfg is J50:
        for _ in range(40):
            if np.asarray(eng.host_views()["counts"])[:, _abi.OC_TERMINATED].all():
                break
            eng.rollout(_abi.SSIM_POLICY_FAIR, 0, 256)
        done = check_stats(eng, "terminated")
        assert (done[:, 1] == 50).all() and (done[:, 2] == 50).all()
    eng.close()


def test_episode_stats_no_arrived_job_is_nan():
    """An env with no arrived job: 0 / 0 arrived jobs gives nan, as avg_job_durations does."""
    out = stats_avg_job_durations(np.array([[0.0, 0.0, 0.0, 0.0], [3000.0, 2.0, 1.0, 10.0]]))
    assert np.isnan(out[0]) and out[1] == 1.5


def test_evaluate_fair_keeps_its_numbers_host(dataset, env_cfg):
    """evaluate_policy("fair") on the host build returns what it returned when its numbers came from the job tables
    copied to the host: the values to 1e-12, the integer fields exactly."""
    from host_episode_stats import StatsHostEngine

    seeds = [21, 22, 23]
    kept = []

    def factory(cfg, B, ds):
        eng = StatsHostEngine(cfg, B, ds)
        close = eng.close

        def keep():  # the dict as the job tables give it, before the engine goes
            if eng.handle is None:  # (already closed: __del__ closes again)
                return
            c = np.asarray(eng.host_views()["counts"])
            kept.append({"avg_job_duration": avg_job_durations(eng),
                         "completed_jobs": c[:, _abi.OC_NUM_COMPLETED].astype(np.int64),
                         "decisions": c[:, _abi.OC_DECISIONS].astype(np.int64),
                         "wall_time": np.asarray(eng.host_views()["wall_time"], dtype=np.float64).copy()})
            close()

        eng.close = keep
        return eng

    out = evaluate_policy(env_cfg, "fair", seeds, dataset=dataset, engine_factory=factory)
    want = kept[0]
    assert set(out) == set(want) | {"launches"} and out["launches"] >= 4
    np.testing.assert_allclose(out["avg_job_duration"], want["avg_job_duration"], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(out["wall_time"], want["wall_time"], rtol=1e-12, atol=0.0)
    for key in ("completed_jobs", "decisions"):
        assert out[key].dtype == np.int64 and out[key].tolist() == want[key].tolist(), key
    assert (out["completed_jobs"] == env_cfg["job_arrival_cap"]).all()


def test_evaluate_decima_arguments(dataset, env_cfg):
    from hostsim.driver import HostEngine

    with pytest.raises(ValueError, match="needs policy="):
        evaluate_policy(env_cfg, "decima", [1], dataset=dataset)
    with pytest.raises(ValueError, match="kind 'decima' only"):
        evaluate_policy(env_cfg, "fair", [1], dataset=dataset, policy=object())
    with pytest.raises(ValueError, match="no persistent Decima rollout"):
        evaluate_policy(env_cfg, "decima", [1], dataset=dataset, policy=object(),
                        engine_factory=lambda cfg, B, ds: HostEngine(cfg, B, ds))


# ------------------------------------------------------------------------------------------ on the device
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,B", [(J50, 64), (J200, 16)], ids=["j50_b64", "j200_n50_b16"])
def test_episode_stats_gpu(gpu_device, dataset, cfg, B):
    """After a 300-decision fair rollout: the device reduction against the job tables copied to the host."""
    from spark_sched_sim.engine import DeviceEngine

    eng = DeviceEngine(cfg, B, dataset, device=gpu_device)
    eng.reset(seeds=list(range(40, 40 + B)))
    check_stats(eng, "after reset")
    eng.rollout(_abi.SSIM_POLICY_FAIR, 0, 300)
    stats = check_stats(eng, "after 300 decisions")
    assert (stats[:, 2] > 0).all() and (stats[:, 1] > stats[:, 2]).any()
    eng.close()


def _replay(env_cfg, dataset, seed, actions):
    from oracle.restatement import SparkSchedOracle, avg_job_duration

    o = SparkSchedOracle(env_cfg, dataset)
    o.reset(seed=seed)
    term = False
    for si, ne in actions:
        assert not term
        _, _, term, _, _ = o.step({"stage_idx": int(si), "num_exec": int(ne)})
    assert term, "the oracle's episode goes on after the logged actions"
    return o, float(avg_job_duration(o)) * 1e-3


@pytest.mark.gpu
def test_evaluate_decima_gpu(gpu_device, dataset, tmp_path):
    """evaluate_policy("decima", greedy=True) from a checkpoint, 8 seeds at N = 10 / J = 20 to termination: decisions,
    completed jobs and wall times equal the oracle env replaying the run's action log, durations to 1e-12; the greedy
    run does not depend on policy_seed; greedy=False with a fixed policy_seed is reproducible, whatever the launch
    length, and differs from the greedy run."""
    from test_greedy_audit import policy_state

    cfg = dict(TPCH, num_executors=10, job_arrival_cap=20)
    seeds = list(range(300, 308))
    pol, _ = policy_state(10)
    pol.save(tmp_path / "pol.pt")
    logs = []
    out = evaluate_policy(cfg, "decima", seeds, device=gpu_device, dataset=dataset, policy=tmp_path / "pol.pt",
                          greedy=True, steps_per_launch=64, action_log=logs)
    assert out["launches"] == len(logs) >= 2
    log = np.concatenate(logs, axis=0)  # [launches * 64][B][2]
    for i, seed in enumerate(seeds):
        rows = log[:, i][log[:, i, 1] >= 1]
        assert len(rows) == out["decisions"][i]
        o, avg = _replay(cfg, dataset, seed, rows)
        assert out["completed_jobs"][i] == sum(1 for j in o.jobs.values() if np.isfinite(j.t_completed)) == 20
        assert out["wall_time"][i] == float(o.wall_time)
        np.testing.assert_allclose(out["avg_job_duration"][i], avg, rtol=1e-12, atol=0.0)
    again = evaluate_policy(cfg, "decima", seeds, device=gpu_device, dataset=dataset, policy=pol.to(gpu_device),
                            greedy=True, policy_seed=99)
    for key in ("avg_job_duration", "completed_jobs", "decisions", "wall_time"):
        assert np.array_equal(out[key], again[key]), key
    sampled = [evaluate_policy(cfg, "decima", seeds, device=gpu_device, dataset=dataset, policy=pol, greedy=False,
                               policy_seed=7, steps_per_launch=k) for k in (256, 256, 50)]
    for other in sampled[1:]:
        for key in ("avg_job_duration", "completed_jobs", "decisions", "wall_time"):
            assert np.array_equal(sampled[0][key], other[key]), key
    assert not np.array_equal(sampled[0]["decisions"], out["decisions"])
