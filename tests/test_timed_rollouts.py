"""Fixed-duration Decima rollouts in persistent launches (ssim_decima_rollout_timed, csrc/decima_rollout.h timed mode;
trainers/rollouts.py DeviceAsyncRolloutCollector): RolloutWorkerAsync.collect_rollout (trainers/rollout_worker.py:
160-206) per env on the device, with reseeded in-place resets from a host-filled schedule.

CPU tests: the schedule helper against StochasticTimeLimitSampler called once per reset, and the inputs of the GPU
cases (whether an env resets is decided by its time limits, or in the small case by its 6-job episodes ending, not by
the policy). GPU tests: the recorded actions replayed on the oracle through the reference's async loop (small unit,
one schedule slot and a small arena, so refills and growths happen), equality with the lockstep AsyncRolloutCollector
on the shipped 50-executor units, argument validation, and PPO on a device engine.
"""

import numpy as np
import pytest
import torch

import parity
from oracle.restatement import SparkSchedOracle
from spark_sched_sim import _abi
from spark_sched_sim.engine import obs_dict
from spark_sched_sim.wrappers import StochasticTimeLimitSampler
from test_decima_audit import DENSE50

# cases.case_async_rollouts' own numbers (B = 6 rows, two per sequence)
SMALL = dict(cfg=dict(num_executors=4, job_arrival_cap=6, job_arrival_rate=1e-4), B=6,
             bases=[11 + i // 2 for i in range(6)], step=3, mean=4e5, duration=2.5e5, calls=3)
# the shipped units (dr_lds50 / dr_hbm50): base 703 draws 82823 ms first, so the fourth row takes another base
SHIPPED = dict(cfg=DENSE50, B=4, bases=[700, 701, 702, 723], step=4, mean=3e4, duration=4e4, calls=3)


def _cum_limits(case, n=3):
    return np.array([np.cumsum([np.random.RandomState(b + case["step"] * k).exponential(case["mean"])
                                for k in range(n)]) for b in case["bases"]])


# ---------------------------------------------------------------------------------------------- not gpu
@pytest.mark.parametrize("bases,step", [([11, 0, 7], 3), ([5, 0], 0)], ids=["step3", "step0"])
def test_reset_schedule_matches_sampler(bases, step):
    """Precompute cap_resets slots, consume some of them, precompute again and continue: the (seed, limit) sequence of
    every row equals, bit for bit, StochasticTimeLimitSampler.sample(e, base + step * k) called once per reset in order
    (a zero seed continues the row's RandomState; the draws of slots never consumed must not advance it)."""
    from spark_sched_sim.trainers.rollouts import ResetSchedule

    B, mean, cap = len(bases), 4e5, 3
    sampler = StochasticTimeLimitSampler(mean, B)
    sched = ResetSchedule(bases, step, sampler)
    count = np.zeros(B, dtype=np.int64)
    got = [[] for _ in range(B)]
    for e in range(B):  # reset 0 of every row runs on the host path (AsyncRolloutCollector._reset)
        seed = bases[e] + step * int(count[e])
        got[e].append((seed, sampler.sample(e, seed)))
        count[e] += 1
    for used in ([2, 0, 1], [0, 3, 3], [3, 1, 0], [1, 2, 2]):
        before = [r.get_state()[1].copy() for r in sampler.rngs]
        seeds, limits = sched.fill(count, cap)
        assert seeds.shape == limits.shape == (B, cap) and seeds.dtype == np.uint64 and limits.dtype == np.float64
        assert all((b == r.get_state()[1]).all() for b, r in zip(before, sampler.rngs)), "fill advanced the sampler"
        for e in range(B):
            n = used[e]
            sched.commit(e, seeds[e, :n], limits[e, :n])
            got[e] += [(int(seeds[e, k]), float(limits[e, k])) for k in range(n)]
            count[e] += n
    ref = StochasticTimeLimitSampler(mean, B)
    for e in range(B):
        want = [(bases[e] + step * k, ref.sample(e, bases[e] + step * k)) for k in range(len(got[e]))]
        assert got[e] == want, f"row {e}"
        assert len(got[e]) >= 5


def test_gpu_case_inputs():
    """The GPU cases' inputs from numpy alone. Shipped units: every env's first two limits sum to at most half of
    calls * duration, so each env resets at least once whatever the actions (the values are the issue's: 5108 / 14885 /
    15343, 3840 / 33128 / 74587, 5045 / 24060 / 81633 for bases 700-702). Small case (case_async_rollouts' numbers):
    rows 0-1 meet the same bound (79512 / 368084 / 507717); rows 2-5 do not (base 13 draws 601495 first), their
    resets come from their 6-job episodes terminating, which test_small_config_resets_on_host_build shows; rows 4-5
    have two consecutive limits inside the third call's window, the cap_resets = 1 refill."""
    c = _cum_limits(SHIPPED)
    assert np.round(c[:3]).tolist() == [[5108, 14885, 15343], [3840, 33128, 74587], [5045, 24060, 81633]]
    assert (c[:, 1] <= 0.5 * SHIPPED["calls"] * SHIPPED["duration"]).all(), c
    assert np.random.RandomState(703).exponential(SHIPPED["mean"]) > 0.5 * SHIPPED["calls"] * SHIPPED["duration"]
    s = _cum_limits(SMALL)
    assert np.round(s[0]).tolist() == [79512, 368084, 507717] and np.round(s[4]).tolist() == [601495, 702571, 743621]
    assert (s[:2, 1] <= 0.5 * SMALL["calls"] * SMALL["duration"]).all()
    d = SMALL["duration"]
    two_in_one = [(e, k) for e in range(SMALL["B"]) for k in range(2) if s[e, k] // d == s[e, k + 1] // d]
    assert two_in_one and all(s[e, k + 1] < SMALL["calls"] * d for e, k in two_in_one), s


def test_small_config_resets_on_host_build(dataset, env_cfg):
    """The small case's config through the lockstep AsyncRolloutCollector on the host build: some env resets twice in
    one call (the cap_resets = 1 refill of the GPU case) and there are at least B resets in all. The CPU policy may
    draw other actions than the GPU's: this validates the inputs, it is no parity check."""
    from hostsim.driver import HostEngine
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers import AsyncRolloutCollector

    c = SMALL
    eng = HostEngine(dict(env_cfg, **c["cfg"]), c["B"], dataset, trace_cap=0)
    torch.manual_seed(3)
    col = AsyncRolloutCollector(eng, DecimaScheduler(4), c["duration"], c["bases"], c["step"],
                                mean_time_limit=c["mean"], fused=True, seed=5)
    bufs = [col.collect() for _ in range(c["calls"])]
    per_call = [np.bincount([e for e, _ in b.resets], minlength=c["B"]) for b in bufs]
    assert max(int(n.max()) for n in per_call) >= 2, per_call
    assert sum(int(n.sum()) for n in per_call) >= c["B"], per_call


# ---------------------------------------------------------------------------------------------- gpu
def _call(buf):
    """One call's buffer on the host (the arena is reused by the next call): times, rewards, lengths, sample map,
    flat actions, observations, resets."""
    times, rewards, lengths, sample = buf.trajectories()
    obs, acts = buf.samples()
    if not getattr(buf, "row_major", False):
        from spark_sched_sim.schedulers.decima import select_envs

        canon = sample[sample >= 0]
        obs = select_envs(obs, canon)
        acts = {k: v[canon] for k, v in acts.items()}
    return dict(times=times.cpu(), rewards=rewards.cpu(), lengths=lengths.cpu(), sample=sample.cpu(),
                acts={k: v.cpu() for k, v in acts.items()}, obs=obs, resets=list(buf.resets))


@pytest.mark.gpu
def test_timed_collector_replays_on_oracle_gpu(gpu_device, dataset, env_cfg):
    """cases.case_async_rollouts' shape through DeviceAsyncRolloutCollector with ONE schedule slot and a 32-sample
    arena, the recorded actions replayed on the oracle through the reference's async loop: per env and call the
    decision count, every elapsed time bit for bit (the last included), rewards (parity.close_rel), the reset steps and
    the final observation."""
    from spark_sched_sim.engine import DeviceEngine
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers import AsyncRolloutCollector, DeviceAsyncRolloutCollector

    c = SMALL
    cfg, B, base, duration = dict(env_cfg, **c["cfg"]), c["B"], c["bases"], c["duration"]
    eng = DeviceEngine(cfg, B, dataset, device=gpu_device)
    torch.manual_seed(3)
    pol = DecimaScheduler(4).to(gpu_device)
    col = DeviceAsyncRolloutCollector(eng, pol, duration, base, c["step"], mean_time_limit=c["mean"], seed=5,
                                      cap_resets=1, cap_samples=32, cap_nodes=1 << 10, cap_edges=1 << 10,
                                      cap_dags=1 << 7)
    assert isinstance(col, AsyncRolloutCollector)
    calls = [_call(col.collect()) for _ in range(c["calls"])]
    assert not (eng.views["counts"][:, _abi.OC_ERR].cpu().numpy() & _abi.SSIM_ERR_STICKY).any()
    v = eng.host_views()
    total_resets = 0
    for e in range(B):
        o = SparkSchedOracle(cfg, dataset)
        rng, reset_count, limit = np.random.RandomState(42), 0, None

        def reset():
            nonlocal rng, reset_count, limit
            seed = base[e] + c["step"] * reset_count
            if seed:  # stochastic_time_limit.py:15-16
                rng = np.random.RandomState(seed)
            limit = float(rng.exponential(c["mean"]))
            ob, _ = o.reset(seed=seed, options={"time_limit": limit})
            reset_count += 1
            return ob

        ob = reset()
        next_wall = 0.0
        for ci, b in enumerate(calls):
            times, rewards, sample = b["times"], b["rewards"], b["sample"]
            si, ne = b["acts"]["stage_idx"].numpy(), 1 + b["acts"]["exec_idx"].numpy()
            n = int(b["lengths"][e])
            elapsed, k, resets = 0.0, 0, []
            while elapsed < duration:
                wall = next_wall
                assert k < n, f"env{e} call{ci}: device stopped after {n} decisions, oracle continues"
                i = int(sample[e, k])
                ob, rew, term, trunc, info = o.step({"stage_idx": int(si[i]), "num_exec": int(ne[i])})
                trunc = trunc or info["wall_time"] >= limit
                assert float(times[e, k]) == elapsed, f"env{e} call{ci} step{k} elapsed"
                assert parity.close_rel(float(rewards[e, k]), rew), f"env{e} call{ci} step{k} reward"
                next_wall = info["wall_time"]
                elapsed += next_wall - wall
                if term or trunc:
                    ob = reset()
                    next_wall = 0.0
                    resets.append(k)
                k += 1
            assert k == n, f"env{e} call{ci}: {n} device decisions, oracle {k}"
            assert float(times[e, n]) == elapsed
            assert sorted(kk for ee, kk in b["resets"] if ee == e) == resets
            total_resets += len(resets)
        assert reset_count == int(col.reset_count[e])
        parity.compare_obs(ob, obs_dict(v, e), f"env{e} final")
    assert total_resets >= B, total_resets
    assert total_resets == col.total_resets
    assert col.refills > 0 and col.growths > 0, (col.launches, col.refills, col.growths)


def _batch_equal(want, got, what):
    for name in want.__dataclass_fields__:
        a, b = getattr(want, name), getattr(got, name)
        if isinstance(a, torch.Tensor):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), f"{what}: {name}"
        else:
            assert a == b, f"{what}: {name}"


@pytest.mark.gpu
@pytest.mark.parametrize("flags,unit,waves", [(0, "dr_lds50", 4), (_abi.SSIM_CFG_FORCE_HBM, "dr_hbm50", 1)],
                         ids=["dr_lds50", "dr_hbm50"])
def test_timed_collector_matches_lockstep_gpu(gpu_device, dataset, flags, unit, waves):
    """DeviceAsyncRolloutCollector against the lockstep AsyncRolloutCollector on the shipped 50-executor units, 4 rows,
    3 calls of 4e4 ms with StochasticTimeLimit draws of mean 3e4 ms: lengths, elapsed times and rewards bit for bit,
    every observation bit for bit, the same actions, log-probs within float rounding, the same reset steps, reset
    counts and row statistics."""
    import ctypes as ct

    from spark_sched_sim import native
    from spark_sched_sim.engine import DeviceEngine
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers import AsyncRolloutCollector, DeviceAsyncRolloutCollector

    c = SHIPPED
    torch.manual_seed(3)
    pol = DecimaScheduler(c["cfg"]["num_executors"]).to(gpu_device)
    out = []
    for cls in (AsyncRolloutCollector, DeviceAsyncRolloutCollector):
        eng = DeviceEngine(c["cfg"], c["B"], dataset, device=gpu_device, config_flags=flags)
        assert native.lib().ssim_debug_kernel_name(eng.handle, _abi.SSIM_DEBUG_DECIMA).decode() == unit
        cap, wv = ct.c_int32(), ct.c_int32()
        native.check(native.lib().ssim_debug_decima_plan(eng.handle, ct.byref(cap), ct.byref(wv)), "plan")
        assert wv.value == waves
        col = cls(eng, pol, c["duration"], c["bases"], c["step"], mean_time_limit=c["mean"], seed=77, row_offset=2)
        calls = [_call(col.collect()) for _ in range(c["calls"])]
        assert not (eng.views["counts"][:, _abi.OC_ERR].cpu().numpy() & _abi.SSIM_ERR_STICKY).any()
        out.append((calls, col.reset_count.copy(), col.row_stats().cpu(), col))
    (lock, count1, stats1, _), (dev, count2, stats2, col) = out
    for ci, (a, b) in enumerate(zip(lock, dev)):
        what = f"call {ci}"
        assert torch.equal(a["lengths"], b["lengths"]), (what, a["lengths"], b["lengths"])
        assert int(a["lengths"].min()) >= 40, (what, a["lengths"])
        assert torch.equal(a["times"], b["times"]), what
        assert torch.equal(a["rewards"], b["rewards"]), what
        _batch_equal(a["obs"], b["obs"], f"{what}: device vs lockstep observations")
        for k in ("stage_idx", "job_idx", "exec_idx"):
            assert torch.equal(a["acts"][k].long(), b["acts"][k].long()), (what, k)
        assert torch.allclose(a["acts"]["lgprob"], b["acts"]["lgprob"], rtol=1e-5, atol=1e-5), what
        assert a["resets"] == b["resets"], (what, a["resets"], b["resets"])
    assert (count1 == count2).all() and (count2 > 1).all(), (count1, count2)  # every row reset in place
    assert torch.equal(torch.isnan(stats1), torch.isnan(stats2)), (stats1, stats2)
    assert torch.equal(torch.nan_to_num(stats1), torch.nan_to_num(stats2)), (stats1, stats2)
    assert col.launches >= c["calls"]


@pytest.mark.gpu
def test_timed_rollout_argument_validation_gpu(gpu_device, dataset, env_cfg):
    """A missing arena, cap_resets = 0 and SSIM_ROLLOUT_PREEMPT / SSIM_ROLLOUT_AUTORESET with the timed mode are
    refused with SSIM_E_ARG (-1) before anything runs: the envs' observation counts stay as they were."""
    from spark_sched_sim import native
    from spark_sched_sim.engine import DeviceEngine
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers import DeviceAsyncRolloutCollector

    c = SMALL
    eng = DeviceEngine(dict(env_cfg, **c["cfg"]), c["B"], dataset, device=gpu_device)
    torch.manual_seed(3)
    pol = DecimaScheduler(4).to(gpu_device)
    col = DeviceAsyncRolloutCollector(eng, pol, c["duration"], c["bases"], c["step"], mean_time_limit=c["mean"], seed=5)
    col._reset(np.arange(c["B"]))
    col._fill_schedule()
    params = pol.packed_params(eng.device)
    before = eng.views["counts"].clone()
    zero = col._timed()
    zero.cap_resets = 0
    for kw in (dict(samples=None, timed=col._timed()),
               dict(samples=col.arena, timed=zero),
               dict(samples=col.arena, timed=col._timed(), flags=_abi.SSIM_ROLLOUT_PREEMPT, total_decisions=64),
               dict(samples=col.arena, timed=col._timed(), flags=_abi.SSIM_ROLLOUT_PREEMPT),
               dict(samples=col.arena, timed=col._timed(), flags=_abi.SSIM_ROLLOUT_AUTORESET),
               dict(samples=col.arena, timed=col._timed(), total_decisions=64)):
        with pytest.raises(native.NativeError, match=r"ssim_decima_rollout_timed failed \(-1\)"):
            eng.decima_rollout_timed(params, 5, 1, 100, **kw)
        torch.cuda.synchronize()
        assert torch.equal(eng.views["counts"], before), kw
    assert int(col.arena.cursor.abs().sum()) == 0 and int(col.sched.abs().sum()) == 0


@pytest.mark.gpu
def test_ppo_timed_rollouts_gpu(gpu_device, dataset):
    """PPO on a device engine with rollout_duration: the persistent collector, unless lockstep_rollouts keeps the
    per-decision one; two iterations train with finite losses and reset rows in place."""
    from spark_sched_sim.trainers import PPO, AsyncRolloutCollector, DeviceAsyncRolloutCollector
    from test_trainers import SMALL_ENV, TRAIN

    env = dict(SMALL_ENV, mean_time_limit=4e5)
    lock = PPO({"embed_dim": 16}, env, dict(TRAIN, rollout_duration=1.5e5, lockstep_rollouts=True), dataset=dataset,
               device=gpu_device)
    assert type(lock.collector) is AsyncRolloutCollector
    ppo = PPO({"embed_dim": 16}, env, dict(TRAIN, rollout_duration=1.5e5), dataset=dataset, device=gpu_device)
    assert isinstance(ppo.collector, DeviceAsyncRolloutCollector)
    hist = ppo.train(2, log=None)
    assert len(hist) == 2 and all(np.isfinite(h["policy loss"]) for h in hist)
    assert int(ppo.collector.reset_count.sum()) > ppo.rows
