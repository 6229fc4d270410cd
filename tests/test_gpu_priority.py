"""Shortest-job-first schedulers on the device (`-m gpu`): k_policy's SJF / SJF-CP and the fused k_rollout_prio kernels of
both residencies against the oracle driven by the host scheduler (cases_priority.py, the cases of
test_priority_schedulers.py), the budget path by trace parity, evaluate_policy, and the argument checks."""

import pytest

import cases
import cases_priority as P
from spark_sched_sim import _abi

pytestmark = pytest.mark.gpu


def _factory(gpu_device, config_flags=0):
    from spark_sched_sim.engine import DeviceEngine

    return lambda cfg, B, ds, trace_cap: DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap,
                                                     config_flags=config_flags)


@pytest.fixture
def make(gpu_device):
    return _factory(gpu_device)


@pytest.mark.parametrize("is_overloaded", [False, True], ids=["default", "overloaded"])
@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_policy_lockstep(make, dataset, env_cfg, name, is_overloaded):
    seeds = P.OVERLOADED_SEEDS[:2] if is_overloaded else P.DEFAULT_SEEDS
    P.case_policy_lockstep(make, dataset, env_cfg, name, is_overloaded, seeds)


@pytest.mark.parametrize("is_overloaded", [False, True], ids=["default", "overloaded"])
@pytest.mark.parametrize("config_flags", [0, _abi.SSIM_CFG_FORCE_HBM], ids=["lds", "hbm"])
@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_fused_rollout(gpu_device, dataset, env_cfg, name, config_flags, is_overloaded):
    from spark_sched_sim import native

    seeds = P.OVERLOADED_SEEDS if is_overloaded else P.DEFAULT_SEEDS
    eng = P.case_fused_rollout(_factory(gpu_device, config_flags), dataset, env_cfg, name, is_overloaded, seeds)
    assert bool(eng.layout.lds_resident) == (config_flags == 0)
    unit = native.lib().ssim_debug_kernel_name(eng.handle, _abi.SSIM_DEBUG_PRIO).decode()
    assert unit == ("prio_lds" if config_flags == 0 else "prio_hbm")


@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_rollout_budget_replay(make, dataset, env_cfg, name):
    cases.case_rollout_replay(make, dataset, env_cfg, P.KINDS[name], B=64, K=400, stride=8, budget=150)


@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_evaluate_policy(gpu_device, dataset, env_cfg, name):
    out = P.case_evaluate(name, env_cfg, dataset, P.DEFAULT_SEEDS, device=gpu_device)
    assert (out["completed_jobs"] == env_cfg["job_arrival_cap"]).all()


@pytest.mark.parametrize("config_flags", [0, _abi.SSIM_CFG_FORCE_HBM], ids=["lds", "hbm"])
@pytest.mark.parametrize("name", ["sjf", "sjf-cp"])
def test_wide_jobs(gpu_device, env_cfg, name, config_flags):
    P.case_wide_jobs(_factory(gpu_device, config_flags), env_cfg, name)


def test_critical_path_stage_limit(make, env_cfg):
    """More than 64 stages per job: SJF-CP is refused with a message by ssim_policy and the rollouts, SJF runs."""
    import numpy as np

    from spark_sched_sim import native

    cfg, seeds = P.wide_cfg(env_cfg), [5, 6]
    eng = make(cfg, 2, P.datasets("wide70"), 0)
    assert eng.cfg.max_stages == 70
    eng.reset(seeds=seeds)
    L, a = native.lib(), eng.actions
    before = eng.snapshot_obs()
    assert L.ssim_policy(eng.handle, _abi.SSIM_POLICY_SJF_CP, 0, 0, a[0].data_ptr(), a[1].data_ptr(),
                         eng._stream()) == -1  # SSIM_E_ARG
    assert b"at most 64 stages" in L.ssim_last_error()
    assert L.ssim_rollout(eng.handle, _abi.SSIM_POLICY_SJF_CP, 0, 4, None, eng._stream()) == -1
    assert b"at most 64 stages" in L.ssim_last_error()
    assert L.ssim_rollout_budget(eng.handle, _abi.SSIM_POLICY_SJF_CP, 0, 4, 8, 0, None, None, eng._stream()) == -1
    assert (eng.snapshot_obs() == before).all()
    si, ne = eng.policy(_abi.SSIM_POLICY_SJF)
    got = np.stack([eng.to_numpy(si), eng.to_numpy(ne)], axis=1)
    ref = [P.oracle_episode(cfg, "sjf", s, 1, ds_key="wide70").actions[0] for s in seeds]
    assert got.tolist() == np.array(ref).tolist()


def test_unknown_kind_is_refused(make, dataset, env_cfg):
    from spark_sched_sim import native

    eng = make(env_cfg, 2, dataset, 0)
    eng.reset(seeds=[1, 2])
    L, a = native.lib(), eng.actions
    before = eng.snapshot_obs()
    assert L.ssim_policy(eng.handle, 6, 0, 0, a[0].data_ptr(), a[1].data_ptr(), eng._stream()) == -1  # SSIM_E_ARG
    assert b"unknown policy 6" in L.ssim_last_error()
    assert L.ssim_rollout(eng.handle, 6, 0, 4, None, eng._stream()) == -1
    assert b"unknown policy 6" in L.ssim_last_error()
    assert (eng.snapshot_obs() == before).all()
