"""Weighted-fair schedulers on the device (`-m gpu`): the arithmetic through ssim_debug_wfair bit for bit against numpy,
k_policy's weighted-fair kinds and the fused k_rollout_wfair kernels of both residencies against the oracle driven by
the host scheduler (cases_wfair.py, the cases of test_weighted_fair.py), the budget path by trace parity,
evaluate_policy, and the argument checks."""

import numpy as np
import pytest

import cases
import cases_wfair as C
from spark_sched_sim import _abi

pytestmark = pytest.mark.gpu


def _factory(gpu_device, config_flags=0):
    from spark_sched_sim.engine import DeviceEngine

    return lambda cfg, B, ds, trace_cap: DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap,
                                                     config_flags=config_flags)


@pytest.fixture
def make(gpu_device):
    return _factory(gpu_device)


def test_arithmetic_kat(gpu_device):
    import torch

    from spark_sched_sim import native

    L = native.lib()
    stream = torch.cuda.current_stream(gpu_device).cuda_stream

    def run(W, alpha2, n_exec):
        n = len(W)
        w = torch.as_tensor(np.array(W, dtype=np.float64), device=gpu_device)  # (a writable copy)
        p = torch.zeros(n, dtype=torch.float64, device=gpu_device)
        total = torch.zeros(1, dtype=torch.float64, device=gpu_device)
        cap = torch.zeros(n, dtype=torch.int32, device=gpu_device)
        native.check(L.ssim_debug_wfair(w.data_ptr(), n, alpha2, n_exec, p.data_ptr(), total.data_ptr(),
                                        cap.data_ptr(), stream), "ssim_debug_wfair")
        return p.cpu().numpy(), total.cpu().numpy()[0], cap.cpu().numpy()

    C.case_kat(run)
    assert L.ssim_debug_wfair(None, 4, 0, 10, None, None, None, stream) == -1  # SSIM_E_ARG
    w = torch.zeros(8, dtype=torch.float64, device=gpu_device)
    c = torch.zeros(8, dtype=torch.int32, device=gpu_device)
    for n, alpha2, n_exec in ((0, 0, 10), (4, 5, 10), (4, -5, 10), (4, 0, 0), (4097, 0, 10)):
        assert L.ssim_debug_wfair(w.data_ptr(), n, alpha2, n_exec, w.data_ptr(), w.data_ptr(), c.data_ptr(),
                                  stream) == -1
        assert b"ssim_debug_wfair" in L.ssim_last_error()


def test_alpha_zero_rollout_is_fair(make, dataset, env_cfg):
    logs = []
    for kind in (0x104, _abi.SSIM_POLICY_FAIR):
        eng = make(env_cfg, 2, dataset, 0)
        eng.reset(seeds=list(C.DEFAULT_SEEDS))
        log = eng.alloc_action_log(1200)
        log.fill_(-7)
        eng.rollout(kind, 0, 1200, log)
        assert (eng.host_views()["counts"][:, _abi.OC_TERMINATED] != 0).all()
        logs.append(np.asarray(eng.to_numpy(log)).copy())
    assert (logs[0] == logs[1]).all()
    C.case_fused_rollout(make, dataset, env_cfg, 0, False, C.DEFAULT_SEEDS)


@pytest.mark.parametrize("alpha2", [-2, 1])
def test_policy_lockstep(make, dataset, env_cfg, alpha2):
    C.case_policy_lockstep(make, dataset, env_cfg, alpha2, False, C.DEFAULT_SEEDS)


@pytest.mark.parametrize("config_flags", [0, _abi.SSIM_CFG_FORCE_HBM], ids=["lds", "hbm"])
def test_fused_rollout(gpu_device, dataset, env_cfg, config_flags):
    """All eight exponents on the default env, on the unit of each residency."""
    from spark_sched_sim import native

    for alpha2 in C.NONZERO:
        eng = C.case_fused_rollout(_factory(gpu_device, config_flags), dataset, env_cfg, alpha2, False,
                                   C.DEFAULT_SEEDS)
        assert bool(eng.layout.lds_resident) == (config_flags == 0)
        name = native.lib().ssim_debug_kernel_name
        assert name(eng.handle, _abi.SSIM_DEBUG_WFAIR).decode() == ("wfair_lds" if config_flags == 0 else "wfair_hbm")
        # (the SJF kinds' unit of the same handle is unchanged)
        assert name(eng.handle, _abi.SSIM_DEBUG_PRIO).decode() == ("prio_lds" if config_flags == 0 else "prio_hbm")


@pytest.mark.parametrize("alpha2", [-2, 2])
def test_busy_env(make, dataset, env_cfg, alpha2):
    """More than 64 active jobs: the multi-block sum, by `policy(kind)` in lockstep and by a fused rollout."""
    C.case_policy_lockstep(make, dataset, env_cfg, alpha2, True, C.BUSY_SEEDS)
    C.case_fused_rollout(make, dataset, env_cfg, alpha2, True, C.BUSY_SEEDS)


@pytest.mark.parametrize("config_flags", [0, _abi.SSIM_CFG_FORCE_HBM], ids=["lds", "hbm"])
def test_wide_jobs(gpu_device, env_cfg, config_flags):
    C.case_wide_jobs(_factory(gpu_device, config_flags), env_cfg, -2)


def test_rollout_budget_replay(make, dataset, env_cfg):
    cases.case_rollout_replay(make, dataset, env_cfg, C.kind_of(-2), B=64, K=400, stride=8, budget=150)


def test_evaluate_policy(gpu_device, dataset, env_cfg):
    out = C.case_evaluate(-2, env_cfg, dataset, C.DEFAULT_SEEDS, device=gpu_device)
    assert (out["completed_jobs"] == env_cfg["job_arrival_cap"]).all()


def test_kind_past_the_family_is_refused(make, dataset, env_cfg):
    from spark_sched_sim import native

    eng = make(env_cfg, 2, dataset, 0)
    eng.reset(seeds=[1, 2])
    L, a = native.lib(), eng.actions
    before = eng.snapshot_obs()
    for kind in (0x109, 0xFF):
        assert L.ssim_policy(eng.handle, kind, 0, 0, a[0].data_ptr(), a[1].data_ptr(), eng._stream()) == -1  # E_ARG
        assert f"unknown policy {kind}".encode() in L.ssim_last_error()
        assert L.ssim_rollout(eng.handle, kind, 0, 4, None, eng._stream()) == -1
        assert f"unknown policy {kind}".encode() in L.ssim_last_error()
        assert L.ssim_rollout_budget(eng.handle, kind, 0, 4, 8, 0, None, None, eng._stream()) == -1
    assert L.ssim_policy(eng.handle, 0x109, 0, 0, a[0].data_ptr(), a[1].data_ptr(), eng._stream()) == -1
    assert b"0x100..0x108" in L.ssim_last_error()
    assert (eng.snapshot_obs() == before).all()
