"""Batched Decima GNN policy (spark_sched_sim/schedulers/decima.py) vs the per-observation CPU fp32
restatement (oracle/decima_gnn.py), on the test-only host build of the engine (CPU suite) and on the
device engine (`-m gpu`, the policy on the GPU)."""

import pytest

import cases


@pytest.fixture(scope="module")
def make_host():
    from hostsim.driver import HostEngine

    def _make(cfg, B, ds, trace_cap):
        return HostEngine(cfg, B, ds, trace_cap=trace_cap)

    return _make


@pytest.mark.parametrize("cfg_over,B,seed0,every", cases.POLICY_CONFIGS)
def test_decima_policy_host(make_host, dataset, env_cfg, cfg_over, B, seed0, every):
    cases.case_decima_policy(make_host, dataset, env_cfg, cfg_over, min(B, 2), seed0, every * 2, max_steps=250)


def test_decima_schedule_host(make_host, dataset, env_cfg):
    cases.case_decima_schedule_runs(make_host, dataset, env_cfg, B=6, steps=20)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_over,B,seed0,every", cases.POLICY_CONFIGS)
def test_decima_policy_gpu(gpu_device, dataset, env_cfg, cfg_over, B, seed0, every):
    from spark_sched_sim.engine import DeviceEngine

    def make(cfg, B, ds, trace_cap):
        return DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap)

    cases.case_decima_policy(make, dataset, env_cfg, cfg_over, B, seed0, every, device=gpu_device)


@pytest.mark.gpu
def test_decima_schedule_gpu(gpu_device, dataset, env_cfg):
    from spark_sched_sim.engine import DeviceEngine

    def make(cfg, B, ds, trace_cap):
        return DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap)

    cases.case_decima_schedule_runs(make, dataset, env_cfg, B=64, steps=50, device=gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_over,B,seed0,every", cases.FUSED_CONFIGS)
def test_decima_fused_kernel_gpu(gpu_device, dataset, env_cfg, cfg_over, B, seed0, every):
    from spark_sched_sim.engine import DeviceEngine

    def make(cfg, B, ds, trace_cap):
        return DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap)

    expect = cases.FUSED_EXPECT[[c[0] for c in cases.FUSED_CONFIGS].index(cfg_over)]
    seen = cases.case_decima_fused(make, dataset, env_cfg, cfg_over, 32, seed0, device=gpu_device, expect=expect)
    print(f"fused kernel {cfg_over}: decisions checked against the oracle and the paths among them: {seen}")


# ---- the same cases at the "spread" parameter set (cases.spread_params; tests/test_policy_strength.py shows that a 1%
# error in any of the 21 layers moves a compared quantity by at least 4 x its bar there, which the flat set does not)

def test_decima_policy_spread_host(make_host, dataset, env_cfg):
    cases.case_decima_policy(make_host, dataset, env_cfg, dict(), 2, 610, 14, max_steps=250, params=cases.spread_params)


@pytest.mark.gpu
def test_decima_policy_spread_gpu(gpu_device, dataset, env_cfg):
    """The batched module on the device (HipMlp3's forward) at N=10 with the spread parameters."""
    from spark_sched_sim.engine import DeviceEngine

    def make(cfg, B, ds, trace_cap):
        return DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap)

    cases.case_decima_policy(make, dataset, env_cfg, dict(), 4, 610, 7, device=gpu_device, params=cases.spread_params)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_over,B,seed0", [(dict(), 4, 610), (cases.DENSE50_OVER, 2, 620)], ids=["n10", "dense50"])
def test_decima_fused_kernel_spread_gpu(gpu_device, dataset, env_cfg, cfg_over, B, seed0):
    """ssim_decima_policy at the spread parameters, 6 launches: stage scores, exec scores and lgprob of every env
    against the float64 oracle at the standing bars (1e-5 + 1e-4 |score|, 1e-4 + 1e-4 |lgprob|)."""
    import torch

    from spark_sched_sim.engine import DeviceEngine

    def make(cfg, B, ds, trace_cap):
        return DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap)

    seen = cases.case_decima_fused(make, dataset, env_cfg, cfg_over, B, seed0, iters=6, device=gpu_device,
                                   params=cases.spread_params, oracle_dtype=torch.float64, oracle_every=1,
                                   aux_calls=False)
    assert seen["oracle"] >= B * 6 // 2, seen
    print(f"fused kernel, spread parameters {cfg_over}: {seen}")
