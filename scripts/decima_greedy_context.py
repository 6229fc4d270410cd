#!/usr/bin/env python
"""Context numbers for the greedy persistent Decima rollout against the sampled one: decisions per second on
BASELINE configs[2]'s env (50 executors / 200 jobs) at `--envs` envs on one GPU (units drg_hbm50 and dr_hbm50).

Per mode, from the same resets: one warm-up launch, then `--launches` timed launches of `--steps` decisions per env
(no auto-reset: SSIM_ROLLOUT_GREEDY does not combine with it; the episodes are thousands of decisions long, so no env
ends within the run), host clock around a device synchronise, decisions counted from the envs' accumulators. One JSON
line per mode with the median rate, its range and the nodes per decision of the run's observations (the two modes
follow different trajectories, so the rates compare workloads as much as kernels). Not a benchmark of record (that is
bench.py). Needs the GPU.

    python scripts/decima_greedy_context.py [--envs 4096] [--steps 64] [--launches 10]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "gym-sparksched_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ENV_CFG = {"num_executors": 50, "job_arrival_cap": 200, "job_arrival_rate": 4.0e-5, "moving_delay": 2000.0,
           "warmup_delay": 1000.0}  # bench.py's decima workload (BASELINE configs[2])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--peak", type=float, default=1.0,
                    help="scale of the score MLPs' last layers: a large value (e.g. 1000) makes the sampled policy "
                         "nearly deterministic, so both modes follow nearly the same trajectories")
    args = ap.parse_args()

    import numpy as np
    import torch

    from spark_sched_sim import _abi, native
    from spark_sched_sim.data_samplers.synthetic_tpch import generate
    from spark_sched_sim.engine import DeviceEngine
    from spark_sched_sim.schedulers.decima import DecimaScheduler

    if not torch.cuda.is_available():
        raise SystemExit("decima_greedy_context.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    ds = generate(0)
    B, K = args.envs, args.steps
    seeds = np.arange(args.seed, args.seed + B, dtype=np.uint64)
    torch.manual_seed(0)
    pol = DecimaScheduler(ENV_CFG["num_executors"])
    with torch.no_grad():
        for net in (pol.stage_policy_network, pol.exec_policy_network):
            net.mlp_score[-1].weight.mul_(args.peak)
    params = pol.to(dev).packed_params(dev)
    for mode, flags, variant in (("sampled", 0, _abi.SSIM_DEBUG_DECIMA),
                                 ("greedy", _abi.SSIM_ROLLOUT_GREEDY, _abi.SSIM_DEBUG_DECIMA_GREEDY)):
        eng = DeviceEngine(ENV_CFG, B, ds, device=dev)
        unit = native.lib().ssim_debug_kernel_name(eng.handle, variant).decode()
        eng.reset_sampled(_abi.SSIM_RESET_SEED, seeds=seeds)
        eng.decima_rollout(params, 1234, 0, K, flags=flags)  # warm-up
        torch.cuda.synchronize(dev)
        rates = []
        n0 = int(eng.views["acc"][:, _abi.ACC_NODES].sum().item())
        dd0 = int(eng.views["acc"][:, _abi.ACC_DECISIONS].sum().item())
        for _ in range(args.launches):
            d0 = int(eng.views["acc"][:, _abi.ACC_DECISIONS].sum().item())
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng.decima_rollout(params, 1234, 0, K, flags=flags)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            d1 = int(eng.views["acc"][:, _abi.ACC_DECISIONS].sum().item())
            rates.append((d1 - d0) / (t1 - t0))
        c = eng.views["counts"].cpu().numpy()
        n1 = int(eng.views["acc"][:, _abi.ACC_NODES].sum().item())
        dd1 = int(eng.views["acc"][:, _abi.ACC_DECISIONS].sum().item())
        print(json.dumps({"mode": mode, "unit": unit, "envs": B, "peak": args.peak,
                          "nodes_per_decision": (n1 - n0) / max(dd1 - dd0, 1), "steps_per_launch": K,
                          "launches": args.launches,
                          "decisions_per_s_median": float(np.median(rates)), "decisions_per_s_min": float(min(rates)),
                          "decisions_per_s_max": float(max(rates)),
                          "terminated_envs": int((c[:, _abi.OC_TERMINATED] != 0).sum()),
                          "error_envs": int((c[:, _abi.OC_ERR] != 0).sum())}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
