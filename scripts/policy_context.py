#!/usr/bin/env python
"""Context numbers for the device schedulers on the BASELINE configs[1] env (50 TPC-H jobs / 10 executors), 1,024
envs on one GPU: the decision rate of the fused rollout and the average job duration each scheduler reaches.

Per kind (fair, fifo, random, sjf, sjf-cp, wfair), one JSON line with
  decisions_per_s   steady state as bench.py measures it: envs spread over their episodes by a pre-roll, one warm-up
                    launch, then `--launches` timed launches of a shared budget of envs x `--steps` decisions
                    (auto-reset, preemptible), host clock around a device synchronise; and the spread of the launches;
  avg_job_duration  mean over the envs (seeds `--seed` + i) of the episode's average job duration in seconds, every
                    env run from reset to termination (evaluate.evaluate_policy);
  unit              the translation unit the rollout ran: fair / FIFO / random run the unit specialised for the shape,
                    SJF / SJF-CP / weighted fair the run-time-shape unit of the residency, so the rates are context,
                    not a comparison of the rules.
The `wfair` line has the rate at one exponent (`--alpha`, default -1), the average job duration at all nine exponents
(`avg_job_duration_s_by_alpha`, evaluate.tune_weighted_fair on the same seeds) and the tuned one (`tuned_alpha`, whose
duration is the line's `avg_job_duration_s`).
Not a benchmark of record (that is bench.py). Needs the GPU; fails without one.

    python scripts/policy_context.py [--envs 1024] [--steps 300] [--launches 10]
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

ENV_CFG = {"num_executors": 10, "job_arrival_cap": 50, "job_arrival_rate": 4.0e-5, "moving_delay": 2000.0,
           "warmup_delay": 1000.0}  # bench.py ENV_CFG (BASELINE configs[1])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=300, help="decisions per env of one timed launch's budget")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--preroll", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kinds", default="fair,fifo,random,sjf,sjf-cp,wfair")
    ap.add_argument("--alpha", type=float, default=-1.0, help="wfair: the exponent of the rate measurement")
    args = ap.parse_args()

    import numpy as np
    import torch

    from spark_sched_sim import _abi, native
    from spark_sched_sim.data_samplers.synthetic_tpch import generate
    from spark_sched_sim.engine import DeviceEngine
    from spark_sched_sim.evaluate import evaluate_policy, tune_weighted_fair

    if not torch.cuda.is_available():
        raise SystemExit("policy_context.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    ds = generate(0)
    B, K = args.envs, args.steps
    seeds = np.arange(args.seed, args.seed + B, dtype=np.uint64)
    for name in args.kinds.split(","):
        kind = _abi.wfair_kind(args.alpha) if name == "wfair" else _abi.POLICY_KINDS[name]
        prio = kind in (_abi.SSIM_POLICY_SJF, _abi.SSIM_POLICY_SJF_CP)
        eng = DeviceEngine(ENV_CFG, B, ds, device=dev)
        unit = native.lib().ssim_debug_kernel_name(
            eng.handle, _abi.SSIM_DEBUG_WFAIR if name == "wfair" else _abi.SSIM_DEBUG_PRIO if prio
            else _abi.SSIM_DEBUG_ENGINE).decode()
        eng.reset_sampled(_abi.SSIM_RESET_SEED, seeds=seeds)
        pre = np.random.default_rng([args.seed, 7]).integers(0, max(args.preroll, 1), B).astype(np.int32)
        eng.rollout_steps(kind, 4321, pre, int(pre.max()) + 1,
                          flags=_abi.SSIM_ROLLOUT_AUTORESET | _abi.SSIM_ROLLOUT_WARMUP)
        timed = _abi.SSIM_ROLLOUT_AUTORESET | _abi.SSIM_ROLLOUT_PREEMPT
        eng.rollout_budget(kind, 1234, 8 * K, B * K, flags=timed | _abi.SSIM_ROLLOUT_WARMUP)
        torch.cuda.synchronize(dev)
        rates = []
        for _ in range(args.launches):
            d0 = int(eng.views["acc"][:, _abi.ACC_DECISIONS].sum().item())
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng.rollout_budget(kind, 1234, 8 * K, B * K, flags=timed)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            rates.append((int(eng.views["acc"][:, _abi.ACC_DECISIONS].sum().item()) - d0) / (t1 - t0))
        errs = int(np.count_nonzero(np.asarray(eng.host_views()["counts"])[:, _abi.OC_ERR] & _abi.SSIM_ERR_STICKY))
        eng.close()
        extra = {}
        if name == "wfair":
            tuned = tune_weighted_fair(ENV_CFG, [int(s) for s in seeds], device=dev, dataset=ds)
            ev = {"avg_job_duration": tuned["per_seed"][tuned["alpha"]],
                  "decisions": evaluate_policy(ENV_CFG, "wfair", [int(s) for s in seeds], device=dev, dataset=ds,
                                               alpha=tuned["alpha"])["decisions"]}
            extra = {"rate_alpha": args.alpha, "tuned_alpha": tuned["alpha"],
                     "avg_job_duration_s_by_alpha": {f"{a:g}": m for a, m in tuned["mean_avg_job_duration"].items()}}
        else:
            ev = evaluate_policy(ENV_CFG, name, [int(s) for s in seeds], device=dev, dataset=ds)
        print(json.dumps({"policy": name, **extra, "unit": unit, "envs": B, "decisions_per_launch": B * K,
                          "decisions_per_s": float(np.median(rates)), "decisions_per_s_min": float(min(rates)),
                          "decisions_per_s_max": float(max(rates)), "errors": errs,
                          "avg_job_duration_s": float(np.mean(ev["avg_job_duration"])),
                          "avg_job_duration_s_std": float(np.std(ev["avg_job_duration"])),
                          "episode_decisions_mean": float(np.mean(ev["decisions"])),
                          "build": native.build_id()}), flush=True)


if __name__ == "__main__":
    main()
