#!/usr/bin/env python
"""Train -> save -> load -> evaluate, end to end on one GPU: a worked example of the checkpoint and evaluation
workflow, NOT a result about Decima (a policy trained for a few iterations on the synthetic data set has learned
next to nothing; the reference trains for 500 iterations on the TPC-H traces).

  1. a few PPO iterations of config/decima_tpch.yaml's setup (trainers.DECIMA_TPCH: 50 executors, 200 jobs, 16 rollout
     rows) with the persistent device collector;
  2. DecimaScheduler.save(path), then DecimaScheduler.load(path) (torch.load(weights_only=True));
  3. evaluate.evaluate_policy on the same `--envs` seeds, every episode run to termination on the device: the loaded
     policy greedy (arg-max actions) and sampled, against the fair and SJF heuristics.

Prints one table (mean and median over the envs of the episode's average job duration, in seconds) and one JSON line.

    python scripts/train_and_evaluate.py [--iterations 3] [--envs 1024] [--model decima.pt] [--init clone.pt]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "gym-sparksched_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iterations", type=int, default=3, help="PPO iterations before the checkpoint")
    ap.add_argument("--envs", type=int, default=1024, help="evaluation episodes (seeds --seed .. --seed + envs - 1)")
    ap.add_argument("--seed", type=int, default=10000)
    ap.add_argument("--model", default=None, help="checkpoint path (default: a temporary file)")
    ap.add_argument("--steps-per-launch", type=int, default=1024)
    ap.add_argument("--init", default=None, metavar="PATH",
                    help="start PPO from this DecimaScheduler.save checkpoint (agent_cfg['init_checkpoint']), e.g. a "
                         "behaviour-cloned policy of scripts/imitate_and_evaluate.py")
    args = ap.parse_args()

    import numpy as np
    import torch

    from spark_sched_sim.env import resolve_dataset
    from spark_sched_sim.evaluate import evaluate_policy
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers import DECIMA_TPCH, PPO

    if not torch.cuda.is_available():
        raise SystemExit("train_and_evaluate.py runs on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = {k: dict(v) for k, v in DECIMA_TPCH.items()}
    dataset = resolve_dataset(cfg["env"])
    if args.init:
        cfg["agent"]["init_checkpoint"] = args.init
    t0 = time.perf_counter()
    ppo = PPO(cfg["agent"], cfg["env"], cfg["trainer"], dataset=dataset, device=dev)
    hist = ppo.train(args.iterations, log=None)
    torch.cuda.synchronize(dev)
    train_s = time.perf_counter() - t0

    tmp = None
    path = args.model
    if path is None:
        tmp = tempfile.TemporaryDirectory()
        path = os.path.join(tmp.name, "decima.pt")
    ppo.scheduler.save(path)
    policy = DecimaScheduler.load(path, device=dev)
    assert torch.equal(policy.packed_params(dev), ppo.scheduler.packed_params(dev))

    env_cfg = {k: v for k, v in cfg["env"].items() if k not in ("mean_time_limit", "dataset")}
    seeds = list(range(args.seed, args.seed + args.envs))
    rows = []
    for label, kind, kw in (("decima (greedy)", "decima", dict(policy=policy, greedy=True)),
                            ("decima (sampled)", "decima", dict(policy=policy, greedy=False, policy_seed=1)),
                            ("fair", "fair", {}), ("sjf", "sjf", {})):
        t0 = time.perf_counter()
        try:
            out = evaluate_policy(env_cfg, kind, seeds, device=dev, dataset=dataset, max_launches=256,
                                  steps_per_launch=args.steps_per_launch, **kw)
        except RuntimeError as err:  # an env froze (e.g. an assert of the reference's simulator fired on this
            rows.append({"scheduler": label, "error": str(err)})  # trajectory): reported, not hidden
            continue
        torch.cuda.synchronize(dev)
        rows.append({"scheduler": label, "mean_avg_job_duration_s": float(np.mean(out["avg_job_duration"])),
                     "median_avg_job_duration_s": float(np.median(out["avg_job_duration"])),
                     "decisions_per_episode": float(np.mean(out["decisions"])), "launches": out["launches"],
                     "seconds": time.perf_counter() - t0})
    print(f"{args.iterations} PPO iterations in {train_s:.1f} s; {args.envs} evaluation episodes per scheduler "
          f"(50 executors, 200 jobs), to termination")
    print(f"{'scheduler':<18}{'mean avg job duration [s]':>28}{'median [s]':>14}{'decisions / episode':>22}"
          f"{'wall [s]':>10}")
    for r in rows:
        if "error" in r:
            print(f"{r['scheduler']:<18}  no result: {r['error']}")
            continue
        print(f"{r['scheduler']:<18}{r['mean_avg_job_duration_s']:>28.1f}{r['median_avg_job_duration_s']:>14.1f}"
              f"{r['decisions_per_episode']:>22.0f}{r['seconds']:>10.2f}")
    print(json.dumps({"iterations": args.iterations, "train_seconds": train_s, "envs": args.envs,
                      "last_iteration": {k: (float(v) if isinstance(v, (int, float)) else str(v))
                                         for k, v in (hist[-1] if hist else {}).items()}, "rows": rows}))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
