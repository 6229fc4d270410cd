#!/usr/bin/env python
"""Clone a device heuristic into a Decima policy, then evaluate: teacher rollouts -> behaviour cloning -> save -> load ->
evaluate, end to end on one GPU. Context for the Decima workflow, NOT a result about Decima: the clone is trained for a
few iterations on the synthetic data set.

  1. behaviour cloning (trainers.imitation.BehaviourCloning) on config/decima_tpch.yaml's env (50 executors, 200 jobs):
     per iteration one teacher collection of `--bc-envs` episodes (ssim_teacher_rollout: the heuristic's decisions as
     Decima samples, one persistent launch) and `--epochs` x `--batches` Adam steps on the negative log-likelihood of
     the teacher's actions, no-op decisions masked out. The teacher is the tuned weighted-fair scheduler (alpha =
     -0.5), or `--teacher` / `--alpha`;
  2. DecimaScheduler.save(path), then DecimaScheduler.load(path);
  3. evaluate.evaluate_policy on the same `--envs` seeds, every episode to termination: the teacher, the clone
     (greedy) and fair;
  4. with `--ppo-iterations K`: K PPO iterations started from the clone (agent_cfg["init_checkpoint"]), evaluated again.

Prints one table (mean and median over the envs of the episode's average job duration, in seconds) and one JSON line.

    python scripts/imitate_and_evaluate.py [--teacher wfair --alpha -0.5] [--iterations 8] [--envs 1024]
                                           [--ppo-iterations 0] [--model clone.pt]
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
    ap.add_argument("--teacher", default="wfair", help="fair, fifo, random, sjf, sjf-cp or wfair")
    ap.add_argument("--alpha", type=float, default=None, help="wfair: the exponent (default -0.5, the tuned one)")
    ap.add_argument("--iterations", type=int, default=8, help="behaviour-cloning iterations (one collection each)")
    ap.add_argument("--bc-envs", type=int, default=16, help="teacher episodes per collection")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--envs", type=int, default=1024, help="evaluation episodes (seeds --seed .. --seed + envs - 1)")
    ap.add_argument("--seed", type=int, default=10000)
    ap.add_argument("--ppo-iterations", type=int, default=0, help="PPO iterations started from the clone")
    ap.add_argument("--model", default=None, help="checkpoint path of the clone (default: a temporary file)")
    ap.add_argument("--steps-per-launch", type=int, default=1024)
    args = ap.parse_args()

    import numpy as np
    import torch

    from spark_sched_sim.env import resolve_dataset
    from spark_sched_sim.evaluate import evaluate_policy
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers import DECIMA_TPCH, PPO
    from spark_sched_sim.trainers.imitation import BehaviourCloning

    if not torch.cuda.is_available():
        raise SystemExit("imitate_and_evaluate.py runs on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = {k: dict(v) for k, v in DECIMA_TPCH.items()}
    dataset = resolve_dataset(cfg["env"])
    alpha = (-0.5 if args.alpha is None else args.alpha) if args.teacher == "wfair" else None
    env_cfg = {k: v for k, v in cfg["env"].items() if k not in ("mean_time_limit", "dataset")}
    train_cfg = {"teacher": args.teacher, "alpha": alpha, "num_envs": args.bc_envs, "seed": 42,
                 "num_iterations": args.iterations, "num_epochs": args.epochs, "num_batches": args.batches,
                 "lr": args.lr, "max_grad_norm": 0.5}
    t0 = time.perf_counter()
    bc = BehaviourCloning(cfg["agent"], env_cfg, train_cfg, dataset=dataset, device=dev)
    hist = bc.train(log=lambda m: print(m, file=sys.stderr))
    torch.cuda.synchronize(dev)
    bc_s = time.perf_counter() - t0

    tmp = None
    path = args.model
    if path is None:
        tmp = tempfile.TemporaryDirectory()
        path = os.path.join(tmp.name, "clone.pt")
    bc.scheduler.save(path)
    clone = DecimaScheduler.load(path, device=dev)
    assert torch.equal(clone.packed_params(dev), bc.scheduler.packed_params(dev))

    seeds = list(range(args.seed, args.seed + args.envs))
    teacher_label = f"teacher: {args.teacher}" + (f" (alpha {alpha:g})" if alpha is not None else "")
    todo = [(teacher_label, args.teacher, dict(alpha=alpha) if alpha is not None else {}),
            ("clone (greedy)", "decima", dict(policy=clone, greedy=True)), ("fair", "fair", {})]
    ppo_s = None
    if args.ppo_iterations > 0:
        cfg["agent"]["init_checkpoint"] = path
        t0 = time.perf_counter()
        ppo = PPO(cfg["agent"], cfg["env"], cfg["trainer"], dataset=dataset, device=dev)
        ppo.train(args.ppo_iterations, log=None)
        torch.cuda.synchronize(dev)
        ppo_s = time.perf_counter() - t0
        todo.append((f"clone + {args.ppo_iterations} PPO (greedy)", "decima", dict(policy=ppo.scheduler, greedy=True)))
    rows = []
    for label, kind, kw in todo:
        t0 = time.perf_counter()
        try:
            out = evaluate_policy(env_cfg, kind, seeds, device=dev, dataset=dataset, max_launches=256,
                                  steps_per_launch=args.steps_per_launch, **kw)
        except RuntimeError as err:  # an env froze or never terminated: reported, not hidden
            rows.append({"scheduler": label, "error": str(err)})
            continue
        torch.cuda.synchronize(dev)
        rows.append({"scheduler": label, "mean_avg_job_duration_s": float(np.mean(out["avg_job_duration"])),
                     "median_avg_job_duration_s": float(np.median(out["avg_job_duration"])),
                     "decisions_per_episode": float(np.mean(out["decisions"])), "launches": out["launches"],
                     "seconds": time.perf_counter() - t0})
    last = hist[-1] if hist else {}
    print(f"{args.iterations} behaviour-cloning iterations ({args.bc_envs} teacher episodes each, "
          f"{sum(h['samples'] for h in hist)} samples, {sum(h['adam_steps'] for h in hist)} Adam steps) in {bc_s:.1f} s"
          + (f"; {args.ppo_iterations} PPO iterations in {ppo_s:.1f} s" if ppo_s is not None else "")
          + f"; {args.envs} evaluation episodes per scheduler (50 executors, 200 jobs), to termination")
    if last:
        print(f"last iteration: nll {last['nll_before']:.4f} -> {last['nll_after']:.4f}, stage agreement "
              f"{last['stage_agreement']:.3f}, exec agreement {last['exec_agreement']:.3f}")
    print(f"{'scheduler':<28}{'mean avg job duration [s]':>28}{'median [s]':>14}{'decisions / episode':>22}"
          f"{'wall [s]':>10}")
    for r in rows:
        if "error" in r:
            print(f"{r['scheduler']:<28}  no result: {r['error']}")
            continue
        print(f"{r['scheduler']:<28}{r['mean_avg_job_duration_s']:>28.1f}{r['median_avg_job_duration_s']:>14.1f}"
              f"{r['decisions_per_episode']:>22.0f}{r['seconds']:>10.2f}")
    print(json.dumps({"teacher": args.teacher, "alpha": alpha, "bc_iterations": args.iterations, "bc_seconds": bc_s,
                      "ppo_iterations": args.ppo_iterations, "ppo_seconds": ppo_s, "envs": args.envs,
                      "history": hist, "rows": rows}))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
