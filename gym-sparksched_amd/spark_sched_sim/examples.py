"""Episode runner and CLI of the reference's `examples.py` on the MI355X engine.

`run_episode(env_cfg, scheduler, seed)` is `examples.py:84-102`: one `SparkSchedSimEnv` episode (each step is
a gfx950 kernel launch through the C ABI) driven by a host scheduler's `schedule(obs)`, returning the
average job duration in seconds (`metrics.avg_job_duration(env) * 1e-3`).

    python -m spark_sched_sim.examples --sched fair      # examples.py --sched fair (BASELINE configs[0])
    python -m spark_sched_sim.examples --sched sjf-cp    # shortest job first, critical-path stage choice
    python -m spark_sched_sim.examples --sched wfair --alpha -1   # weighted fair: executors in proportion to work^alpha
    python -m spark_sched_sim.examples --sched decima --model decima.pt   # a DecimaScheduler.save checkpoint, greedy
                                                                          # (--sample: draw the actions instead)
"""

from __future__ import annotations

from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pprint import pprint

from . import metrics
from .env import SparkSchedSimEnv
from .schedulers import POLICY_KINDS, host_scheduler

ENV_CFG = {  # examples.py:15-23, without the pygame renderer
    "num_executors": 10,
    "job_arrival_cap": 50,
    "job_arrival_rate": 4.0e-5,
    "moving_delay": 2000.0,
    "warmup_delay": 1000.0,
    "data_sampler_cls": "TPCHDataSampler",
}


def run_episode(env_cfg: dict, scheduler, seed: int = 1234, **env_kwargs) -> float:
    env = SparkSchedSimEnv(env_cfg, **env_kwargs)
    if getattr(scheduler, "env_wrapper_cls", None):
        env = scheduler.env_wrapper_cls(env)
    obs, _ = env.reset(seed=seed, options=None)
    terminated = truncated = False
    while not (terminated or truncated):
        action, _ = scheduler.schedule(obs)
        obs, _, terminated, truncated, _ = env.step(action)
    avg = metrics.avg_job_duration(env) * 1e-3
    env.close()
    return avg


class DecimaHostScheduler:
    """A trained DecimaScheduler as a host scheduler of the one-env facade (the reference's `--sched decima`): the env
    is wrapped in DecimaEnvWrapper and every decision is `DecimaScheduler.schedule` on its observation, greedy
    (arg-max) unless `sample`."""

    name = "Decima"

    def __init__(self, model, sample: bool = False, seed: int = 42):
        import torch

        from .decima import DecimaEnvWrapper

        self.env_wrapper_cls = DecimaEnvWrapper
        self.model = model
        self.greedy = not sample
        self.generator = torch.Generator(device=model.device).manual_seed(seed)

    def schedule(self, obs):
        return self.model.schedule_obs(obs, greedy=self.greedy, generator=self.generator)


def main(argv=None) -> None:
    parser = ArgumentParser(description=__doc__, formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument("--sched", choices=list(POLICY_KINDS) + ["wfair", "decima"], required=True)
    parser.add_argument("--alpha", type=float, default=None,
                        help="--sched wfair: the work exponent, a half-integer in [-2, 2] (default -1)")
    parser.add_argument("--seed", type=int, default=1234)
    parser.add_argument("--model", default=None, help="--sched decima: a DecimaScheduler.save checkpoint")
    parser.add_argument("--sample", action="store_true", help="--sched decima: draw the actions (default: arg-max)")
    args = parser.parse_args(argv)
    if args.sched == "decima":
        if not args.model:
            parser.exit(2, "--sched decima needs --model PATH: a checkpoint written by DecimaScheduler.save (see "
                           "scripts/train_and_evaluate.py)\n")
        from .schedulers.decima import DecimaScheduler

        model = DecimaScheduler.load(args.model)
        if model.num_executors != ENV_CFG["num_executors"]:
            parser.exit(2, f"{args.model}: trained for {model.num_executors} executors, this example's env has "
                           f"{ENV_CFG['num_executors']}\n")
        scheduler = DecimaHostScheduler(model, sample=args.sample, seed=42)
    else:
        try:
            scheduler = host_scheduler(args.sched, ENV_CFG["num_executors"], seed=42, alpha=args.alpha)
        except ValueError as e:  # (--alpha off the grid, or given with another scheduler)
            parser.exit(2, f"{e}\n")
    print(f"Example: {scheduler.name} Scheduler")
    print("Env settings:")
    pprint(ENV_CFG)
    print("Running episode...")
    avg = run_episode(ENV_CFG, scheduler, seed=args.seed)
    print(f"Done! Average job duration: {avg:.1f}s", flush=True)


if __name__ == "__main__":
    main()
