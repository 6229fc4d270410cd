"""Scheduler plugins (reference `schedulers/__init__.py`): host heuristics over the facade's obs dicts, the
batched Decima GNN over device observations, and `make_scheduler` by class name. The batched device action
drivers (fair / FIFO / random / SJF / SJF-CP / weighted fair) used inside the rollout kernels are in csrc/policy.h;
`POLICY_KINDS` maps their names to the device policy kinds (weighted fair: `_abi.wfair_kind(alpha)`)."""

__all__ = ["Scheduler", "DecimaScheduler", "RandomScheduler", "RoundRobinScheduler", "make_scheduler",
           "preprocess_obs", "find_stage", "ShortestJobFirstScheduler", "WeightedFairScheduler", "POLICY_KINDS", "host_scheduler"]

# the classes make_scheduler instantiates by name
SCHEDULER_CLASSES = ("DecimaScheduler", "RandomScheduler", "RoundRobinScheduler", "ShortestJobFirstScheduler",
                     "WeightedFairScheduler")

from copy import deepcopy

from .._abi import POLICY_KINDS
from .heuristics import (RandomScheduler, RoundRobinScheduler, Scheduler, ShortestJobFirstScheduler,
                         WeightedFairScheduler, find_stage, preprocess_obs)


def __getattr__(name):  # torch is imported only when the GNN is asked for
    if name == "DecimaScheduler":
        from .decima import DecimaScheduler

        return DecimaScheduler
    raise AttributeError(name)


def make_scheduler(agent_cfg: dict):
    """Instantiate `agent_cfg["agent_cls"]` with the whole config as keyword arguments
    (schedulers/__init__.py:16-20)."""
    cls = agent_cfg["agent_cls"]
    if cls not in SCHEDULER_CLASSES:
        raise AssertionError(f"'{cls}' is not a valid scheduler.")
    return (globals().get(cls) or __getattr__(cls))(**deepcopy(agent_cfg))


def host_scheduler(name: str, num_executors: int, seed: int = 42, alpha=None):
    """The host scheduler whose device equivalent is policy kind `POLICY_KINDS[name]`: fair, fifo, random, sjf,
    sjf-cp; or "wfair" with `alpha` (default -1): kind `_abi.wfair_kind(alpha)`."""
    if name == "wfair":
        return WeightedFairScheduler(num_executors, alpha=-1.0 if alpha is None else alpha)
    if alpha is not None:
        raise ValueError(f"alpha= goes with scheduler 'wfair' only, not '{name}'")
    if name not in POLICY_KINDS:
        raise ValueError(f"unknown scheduler '{name}' (one of {sorted(POLICY_KINDS)})")
    if name == "random":
        return RandomScheduler(seed=seed)
    if name in ("sjf", "sjf-cp"):
        return ShortestJobFirstScheduler(num_executors, critical_path=name == "sjf-cp")
    return RoundRobinScheduler(num_executors, dynamic_partition=name == "fair")
