"""Host heuristic schedulers over the facade's observation dicts (reference `schedulers/heuristics/`).

These are the policy plugins `examples.py` and the rollout workers call: `schedule(obs) -> (action, info)` on
the single-env obs dict that `SparkSchedSimEnv` returns (`GraphInstance` nodes/edge_links, `dag_ptr`,
`exec_supplies`, `source_job_idx`, `num_committable_execs`). They are pure functions of the observation (plus,
for the random scheduler, a legacy `RandomState` stream), so the actions they return are the reference's for
the same observation. The batched device equivalents used by the vector env live in `csrc/policy.h`.
"""

from __future__ import annotations

import math
from abc import ABC, abstractmethod
from typing import Any

import numpy as np


class Scheduler(ABC):
    """Scheduler interface (schedulers/scheduler.py:10-18)."""

    name: str
    env_wrapper_cls: type | None = None

    @abstractmethod
    def schedule(self, obs: dict) -> tuple[dict, dict]:
        ...


def preprocess_obs(obs: dict[str, Any]) -> None:
    """Adds `frontier_stages` (node rows with no incoming active edge) and `schedulable_stages`
    (node row -> rank among the schedulable rows, i.e. the action's stage_idx) to `obs`
    (heuristics/utils.py:5-17)."""
    graph = obs["dag_batch"]
    n = graph.nodes.shape[0]
    has_parent = np.zeros(n, dtype=bool)
    links = np.asarray(graph.edge_links).reshape(-1, 2)
    if links.shape[0]:
        has_parent[links[:, 1]] = True
    rows = np.flatnonzero(graph.nodes[:, 2].astype(bool))
    obs["frontier_stages"] = set(np.flatnonzero(~has_parent).tolist())
    obs["schedulable_stages"] = {int(r): k for k, r in enumerate(rows.tolist())}


def find_stage(obs: dict[str, Any], job_idx: int) -> int:
    """Action stage_idx of a schedulable stage of job `job_idx`: its first frontier one in node order, else its
    first schedulable one, else -1 (heuristics/utils.py:20-37)."""
    sched = obs["schedulable_stages"]
    frontier = obs["frontier_stages"]
    fallback = -1
    for row in range(int(obs["dag_ptr"][job_idx]), int(obs["dag_ptr"][job_idx + 1])):
        k = sched.get(row)
        if k is None:
            continue
        if row in frontier:
            return k
        if fallback < 0:
            fallback = k
    return fallback


class RoundRobinScheduler(Scheduler):
    """Fair (dynamic_partition) / FIFO scheduler (heuristics/round_robin.py:7-49)."""

    def __init__(self, num_executors: int, dynamic_partition: bool = True, **kwargs):
        self.name = "Fair" if dynamic_partition else "FIFO"
        self.num_executors = num_executors
        self.dynamic_partition = dynamic_partition
        self.env_wrapper_cls = None

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        supplies = obs["exec_supplies"]
        n_jobs = len(supplies)
        committable = obs["num_committable_execs"]
        cap = math.ceil(self.num_executors / max(1, n_jobs)) if self.dynamic_partition else self.num_executors
        src = obs["source_job_idx"]
        if src < n_jobs:  # the job releasing executors keeps all of them if it can use them
            k = find_stage(obs, src)
            if k != -1:
                return {"stage_idx": k, "num_exec": committable}, {}
        for j in range(n_jobs):  # arrival order, below the cap
            if j == src or supplies[j] >= cap:
                continue
            k = find_stage(obs, j)
            if k != -1:
                return {"stage_idx": k, "num_exec": min(committable, cap - supplies[j])}, {}
        return {"stage_idx": -1, "num_exec": committable}, {}


class RandomScheduler(Scheduler):
    """Uniform job, its find_stage pick, uniform executor count (heuristics/random_scheduler.py:7-32).
    Draws from `np.random.RandomState(seed)` in the reference's order: `choice` over the remaining job
    indices until one has a schedulable stage, then `randint(1, committable + 1)`."""

    def __init__(self, seed: int = 42, **kwargs):
        self.name = "Random"
        self.env_wrapper_cls = None
        self.set_seed(seed)

    def set_seed(self, seed: int) -> None:
        self.np_random = np.random.RandomState(seed)

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        candidates = list(range(len(obs["exec_supplies"])))
        k = -1
        while candidates:
            j = self.np_random.choice(candidates)
            k = find_stage(obs, j)
            if k != -1:
                break
            candidates.remove(j)
        num_exec = self.np_random.randint(1, obs["num_committable_execs"] + 1)
        return {"stage_idx": k, "num_exec": num_exec}, {}


class ShortestJobFirstScheduler(Scheduler):
    """Shortest job first, optionally with critical-path stage choice (SJF / SJF-CP); the specification the device
    kinds `SSIM_POLICY_SJF` / `SSIM_POLICY_SJF_CP` (csrc/policy.h) follow action for action.

    w(r) = float64(nodes[r, 0]) * float64(nodes[r, 1]) (remaining tasks x most recent task duration; exact in
    float64). W(k) = the float64 sum of w over job k's rows, added one at a time in row order from 0.0. Among the
    jobs with a schedulable stage (`find_stage(obs, k) != -1`) the one with the smallest (W(k), k) is served with
    every committable executor: SJF takes its `find_stage` stage; SJF-CP its schedulable row with the largest
    cp(r) = w(r) + max(0.0, max over edges (r, c) of cp(c)), the lowest row on ties. With no candidate the action is
    the other heuristics' "nothing to schedule": stage_idx -1. There is no source-job preference and no per-job cap.
    A pure function of the observation."""

    def __init__(self, num_executors: int, critical_path: bool = False, **kwargs):
        self.name = "SJF-CP" if critical_path else "SJF"
        self.num_executors = num_executors
        self.critical_path = critical_path
        self.env_wrapper_cls = None

    @staticmethod
    def row_work(obs: dict) -> np.ndarray:
        nodes = np.asarray(obs["dag_batch"].nodes)
        return nodes[:, 0].astype(np.float64) * nodes[:, 1].astype(np.float64)

    @staticmethod
    def job_work(obs: dict, w: np.ndarray, k: int) -> float:
        total = 0.0
        for r in range(int(obs["dag_ptr"][k]), int(obs["dag_ptr"][k + 1])):
            total += float(w[r])
        return total

    def choose_job(self, obs: dict, w: np.ndarray) -> int:
        """k*: the candidate with the smallest (W, k), -1 if no job has a schedulable stage (after preprocess_obs)."""
        best, best_w = -1, 0.0
        for k in range(len(obs["dag_ptr"]) - 1):
            if find_stage(obs, k) == -1:
                continue
            wk = self.job_work(obs, w, k)
            if best < 0 or wk < best_w:
                best, best_w = k, wk
        return best

    @staticmethod
    def critical_paths(obs: dict, w: np.ndarray, lo: int, hi: int) -> dict:
        """cp(r) of the rows lo <= r < hi of one job (the edges of a job stay within its rows)."""
        links = np.asarray(obs["dag_batch"].edge_links).reshape(-1, 2)
        kids: dict[int, list] = {r: [] for r in range(lo, hi)}
        for u, v in links.tolist():
            if lo <= u < hi:
                kids[int(u)].append(int(v))
        cp: dict[int, float] = {}

        def visit(r):
            if r not in cp:
                tail = 0.0
                for c in kids[r]:
                    tail = max(tail, visit(c))
                cp[r] = float(w[r]) + tail
            return cp[r]

        for r in range(lo, hi):
            visit(r)
        return cp

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        committable = obs["num_committable_execs"]
        w = self.row_work(obs)
        k = self.choose_job(obs, w)
        if k < 0:
            return {"stage_idx": -1, "num_exec": committable}, {}
        if not self.critical_path:
            return {"stage_idx": find_stage(obs, k), "num_exec": committable}, {}
        lo, hi = int(obs["dag_ptr"][k]), int(obs["dag_ptr"][k + 1])
        cp = self.critical_paths(obs, w, lo, hi)
        sched = obs["schedulable_stages"]
        best = -1
        for r in range(lo, hi):
            if r in sched and (best < 0 or cp[r] > cp[best]):
                best = r
        return {"stage_idx": sched[best], "num_exec": committable}, {}
