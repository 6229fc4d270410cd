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


class WeightedFairScheduler(Scheduler):
    """Weighted fair, WFair(alpha): the fair scheduler with the executors shared in proportion to work^alpha; the
    specification the device kinds `SSIM_POLICY_WFAIR_BASE + (2 alpha + 4)` (csrc/policy.h wfair_act) follow action
    for action. alpha is a half-integer in [-2, 2] (alpha2 = 2 alpha), so that every step is one correctly rounded
    float64 operation (multiply, divide, square root, add) and numpy, the host build and the device agree bit for bit.

    W(k): `ShortestJobFirstScheduler.job_work`. p(k) = h(W(k), alpha2) for W(k) > 0, with h(w, a) for a = 0..4 being
    1, sqrt(w), w, w * sqrt(w), w * w and 1 / h(w, -a) for a < 0; for W(k) == 0, p(k) is 1 if alpha2 == 0, else 0.
    P = the sum of p in blocks of 64 consecutive jobs (zero-padded), each block folded by halves (x[:32] + x[32:], then
    16, 8, 4, 2, 1), the block sums added left to right from 0.0. cap(k) = min(N, ceil((N * p(k)) / P)).
    The action is `RoundRobinScheduler`'s with that cap: the source job with every committable executor if it has a
    schedulable stage; else the first job k != src in arrival order with supply(k) < cap(k) and a schedulable stage,
    with min(committable, cap(k) - supply(k)) executors; else (and whenever P == 0) stage_idx -1. alpha = 0 is the
    fair scheduler. A pure function of the observation."""

    def __init__(self, num_executors: int, alpha: float = -1.0, **kwargs):
        from .._abi import wfair_alpha, wfair_kind

        self.kind = wfair_kind(alpha)  # (ValueError off the grid)
        self.alpha = wfair_alpha(self.kind)
        self.alpha2 = int(2 * self.alpha)
        self.name = f"WFair({self.alpha:g})"
        self.num_executors = num_executors
        self.env_wrapper_cls = None

    @staticmethod
    def weight(w, alpha2: int) -> np.float64:
        """p = w^(alpha2 / 2) by the rule's operations."""
        w = np.float64(w)
        if not w > 0.0:
            return np.float64(1.0 if alpha2 == 0 else 0.0)
        a = abs(alpha2)
        h = (np.float64(1.0), np.sqrt(w), w, w * np.sqrt(w), w * w)[a]
        return np.float64(1.0) / h if alpha2 < 0 else h

    @staticmethod
    def total(p) -> np.float64:
        """P: the fold-halves sum of each block of 64 weights, the block sums added left to right."""
        p = np.asarray(p, dtype=np.float64)
        total = np.float64(0.0)
        for k0 in range(0, len(p), 64):
            x = np.zeros(64, dtype=np.float64)
            x[:len(p[k0:k0 + 64])] = p[k0:k0 + 64]
            half = 32
            while half:
                x = x[:half] + x[half:2 * half]
                half //= 2
            total = total + x[0]
        return total

    def cap(self, p, total) -> int:
        """min(N, ceil((N * p) / P)) for P > 0."""
        c = np.ceil((np.float64(self.num_executors) * np.float64(p)) / np.float64(total))
        return int(c) if c < self.num_executors else self.num_executors

    def weights(self, obs: dict) -> list:
        w = ShortestJobFirstScheduler.row_work(obs)
        return [self.weight(ShortestJobFirstScheduler.job_work(obs, w, k), self.alpha2)
                for k in range(len(obs["exec_supplies"]))]

    def other_jobs(self, obs: dict, p, total) -> dict:
        """The action when the source job is not served, from the weights `p` and their sum `total` (after
        preprocess_obs): the first job other than the source under its cap with a schedulable stage."""
        supplies = obs["exec_supplies"]
        committable = obs["num_committable_execs"]
        if total > 0.0:
            for j in range(len(supplies)):
                if j == obs["source_job_idx"]:
                    continue
                cap = self.cap(p[j], total)
                if supplies[j] >= cap:
                    continue
                k = find_stage(obs, j)
                if k != -1:
                    return {"stage_idx": k, "num_exec": min(committable, cap - supplies[j])}
        return {"stage_idx": -1, "num_exec": committable}

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        src = obs["source_job_idx"]
        if src < len(obs["exec_supplies"]):
            k = find_stage(obs, src)
            if k != -1:
                return {"stage_idx": k, "num_exec": obs["num_committable_execs"]}, {}
        p = self.weights(obs)
        return self.other_jobs(obs, p, self.total(p)), {}


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
