"""Behaviour cloning of a device heuristic into a DecimaScheduler.

The heuristic schedulers run on the device engine at 10^7 decisions/s and beat an untrained (or briefly PPO-trained)
Decima policy; PPO from a random initialisation was the only way into the policy. A TEACHER ROLLOUT
(trainers/rollouts.py TeacherRolloutCollector, csrc/teacher_rollout.h) records a heuristic's decisions in the form the
learner consumes: the Decima observation rows plus the action as (stage_idx, job_idx, exec_idx). BehaviourCloning fits
the policy to such collections by maximum likelihood with the learner path PPO uses (learner_counts / minibatch_plans
/ evaluate_actions: CPU tensors take the torch path, device tensors the fused kernels).

Per iteration: one teacher collection; the NO-OP samples (stage_idx = -1: the teacher scheduled nothing; they are
recorded so that the trajectory stays complete) are masked out; one device reduction checks that every remaining
sample is expressible under Decima's masks (the chosen node schedulable, exec_idx < exec_cap[job_idx]); then num_epochs
x num_batches shuffled minibatches minimise the mean of -evaluate_actions(...)["lgprobs"], each followed by an Adam
step. The result is a DecimaScheduler: save / load / evaluate_policy(..., "decima", policy=...) need nothing new, and
PPO starts from it with agent_cfg["init_checkpoint"].
"""

from __future__ import annotations

import time
from typing import Any

import numpy as np
import torch

from ..schedulers.decima import DagBatch, DecimaScheduler, argmax_pick, learner_counts, minibatch_plans, select_envs
from .rollouts import ArenaRolloutBuffer, TeacherRolloutCollector

ACT_KEYS = ("stage_idx", "job_idx", "exec_idx")


def drop_noops(obs: DagBatch, acts: dict):
    """The samples a cloning loss is taken over: those with stage_idx >= 0. Returns (observations, actions, their
    indices in the buffer's sample order, the number of no-op samples dropped)."""
    keep = torch.nonzero(acts["stage_idx"] >= 0).squeeze(1)
    n = int(acts["stage_idx"].numel())
    if int(keep.numel()) == n:
        return obs, {k: acts[k] for k in ACT_KEYS}, keep, 0
    return select_envs(obs, keep), {k: acts[k][keep] for k in ACT_KEYS}, keep, n - int(keep.numel())


def first_invalid(obs: DagBatch, acts: dict) -> int:
    """The mask-validity condition of behaviour cloning, in ONE device reduction: the index of the first sample whose
    action Decima's masks cannot express (stage_idx outside the sample's schedulable nodes, job_idx outside its DAGs,
    or exec_idx >= exec_cap[job_idx]); -1 when every sample is valid. `acts` holds no no-op samples."""
    n = obs.num_envs
    if n == 0:
        return -1
    si, ji, ei = (acts[k].long() for k in ACT_KEYS)
    num_dags = obs.obs_ptr[1:] - obs.obs_ptr[:-1]
    job_ok = (ji >= 0) & (ji < num_dags)
    cap = obs.exec_cap[(ji.clamp(min=0) + obs.obs_ptr[:-1]).clamp(max=max(int(obs.exec_cap.numel()) - 1, 0))]
    bad = ~((si >= 0) & (si < obs.num_stage_acts) & job_ok & (ei >= 0) & (ei < cap))
    idx = torch.arange(n, device=bad.device)
    first = int(torch.where(bad, idx, torch.full_like(idx, n)).min().item())
    return -1 if first == n else first


@torch.no_grad()
def agreement(policy: DecimaScheduler, obs: DagBatch, acts: dict):
    """Per sample: whether the policy's arg-max stage (the first maximal schedulable node) is the teacher's stage, and
    whether the arg-max of its exec scores for the teacher's job is the teacher's exec action."""
    B = obs.num_envs
    dev = obs.x.device
    h = policy.encoder(obs, per_obs_no_mp=True)
    scores = policy.stage_policy_network.scores_all(obs, h)
    pick = argmax_pick(scores, obs.stage_mask, obs.node_env, B)
    stage = policy._sched_rows(obs)[pick.clamp(min=0)]
    stage_ok = (pick >= 0) & (stage == acts["stage_idx"].long())
    envs = torch.arange(B, device=dev)
    es, valid = policy.exec_policy_network.scores_grid(obs, h, acts["job_idx"].long() + obs.obs_ptr[:-1], envs)
    N = policy.num_executors
    seg = envs[:, None].expand(B, N).reshape(-1)
    epick = argmax_pick(es.reshape(-1), valid.reshape(-1), seg, B)
    return stage_ok, (epick - envs * N) == acts["exec_idx"].long()


class BehaviourCloning:
    """train_cfg: teacher (a name of POLICY_KINDS, or "wfair" with alpha), num_envs, seed (base seed: iteration i uses
    seed + i * num_envs + row) or seeds (a list of per-iteration seed lists), num_iterations, num_epochs, num_batches,
    lr (or opt_kwargs), max_grad_norm, optional mean_time_limit (drawn per row as PPO draws it)."""

    def __init__(self, agent_cfg: dict, env_cfg: dict, train_cfg: dict, engine_factory=None, dataset=None,
                 device=None):
        self.device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.seed = int(train_cfg.get("seed", 0))
        torch.manual_seed(self.seed)
        self.num_envs = int(train_cfg["num_envs"])
        self.num_iterations = int(train_cfg.get("num_iterations", 1))
        self.num_epochs = int(train_cfg.get("num_epochs", 1))
        self.num_batches = int(train_cfg.get("num_batches", 1))
        self.seeds = train_cfg.get("seeds")
        env_cfg = dict(env_cfg)
        self.env_cfg = env_cfg
        self.mean_time_limit = train_cfg.get("mean_time_limit", env_cfg.get("mean_time_limit"))
        kw = {k: v for k, v in agent_cfg.items() if k not in ("agent_cls", "init_checkpoint")}
        opt_kwargs = dict(train_cfg.get("opt_kwargs") or {})
        if "lr" in train_cfg:
            opt_kwargs["lr"] = float(train_cfg["lr"])
        self.scheduler = DecimaScheduler(env_cfg["num_executors"], opt_cls=train_cfg.get("opt_cls", "Adam"),
                                         opt_kwargs=opt_kwargs, max_grad_norm=train_cfg.get("max_grad_norm"),
                                         **kw).to(self.device)
        if agent_cfg.get("init_checkpoint"):
            init = DecimaScheduler.load(agent_cfg["init_checkpoint"])
            self.scheduler.load_state_dict(init.state_dict())
        if dataset is None:
            from ..env import resolve_dataset

            dataset = resolve_dataset(env_cfg)
        sim_cfg = {k: v for k, v in env_cfg.items() if k not in ("mean_time_limit", "dataset")}
        if engine_factory is None:
            from ..engine import DeviceEngine

            def engine_factory(cfg, n, ds):
                return DeviceEngine(cfg, n, ds, device=self.device)
        self.engine = engine_factory(sim_cfg, self.num_envs, dataset)
        self.collector = TeacherRolloutCollector(self.engine, train_cfg["teacher"], alpha=train_cfg.get("alpha"),
                                                 seed=self.seed * 7919)
        self.gen = torch.Generator(device=self.device).manual_seed(self.seed * 7919)
        self.time_limit_rngs = [np.random.RandomState(42) for _ in range(self.num_envs)] if self.mean_time_limit else None
        self.iteration = 0

    # ------------------------------------------------------------------ collection
    def _seeds(self) -> list[int]:
        if self.seeds is not None:
            s = self.seeds[self.iteration % len(self.seeds)] if isinstance(self.seeds[0], (list, tuple)) else self.seeds
            assert len(s) == self.num_envs, f"{len(s)} seeds for {self.num_envs} envs"
            return [int(x) for x in s]
        return [self.seed + self.iteration * self.num_envs + r for r in range(self.num_envs)]

    def _time_limits(self, seeds):
        if not self.time_limit_rngs:
            return None
        lim = []
        for i, s in enumerate(seeds):
            if s:
                self.time_limit_rngs[i] = np.random.RandomState(s)
            lim.append(float(self.time_limit_rngs[i].exponential(self.mean_time_limit)))
        return np.array(lim)

    def collect(self) -> ArenaRolloutBuffer:
        seeds = self._seeds()
        return self.collector.collect(seeds, self._time_limits(seeds))

    # ------------------------------------------------------------------ learning
    def _loss(self, obs: DagBatch, acts: dict, plan=None, checked: bool = False) -> torch.Tensor:
        """The mean negative log-likelihood of the teacher's actions. The samples must not hold no-ops: evaluate_actions
        would index job_idx = -1 into the previous sample's DAGs without an error, so unless the caller has `checked`
        (the trainer drops them and validates the rest once per iteration) this raises on the first one."""
        if not checked and bool((acts["stage_idx"] < 0).any()):
            bad = int(torch.nonzero(acts["stage_idx"] < 0)[0])
            raise ValueError(f"behaviour cloning: sample {bad} is a no-op decision (stage_idx -1); no-op samples are "
                             f"masked out of the loss (drop_noops)")
        ev = self.scheduler.evaluate_actions(obs, acts["stage_idx"], acts["job_idx"], acts["exec_idx"], plan=plan)
        return -ev["lgprobs"].mean()

    def _chunks(self, obs: DagBatch, counts, n: int):
        bs = n // self.num_batches + 1
        idx = torch.arange(n, device=obs.x.device)
        groups = [idx[k: k + bs] for k in range(0, n, bs)]
        return groups, minibatch_plans(obs, counts, groups)

    @torch.no_grad()
    def evaluate(self, obs: DagBatch, acts: dict, counts=None) -> dict[str, float]:
        """Mean NLL and the two agreement shares of the current policy over (no-op-free) samples, in num_batches chunks."""
        n = obs.num_envs
        if n == 0:
            return {"nll": float("nan"), "stage_agreement": float("nan"), "exec_agreement": float("nan")}
        self.scheduler.eval()
        counts = learner_counts(obs) if counts is None else counts
        groups, plans = self._chunks(obs, counts, n)
        tot = torch.zeros(3, dtype=torch.float64, device=obs.x.device)
        for idx, (sizes, plan) in zip(groups, plans):
            b = select_envs(obs, idx, sizes)
            a = {k: acts[k][idx] for k in ACT_KEYS}
            ev = self.scheduler.evaluate_actions(b, a["stage_idx"], a["job_idx"], a["exec_idx"], plan=plan)
            s_ok, e_ok = agreement(self.scheduler, b, a)
            tot += torch.stack([-ev["lgprobs"].double().sum(), s_ok.double().sum(), e_ok.double().sum()])
        nll, s, e = (tot / n).tolist()
        return {"nll": nll, "stage_agreement": s, "exec_agreement": e}

    def _update(self, loss: torch.Tensor) -> None:
        s = self.scheduler
        loss.backward()
        if s.max_grad_norm:
            torch.nn.utils.clip_grad_norm_([p for p in s.parameters() if p.grad is not None], s.max_grad_norm,
                                           error_if_nonfinite=True)
        s.optim.step()
        s.optim.zero_grad()

    def train_on_buffer(self, buf: ArenaRolloutBuffer) -> dict[str, Any]:
        obs_all, acts_all = buf.samples()
        obs, acts, keep, noops = drop_noops(obs_all, acts_all)
        n = obs.num_envs
        bad = first_invalid(obs, acts)
        if bad >= 0:
            env, k, _ = buf._sample_rows()
            i = int(keep[bad])
            raise ValueError(f"behaviour cloning: env {int(env[i])} sample {int(k[i])} (stage_idx "
                             f"{int(acts['stage_idx'][bad])}, job_idx {int(acts['job_idx'][bad])}, exec_idx "
                             f"{int(acts['exec_idx'][bad])}) is not expressible under Decima's masks (the node is not "
                             f"schedulable, or exec_idx >= exec_cap[job_idx])")
        counts = learner_counts(obs)
        before = self.evaluate(obs, acts, counts)
        self.scheduler.train()
        bs = n // self.num_batches + 1
        steps = 0
        for _ in range(self.num_epochs if n else 0):
            perm = torch.randperm(n, device=obs.x.device, generator=self.gen)
            groups = [perm[k: k + bs] for k in range(0, n, bs)]
            for idx, (sizes, plan) in zip(groups, minibatch_plans(obs, counts, groups)):
                loss = self._loss(select_envs(obs, idx, sizes), {k: acts[k][idx] for k in ACT_KEYS}, plan, checked=True)
                self._update(loss)
                steps += 1
        after = self.evaluate(obs, acts, counts)
        return {"nll_before": before["nll"], "nll_after": after["nll"], "stage_agreement": after["stage_agreement"],
                "exec_agreement": after["exec_agreement"], "stage_agreement_before": before["stage_agreement"],
                "exec_agreement_before": before["exec_agreement"], "samples": n, "noop_samples": noops,
                "adam_steps": steps}

    def _sync(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def train(self, num_iterations: int | None = None, log=print) -> list[dict]:
        hist = []
        for _ in range(num_iterations or self.num_iterations):
            t0 = time.perf_counter()
            buf = self.collect()
            self._sync()
            t1 = time.perf_counter()
            rec = self.train_on_buffer(buf)
            self._sync()
            t2 = time.perf_counter()
            rec = {"iteration": self.iteration, **rec, "seconds_collect": t1 - t0, "seconds_learn": t2 - t1}
            hist.append(rec)
            self.iteration += 1
            if log is not None:
                log(f"BC iteration {self.iteration}: nll {rec['nll_before']:.4f} -> {rec['nll_after']:.4f}, stage "
                    f"agreement {rec['stage_agreement']:.3f}, exec agreement {rec['exec_agreement']:.3f}, "
                    f"{rec['samples']} samples (+{rec['noop_samples']} no-ops)")
        return hist
