"""Whole-episode evaluation of a device policy kind: one env per seed, every decision taken on the device.

`evaluate_policy(env_cfg, "sjf-cp", seeds)` resets one env per seed, repeats fused rollout launches (policy + step in
one kernel, `DeviceEngine.rollout`) until every episode has terminated, and returns each env's average job duration
in seconds computed like `metrics.avg_job_duration` — the number `examples.py` prints for one env driven from the
host, here for thousands of envs with no host round trip per decision. It takes any policy kind of
`_abi.POLICY_KINDS` (fair, fifo, random, sjf, sjf-cp), by name or by its SSIM_POLICY_* value, "wfair" with `alpha=` a
half-integer in [-2, 2] (weighted fair; `tune_weighted_fair` sweeps the exponent), or "decima" with
`policy=` a `DecimaScheduler` or a checkpoint path (`DecimaScheduler.save`): the persistent Decima rollout, greedy
(arg-max actions, `_abi.SSIM_ROLLOUT_GREEDY`) or sampled, on the same seeds as the heuristics.

The numbers come from `DeviceEngine.episode_stats()` (a per-env reduction on the device); `avg_job_durations(engine)`
is the host-side restatement the tests check it against, `job_table_stats(engine)` the same rows from the job tables
for an engine that has no `episode_stats` (a host test double).
"""

from __future__ import annotations

import numpy as np

from . import _abi


def policy_kind(kind) -> int:
    """A policy kind given by name (`_abi.POLICY_KINDS`) or by value."""
    if isinstance(kind, str):
        if kind not in _abi.POLICY_KINDS:
            raise ValueError(f"unknown policy '{kind}' (one of {sorted(_abi.POLICY_KINDS)})")
        return _abi.POLICY_KINDS[kind]
    if int(kind) not in _abi.POLICY_KINDS.values():
        raise ValueError(f"unknown policy kind {kind}")
    return int(kind)


def avg_job_durations(engine) -> np.ndarray:
    """Per env, `metrics.avg_job_duration` in seconds: the mean over the arrived jobs of min(t_completed, wall
    time) - t_arrival (nan for an env with no arrived job)."""
    ta, tc, st = (np.asarray(x) for x in engine.job_times_np())
    wall = np.asarray(engine.host_views()["wall_time"], dtype=np.float64)
    out = np.full(ta.shape[0], np.nan)
    for e in range(ta.shape[0]):
        arrived = np.nonzero(st[e] > 0)[0]
        if len(arrived):
            out[e] = np.mean([float(min(tc[e, j], wall[e]) - ta[e, j]) for j in arrived]) * 1e-3
    return out


def stats_avg_job_durations(stats: np.ndarray) -> np.ndarray:
    """`avg_job_durations` from `engine.episode_stats()` rows: duration sum (ms) / arrived jobs, in seconds (nan for
    an env with no arrived job)."""
    stats = np.asarray(stats, dtype=np.float64)
    out = np.full(stats.shape[0], np.nan)
    some = stats[:, 1] > 0
    out[some] = stats[some, 0] / stats[some, 1] * 1e-3
    return out


def job_table_stats(engine) -> np.ndarray:
    """The rows of `engine.episode_stats()` from the job tables copied to the host (`job_times_np`, `host_views`): for
    an engine without that entry (a host test double), and the reduction's restatement in numpy."""
    ta, tc, st = (np.asarray(x) for x in engine.job_times_np())
    wall = np.asarray(engine.host_views()["wall_time"], dtype=np.float64)
    arrived = st > 0
    dur = np.where(arrived, np.minimum(tc, wall[:, None]) - ta, 0.0)
    return np.stack([dur.sum(axis=1), arrived.sum(axis=1).astype(np.float64),
                     (st == 2).sum(axis=1).astype(np.float64), wall], axis=1)


def evaluate_policy(env_cfg: dict, kind, seeds, device=None, dataset=None, engine_factory=None,
                    max_launches: int = 64, steps_per_launch: int = 256, policy_seed: int = 0, policy=None,
                    greedy: bool = True, action_log: list | None = None, alpha=None) -> dict:
    """Runs one episode per seed under device policy `kind` to termination.

    kind "wfair": weighted fair with exponent `alpha` (a half-integer in [-2, 2], default -1; `_abi.wfair_kind`), or
    one of the weighted-fair kinds by value. `alpha=` with any other kind is a ValueError.

    kind "decima": `policy` is a `DecimaScheduler` or the path of a checkpoint (`DecimaScheduler.save`); every launch
    is a persistent Decima rollout of up to `steps_per_launch` decisions per env, with the arg-max action (`greedy`,
    the default: `_abi.SSIM_ROLLOUT_GREEDY`) or sampled with `policy_seed`, each launch's counter continuing from the
    decisions already taken (an env's n-th decision draws from (policy_seed, env, n) however the launches split).
    `action_log` (a list) receives each launch's device log as a numpy array [steps_per_launch][B][2], rows an env did
    not reach being -1.

    engine_factory(env_cfg, num_envs, dataset) builds the engine (default: a `DeviceEngine` on `device`, "cuda" when
    None; the tests pass the host build's). Each launch gives every running env up to `steps_per_launch` decisions;
    a terminated env takes no more. Raises RuntimeError if an env reports an error or is still running after
    `max_launches` launches (an env without `job_arrival_cap` never terminates).

    Returns {"avg_job_duration": float64 [B] seconds, "completed_jobs": int64 [B], "decisions": int64 [B],
    "wall_time": float64 [B] ms, "launches": int}."""
    from .env import resolve_dataset

    decima = isinstance(kind, str) and kind == "decima"
    if decima:
        if policy is None:
            raise ValueError("evaluate_policy: kind 'decima' needs policy= (a DecimaScheduler or a checkpoint path)")
    else:
        if policy is not None:
            raise ValueError("evaluate_policy: policy= goes with kind 'decima' only")
        if isinstance(kind, str) and kind == "wfair":
            kind = _abi.wfair_kind(-1.0 if alpha is None else alpha)
        elif alpha is not None:
            raise ValueError(f"evaluate_policy: alpha= goes with kind 'wfair' only, not {kind!r}")
        elif not isinstance(kind, str) and _abi.is_wfair_kind(kind):
            kind = int(kind)
        else:
            kind = policy_kind(kind)
    seeds = [int(s) for s in seeds]
    dataset = resolve_dataset(env_cfg, dataset)
    if engine_factory is None:
        from .engine import DeviceEngine

        engine = DeviceEngine(env_cfg, len(seeds), dataset, device="cuda" if device is None else device)
    else:
        engine = engine_factory(env_cfg, len(seeds), dataset)
    try:
        params = log = None
        if decima:
            if not hasattr(engine, "decima_rollout"):
                raise ValueError("evaluate_policy: this engine has no persistent Decima rollout (the host build runs "
                                 "the heuristic kinds only)")
            if isinstance(policy, (str, bytes)) or hasattr(policy, "__fspath__"):
                from .schedulers.decima import DecimaScheduler

                policy = DecimaScheduler.load(policy, device=engine.device)
            if policy.num_executors != env_cfg["num_executors"]:
                raise ValueError(f"evaluate_policy: the policy was built for {policy.num_executors} executors, the env "
                                 f"has {env_cfg['num_executors']}")
            params = policy.packed_params(engine.device)
            if action_log is not None:
                log = engine.alloc_action_log(steps_per_launch)
        engine.reset(seeds=seeds)
        launches = 0
        while True:
            counts = np.asarray(engine.host_views()["counts"])
            err = counts[:, _abi.OC_ERR]
            if err.any():
                bad = int(np.flatnonzero(err)[0])
                raise RuntimeError(f"evaluate_policy: env {bad} (seed {seeds[bad]}) reports error bits "
                                   f"{int(err[bad]):#x}")
            if (counts[:, _abi.OC_TERMINATED] != 0).all():
                break
            if launches >= max_launches:
                raise RuntimeError(f"evaluate_policy: {int((counts[:, _abi.OC_TERMINATED] == 0).sum())} env(s) still "
                                   f"running after {launches} launches of {steps_per_launch} decisions")
            if decima:
                if log is not None:
                    log.fill_(-1)
                # (the kernel's stream is counter + the env's decision index in its episode: 0 keeps draw n of an env
                # at (policy_seed, env, n) in every launch)
                engine.decima_rollout(params, policy_seed, 0, steps_per_launch,
                                      flags=_abi.SSIM_ROLLOUT_GREEDY if greedy else 0, action_log=log)
                if log is not None:
                    action_log.append(engine.to_numpy(log).copy())
            else:
                engine.rollout(kind, policy_seed, steps_per_launch)
            launches += 1
        # (every DeviceEngine reduces on the device; an engine without the entry gives its job tables)
        stats = np.asarray(engine.episode_stats() if hasattr(engine, "episode_stats") else job_table_stats(engine),
                           dtype=np.float64)
        return {"avg_job_duration": stats_avg_job_durations(stats),
                "completed_jobs": stats[:, 2].astype(np.int64),
                "decisions": counts[:, _abi.OC_DECISIONS].astype(np.int64),
                "wall_time": stats[:, 3].copy(),
                "launches": launches}
    finally:
        engine.close()


def tune_weighted_fair(env_cfg: dict, seeds, alphas=None, **kw) -> dict:
    """The tuned weighted-fair baseline: one `evaluate_policy(env_cfg, "wfair", seeds, alpha=a, **kw)` per exponent of
    `alphas` (default: the nine half-integers of [-2, 2]) and the exponent with the smallest mean average job duration
    over the seeds; ties go to the smaller |alpha|, then to the smaller alpha.

    Returns {"alpha": best, "mean_avg_job_duration": {alpha: mean over seeds, seconds}, "per_seed": {alpha: float64
    [len(seeds)]}}."""
    seeds = [int(s) for s in seeds]
    alphas = list(_abi.WFAIR_ALPHAS) if alphas is None else [_abi.wfair_alpha(_abi.wfair_kind(a)) for a in alphas]
    if not alphas:
        raise ValueError("tune_weighted_fair: no exponent to try")
    per_seed = {a: evaluate_policy(env_cfg, "wfair", seeds, alpha=a, **kw)["avg_job_duration"] for a in alphas}
    mean = {a: float(np.mean(d)) for a, d in per_seed.items()}
    best = min(mean, key=lambda a: (mean[a], abs(a), a))
    return {"alpha": best, "mean_avg_job_duration": mean, "per_seed": per_seed}
