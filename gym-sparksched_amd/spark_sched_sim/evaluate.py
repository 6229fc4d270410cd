"""Whole-episode evaluation of a device policy kind: one env per seed, every decision taken on the device.

`evaluate_policy(env_cfg, "sjf-cp", seeds)` resets one env per seed, repeats fused rollout launches (policy + step in
one kernel, `DeviceEngine.rollout`) until every episode has terminated, and returns each env's average job duration
in seconds computed like `metrics.avg_job_duration` — the number `examples.py` prints for one env driven from the
host, here for thousands of envs with no host round trip per decision. It takes any policy kind of
`_abi.POLICY_KINDS` (fair, fifo, random, sjf, sjf-cp), by name or by its SSIM_POLICY_* value.
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


def evaluate_policy(env_cfg: dict, kind, seeds, device=None, dataset=None, engine_factory=None,
                    max_launches: int = 64, steps_per_launch: int = 256, policy_seed: int = 0) -> dict:
    """Runs one episode per seed under device policy `kind` to termination.

    engine_factory(env_cfg, num_envs, dataset) builds the engine (default: a `DeviceEngine` on `device`, "cuda" when
    None; the tests pass the host build's). Each launch gives every running env up to `steps_per_launch` decisions;
    a terminated env takes no more. Raises RuntimeError if an env reports an error or is still running after
    `max_launches` launches (an env without `job_arrival_cap` never terminates).

    Returns {"avg_job_duration": float64 [B] seconds, "completed_jobs": int64 [B], "decisions": int64 [B],
    "wall_time": float64 [B] ms, "launches": int}."""
    from .env import resolve_dataset

    kind = policy_kind(kind)
    seeds = [int(s) for s in seeds]
    dataset = resolve_dataset(env_cfg, dataset)
    if engine_factory is None:
        from .engine import DeviceEngine

        engine = DeviceEngine(env_cfg, len(seeds), dataset, device="cuda" if device is None else device)
    else:
        engine = engine_factory(env_cfg, len(seeds), dataset)
    try:
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
            engine.rollout(kind, policy_seed, steps_per_launch)
            launches += 1
        return {"avg_job_duration": avg_job_durations(engine),
                "completed_jobs": counts[:, _abi.OC_NUM_COMPLETED].astype(np.int64),
                "decisions": counts[:, _abi.OC_DECISIONS].astype(np.int64),
                "wall_time": np.asarray(engine.host_views()["wall_time"], dtype=np.float64).copy(),
                "launches": launches}
    finally:
        engine.close()
