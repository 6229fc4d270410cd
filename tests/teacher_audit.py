"""TEST INFRASTRUCTURE ONLY — audits a sample arena filled by a teacher rollout (ssim_teacher_rollout,
csrc/teacher_rollout.h; or its host build, tests/hostsim/teacher.cpp) against the CPU oracle: the env
(oracle/restatement.py), the Decima observation wrapper (oracle/decima.py) and, for the deterministic teachers, the host
scheduler that specifies the kind (spark_sched_sim.schedulers.host_scheduler).

ONE walk per env drives the oracle from reset(seed, limit) with the launch's LOGGED actions (the device's action log,
as cases.case_rollout_replay replays it) and checks, per decision, raising parity.Mismatch on the first failure:

  observation   node features and schedulable flags, edge links and edge-mask words, DAG node counts and commit caps,
                bit for bit (parity.compare_decima on decima_audit.sample_observation), and the depth
  times         wall_before bit for bit, the reward under parity.reward_close (as decima_audit compares it)
  action        stage_idx / num_exec equal to the log; job_idx the DAG of the chosen node and exec_idx = num_exec - 1;
                a no-op (logged stage_idx -1) recorded as stage_idx = -1, job_idx = -1, exec_idx = 0; lgprob == 0
  validity      every non-no-op sample is expressible under Decima's masks: stage_idx below the number of schedulable
                nodes and exec_idx < the commit cap of job_idx (trainers/imitation.py checks the same on the device)
  consistency   node / edge / DAG offsets the running sums of the earlier samples' counts, and the arena's sample count
                equal to the episode's decision count (the logged decisions, and the episode over after them)
  teacher       deterministic kinds only: the logged action equals the host scheduler's on the oracle's observation

  collect_logged   one collection into an arena with an action log per launch (any engine with teacher_rollout)
  audit            the checks; returns per-sample arrays (env, k, nodes, dags, sched, noop, stage_idx, job_idx, exec_idx,
                   cap, scratch: where the features' scratch of the decision lay for a given plan cap)
  reference_walk   the same walk with the host scheduler's own actions and no arena (what a correct rollout records:
                   decisions and no-ops per env), for choosing seeds and limits on the CPU
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import decima_audit as A
import parity
from oracle.decima import decima_observation
from oracle.decima_gnn import job_of_stage
from oracle.restatement import SparkSchedOracle
from spark_sched_sim import _abi
from spark_sched_sim.schedulers import host_scheduler

LOG_STEPS = 512  # decisions per env and launch the action log holds


def scheduler_of(teacher: str, num_executors: int, alpha=None):
    """The host scheduler of a deterministic teacher (None for "random": its device stream is counter-based)."""
    return None if teacher == "random" else host_scheduler(teacher, num_executors, alpha=alpha)


def kind_of(teacher: str, alpha=None) -> int:
    return _abi.wfair_kind(alpha) if teacher == "wfair" else _abi.POLICY_KINDS[teacher]


def collect_logged(eng, arena, kind: int, seed: int, seeds, limits) -> SimpleNamespace:
    """reset_sampled(seeds, limits), then teacher launches of at most LOG_STEPS decisions per env, each with an action
    log of its own, until no env stopped on a full arena or on the launch's step cap; the arena grows between launches
    as the collectors grow it. Returns the logged actions per env ([n_e][2] int32), launches and growths."""
    B = eng.num_envs
    lim = None if limits is None else np.array([np.inf if x is None else float(x) for x in limits], dtype=np.float64)
    eng.reset_sampled(_abi.SSIM_RESET_SEED, seeds=np.asarray(seeds, dtype=np.uint64), time_limits=lim)
    arena.clear()
    actions = [np.zeros((0, 2), dtype=np.int32) for _ in range(B)]
    launches = grown = 0
    while True:
        before = arena.cursor[:, _abi.CUR_SAMPLES].cpu().numpy().copy()
        log = eng.alloc_action_log(LOG_STEPS)
        eng.teacher_rollout(kind, seed, LOG_STEPS, arena, action_log=log)
        launches += 1
        cur = arena.cursor.cpu().numpy()
        lg = np.asarray(eng.to_numpy(log))
        took = cur[:, _abi.CUR_SAMPLES] - before
        for e in range(B):
            actions[e] = np.concatenate([actions[e], lg[: int(took[e]), e]])
        full = bool((cur[:, _abi.CUR_FULL] != 0).any())
        if full:
            arena.grow(cur)
            grown += 1
        if not full and not (took >= LOG_STEPS).any():
            break
    v = eng.host_views()
    err = np.asarray(v["counts"])[:, _abi.OC_ERR]
    assert not err.any(), [hex(int(x)) for x in err]
    return SimpleNamespace(actions=actions, launches=launches, grown=grown)


def _walk_env(env_cfg, dataset, env, seed, limit, sched, arena, actions, complete, max_decisions, plan_cap):
    N = env_cfg["num_executors"]
    limit = float("inf") if limit is None else float(limit)
    o = SparkSchedOracle(env_cfg, dataset)
    obs, _ = o.reset(seed=int(seed), options={"time_limit": limit})
    ns = int(arena.cursor[env, _abi.CUR_SAMPLES]) if arena is not None else max_decisions
    if arena is not None and len(actions) != ns:
        raise parity.Mismatch(f"env{env}: the arena holds {ns} samples, the launches logged {len(actions)} decisions")
    rows, over, off = [], False, [0, 0, 0]
    for k in range(ns):
        where = f"env{env} sample{k}"
        if over:
            if arena is None:
                break
            raise parity.Mismatch(f"{where}: recorded after the reference episode ended ({k} decisions)")
        dobs = decima_observation(obs, N)
        nsch = int(np.count_nonzero(dobs["stage_mask"]))
        want = None
        if sched is not None:
            a, _ = sched.schedule(obs)
            want = (int(a["stage_idx"]), int(a["num_exec"]))
        si, ne = want if arena is None else (int(actions[k][0]), int(actions[k][1]))
        if arena is not None:
            if want is not None and (si, ne) != want:
                raise parity.Mismatch(f"{where}: teacher: logged action {(si, ne)}, the host scheduler chooses {want}")
            r = A.sample_record(arena, env, k)
            parity.compare_decima(dobs, A.sample_observation(arena, env, k, N), where)
            if np.float64(r["wall_before"]).tobytes() != np.float64(o.wall_time).tobytes():
                raise parity.Mismatch(f"{where}: wall_before {r['wall_before']!r} != {float(o.wall_time)!r}")
            for name, w in (("node_off", off[0]), ("edge_off", off[1]), ("dag_off", off[2])):
                if r[name] != w:
                    raise parity.Mismatch(f"{where}: {name} {r[name]} != running sum {w}")
            off = [off[0] + r["num_nodes"], off[1] + r["num_edges"], off[2] + r["num_dags"]]
            levels = int(np.asarray(dobs["edge_masks"]).shape[0])
            if max(r["depth"] - 1, 0) != levels:
                raise parity.Mismatch(f"{where}: depth {r['depth']} vs {levels} oracle edge-mask levels")
            if si < 0 and (r["stage_idx"], r["job_idx"], r["exec_idx"]) != (-1, -1, 0):
                raise parity.Mismatch(f"{where}: no-op recorded as stage_idx {r['stage_idx']}, job_idx {r['job_idx']}, "
                                      f"exec_idx {r['exec_idx']} (want -1, -1, 0)")
            if (r["stage_idx"], r["num_exec"]) != (si, ne):
                raise parity.Mismatch(f"{where}: stage_idx / num_exec {(r['stage_idx'], r['num_exec'])} != the logged "
                                      f"action {(si, ne)}")
            if r["lgprob"] != 0.0:
                raise parity.Mismatch(f"{where}: lgprob {r['lgprob']!r} != 0")
        if si < 0:
            job, cap = -1, 0
        else:
            if not si < nsch:
                raise parity.Mismatch(f"{where}: validity: stage_idx {si} outside the {nsch} schedulable stages")
            job = job_of_stage(dobs, si)
            cap = int(dobs["commit_caps"][job])
            if arena is not None:
                if r["job_idx"] != job:
                    raise parity.Mismatch(f"{where}: job_idx {r['job_idx']} != DAG of stage {si} ({job})")
                if r["exec_idx"] != ne - 1:
                    raise parity.Mismatch(f"{where}: exec_idx {r['exec_idx']} != num_exec {ne} - 1")
            if not 0 <= ne - 1 < cap:
                raise parity.Mismatch(f"{where}: validity: exec_idx {ne - 1} outside commit cap {cap} of job {job}")
        n = int(dobs["stage_mask"].shape[0])
        rows.append(dict(env=env, k=k, nodes=n, dags=len(dobs["dag_ptr"]) - 1, sched=nsch, noop=si < 0, stage_idx=si,
                         job_idx=job, exec_idx=ne - 1 if si >= 0 else 0, num_exec=ne, cap=cap,
                         scratch="lds" if n <= plan_cap and len(dobs["dag_ptr"]) - 1 <= A.LDS_PLAN_DAGS else "global"))
        try:
            obs, rew, term, _, info = o.step({"stage_idx": si, "num_exec": ne})
        except (ValueError, KeyError) as err:
            raise parity.Mismatch(f"{where}: the oracle env refuses the logged action ({si}, {ne}): {err}")
        if arena is not None and not parity.reward_close(r["reward"], float(rew), o.beta, len(o.jobs)):
            raise parity.Mismatch(f"{where}: reward {r['reward']!r} != {rew!r}")
        over = bool(term) or info["wall_time"] >= limit
    if arena is not None and complete and not over:
        raise parity.Mismatch(f"env{env}: {ns} samples recorded, the reference episode goes on (wall {o.wall_time!r}, "
                              f"limit {limit!r})")
    return rows, over


def _report(rows, over):
    rep = {key: np.array([r[key] for r in rows]) for key in rows[0]} if rows else {}
    rep["episode_over"] = over
    return rep


def audit(arena, env_cfg: dict, dataset, seeds, limits, actions, teacher: str, alpha=None, plan_cap: int = 0,
          complete: bool = True, envs=None) -> dict:
    """Audits a host copy (decima_audit.host_arena) of ONE teacher collection that started with reset(seeds[e],
    limits[e]); `actions`: the logged decisions per env (collect_logged). The module docstring lists the checks."""
    rows, over = [], []
    for e in (range(arena.cursor.shape[0]) if envs is None else envs):
        sched = scheduler_of(teacher, env_cfg["num_executors"], alpha)
        r, ov = _walk_env(env_cfg, dataset, e, seeds[e], None if limits is None else limits[e], sched, arena,
                          actions[e], complete, 0, plan_cap)
        rows += r
        over.append(ov)
    return _report(rows, over)


def reference_walk(env_cfg: dict, dataset, seeds, limits, teacher: str, alpha=None, plan_cap: int = 0,
                   max_decisions: int = 10**9) -> dict:
    """The collection a correct teacher rollout records for a deterministic teacher, without an engine: the oracle
    driven by the host scheduler. The report of `audit`."""
    rows, over = [], []
    for e in range(len(seeds)):
        sched = scheduler_of(teacher, env_cfg["num_executors"], alpha)
        assert sched is not None, "the random teacher has no host reference"
        r, ov = _walk_env(env_cfg, dataset, e, seeds[e], None if limits is None else limits[e], sched, None, None, True,
                          max_decisions, plan_cap)
        rows += r
        over.append(ov)
    return _report(rows, over)
