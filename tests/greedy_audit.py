"""TEST INFRASTRUCTURE ONLY — audits a sample arena filled by a GREEDY persistent Decima rollout (ssim_decima_rollout
with SSIM_ROLLOUT_GREEDY, csrc/decima_policy.h kGreedy) against the CPU oracle, by REGRET and with no skipping.

The sampled audit (tests/decima_audit.py) compares Gumbel-max winners and skips draws inside the score margin; with
the noise at zero that rule skips too much (2.7-3.3% of an untrained policy's decisions lie inside the margin, up to
96% once the tanh layers saturate). Here every recorded choice must be numerically indistinguishable from the best:

  every sample   the env, feature, wall-time, reward and record-consistency checks of decima_audit.audit;
                 lgprob within 1e-4 + 1e-4 |want| of the oracle's log-softmax at the recorded pair;
                 ss[stage_idx] >= max(ss) - s_margin and es[exec_idx] >= max(es) - e_margin, with ss / es from
                 oracle/decima_gnn.py and the margins 2 (1e-5 + 1e-4 max|score|) of decima_audit.

Where the oracle's winner leads by more than the margin this forces the recorded choice to be the winner; elsewhere
it accepts only choices within the margin of the best. A decision is DECISIVE when both leads exceed their margins.

  greedy_policy      the oracle's scores, arg-max winners (first maximal index), leads and margins of one observation
  audit              the checks, per env; raises parity.Mismatch; returns the per-sample report
  reference_rollout  the same walk with the oracle's arg-max actions (what a correct kernel records), no engine
  collect_reference  a sample arena filled on the host build of the engine with the oracle's arg-max actions
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import parity
from decima_audit import (I32, LGPROB_ATOL, LGPROB_RTOL, SCORE_ATOL, SCORE_RTOL, classify, fill_arena_like_kernel,
                          host_arena, sample_observation, sample_record)
from oracle import decima_gnn as G
from oracle.decima import decima_observation
from oracle.restatement import SparkSchedOracle
from spark_sched_sim import _abi

__all__ = ["greedy_policy", "audit", "reference_rollout", "collect_reference", "host_arena"]


def _lead(x: np.ndarray, win: int) -> float:
    return float(x[win] - np.partition(x, -2)[-2]) if x.size > 1 else np.inf


def greedy_policy(sd: dict, dobs: dict, num_executors: int, stage_of=None) -> SimpleNamespace:
    """The oracle policy on one observation, without noise: stage scores `ss` over the schedulable stages, their
    arg-max (first maximal index) and its lead over the runner-up; then, for the DAG of stage `stage_of` (default: the
    winner), the same for the exec scores `es`. Margins as decima_audit._policy."""
    enc = G.encode(sd, dobs)
    ss = G.stage_scores(sd, dobs, enc)
    s = ss.numpy().astype(np.float32)
    s_win = int(np.argmax(s))
    si = s_win if stage_of is None else stage_of
    job = G.job_of_stage(dobs, si)
    es = G.exec_scores(sd, dobs, enc, job, num_executors)
    e = es.numpy().astype(np.float32)
    e_win = int(np.argmax(e)) if e.size else 0
    return SimpleNamespace(ss=ss, es=es, job=job, s_win=s_win, s_lead=_lead(s, s_win), e_win=e_win,
                           e_lead=_lead(e, e_win) if e.size else np.inf,
                           s_margin=2.0 * (SCORE_ATOL + SCORE_RTOL * float(ss.abs().max())),
                           e_margin=2.0 * (SCORE_ATOL + SCORE_RTOL * float(es.abs().max())) if es.numel() else 0.0)


def _lgprob(p, si: int, ei: int) -> float:
    return float(torch.log_softmax(p.ss, 0)[si] + torch.log_softmax(p.es, 0)[ei])


def _walk_env(env_cfg, dataset, env, env_seed, limit, sd, arena, plan_cap, helper, complete, max_decisions):
    """One env: the oracle from reset(env_seed, limit) through the recorded samples (arena given: every check), or
    through the oracle's own arg-max actions (arena None), at most max_decisions of them."""
    N = env_cfg["num_executors"]
    limit = float("inf") if limit is None else float(limit)
    o = SparkSchedOracle(env_cfg, dataset)
    obs, _ = o.reset(seed=int(env_seed), options={"time_limit": limit})
    ns = int(arena.cursor[env, _abi.CUR_SAMPLES]) if arena is not None else max_decisions
    rows, over = [], False
    off = [0, 0, 0]
    for k in range(ns):
        where = f"env{env} sample{k}"
        if over:
            if arena is None:
                break
            raise parity.Mismatch(f"{where}: recorded after the reference episode ended ({k} decisions)")
        dobs = decima_observation(obs, N)
        nsch = int(np.count_nonzero(dobs["stage_mask"]))
        if arena is not None:
            r = sample_record(arena, env, k)
            got = sample_observation(arena, env, k, N)
            parity.compare_decima(dobs, got, where)
            if np.float64(r["wall_before"]).tobytes() != np.float64(o.wall_time).tobytes():
                raise parity.Mismatch(f"{where}: wall_before {r['wall_before']!r} != {float(o.wall_time)!r}")
            want_off = {"node_off": off[0], "edge_off": off[1], "dag_off": off[2]}
            for name, w in want_off.items():
                if r[name] != w:
                    raise parity.Mismatch(f"{where}: {name} {r[name]} != running sum {w}")
            off = [off[0] + r["num_nodes"], off[1] + r["num_edges"], off[2] + r["num_dags"]]
            levels = int(np.asarray(dobs["edge_masks"]).shape[0])
            if max(r["depth"] - 1, 0) != levels:
                raise parity.Mismatch(f"{where}: depth {r['depth']} vs {levels} oracle edge-mask levels")
            if not 0 <= r["stage_idx"] < nsch:
                raise parity.Mismatch(f"{where}: stage_idx {r['stage_idx']} outside the {nsch} schedulable stages")
            job = G.job_of_stage(dobs, r["stage_idx"])
            if r["job_idx"] != job:
                raise parity.Mismatch(f"{where}: job_idx {r['job_idx']} != job of stage {r['stage_idx']} ({job})")
            cap = int(dobs["commit_caps"][job])
            if r["num_exec"] != r["exec_idx"] + 1:
                raise parity.Mismatch(f"{where}: num_exec {r['num_exec']} != exec_idx {r['exec_idx']} + 1")
            if not 0 <= r["exec_idx"] < cap:
                raise parity.Mismatch(f"{where}: exec_idx {r['exec_idx']} outside commit cap {cap} of job {job}")
            si, ei = r["stage_idx"], r["exec_idx"]
            p = greedy_policy(sd, dobs, N, stage_of=si)
            s_best, s_got = float(p.ss.max()), float(p.ss[si])
            if not s_got >= s_best - p.s_margin:
                raise parity.Mismatch(f"{where}: stage choice: recorded {si} scores {s_got!r}, the oracle's best ("
                                      f"{p.s_win}) {s_best!r}: regret {s_best - s_got:.3e} > margin {p.s_margin:.3e}")
            e_best, e_got = float(p.es.max()), float(p.es[ei])
            if not e_got >= e_best - p.e_margin:
                raise parity.Mismatch(f"{where}: exec choice: recorded {ei} scores {e_got!r}, the oracle's best ("
                                      f"{p.e_win}) {e_best!r}: regret {e_best - e_got:.3e} > margin {p.e_margin:.3e}")
            want = _lgprob(p, si, ei)
            if not abs(r["lgprob"] - want) <= LGPROB_ATOL + LGPROB_RTOL * abs(want):
                raise parity.Mismatch(f"{where}: lgprob {r['lgprob']!r} vs oracle {want!r} "
                                      f"(diff {abs(r['lgprob'] - want):.3e})")
            lg = r["lgprob"]
        else:
            p = greedy_policy(sd, dobs, N)
            si, ei, job = p.s_win, p.e_win, p.job
            cap = int(dobs["commit_caps"][job])
            lg = _lgprob(p, si, ei)
        plan, exec_path = classify(dobs, job, N, plan_cap, helper)
        rows.append(dict(env=env, k=k, nodes=int(dobs["stage_mask"].shape[0]), dags=len(dobs["dag_ptr"]) - 1,
                         sched=nsch, cap=cap, plan=plan, exec_path=exec_path, stage_idx=si, exec_idx=ei, job_idx=job,
                         lgprob=lg, decisive=bool(p.s_lead > p.s_margin and p.e_lead > p.e_margin),
                         s_win=p.s_win, e_win=p.e_win))
        try:
            obs, rew, term, _, info = o.step({"stage_idx": int(si), "num_exec": int(ei) + 1})
        except (ValueError, KeyError) as err:
            raise parity.Mismatch(f"{where}: the oracle env refuses the recorded action ({si}, {ei + 1}): {err}")
        if arena is not None and not parity.reward_close(r["reward"], float(rew), o.beta, len(o.jobs)):
            raise parity.Mismatch(f"{where}: reward {r['reward']!r} != {rew!r}")
        over = bool(term) or info["wall_time"] >= limit
    if arena is not None and complete and not over:
        raise parity.Mismatch(f"env{env}: {ns} samples recorded, the reference episode goes on (wall {o.wall_time!r}, "
                              f"limit {limit!r})")
    return rows, over


def _report(rows: list[dict], over: list[bool]) -> dict:
    rep = {key: np.array([r[key] for r in rows]) for key in rows[0]} if rows else {}
    rep["episode_over"] = list(over)
    rep["plan_counts"] = {p: int((rep["plan"] == p).sum()) if rows else 0 for p in ("lds", "global")}
    rep["exec_path_counts"] = {p: int((rep["exec_path"] == p).sum()) if rows else 0 for p in ("spec", "many", "single")}
    if rows:
        d = rep["decisive"]
        rep["decisions"] = len(rows)
        rep["decisive_share"] = float(d.mean())
        rep["decisive_exec_nonzero"] = int((d & (rep["e_win"] > 0)).sum())      # exec winner k > 0
        rep["decisive_stage_nonfirst"] = int((d & (rep["s_win"] > 0)).sum())    # not the first schedulable stage
    return rep


def audit(arena, env_cfg: dict, dataset, seeds, limits, sd: dict, plan_cap: int = 0, helper: bool = False,
          complete=True, envs=None) -> dict:
    """Audits a filled sample arena (host copies: host_arena) of ONE greedy collection that started with
    reset(seeds[e], limits[e]); `sd`: the policy's state_dict, fp32 on the CPU. Every sample of every env goes through
    every check of the module docstring; parity.Mismatch on the first failure. `complete`: a bool, or one per env
    (an env stopped by the launch's max_steps has not ended its episode). Returns the per-sample arrays env, k, nodes,
    dags, sched, cap, plan, exec_path (decima_audit.classify), stage_idx, exec_idx, job_idx, lgprob, decisive, s_win,
    e_win, and plan_counts, exec_path_counts, decisions, decisive_share, decisive_exec_nonzero,
    decisive_stage_nonfirst."""
    B = arena.cursor.shape[0]
    rows, over = [], []
    for e in (range(B) if envs is None else envs):
        done = complete if isinstance(complete, bool) else bool(complete[e])
        r, ov = _walk_env(env_cfg, dataset, e, seeds[e], None if limits is None else limits[e], sd, arena, plan_cap,
                          helper, done, 0)
        rows += r
        over.append(ov)
    return _report(rows, over)


def reference_rollout(env_cfg: dict, dataset, seeds, limits, sd: dict, plan_cap: int = 0, helper: bool = False,
                      max_decisions: int = 10**9) -> dict:
    """The collection a correct greedy kernel records, without an engine: per env the oracle from
    reset(seeds[e], limits[e]) with the oracle's own arg-max actions, until the episode ends or max_decisions."""
    rows, over = [], []
    for e in range(len(seeds)):
        r, ov = _walk_env(env_cfg, dataset, e, seeds[e], None if limits is None else limits[e], sd, None, plan_cap,
                          helper, True, max_decisions)
        rows += r
        over.append(ov)
    return _report(rows, over)


def collect_reference(eng, arena, seeds, limits, sd: dict):
    """decima_audit.collect_reference with the oracle's ARG-MAX actions: one collection on the host build of the
    engine into the CPU DecimaSampleArena `arena`, the way the greedy kernel runs it."""
    from spark_sched_sim.engine import decima_obs_dict

    B, N = eng.num_envs, eng.layout.num_executors
    limits = [float("inf") if x is None else float(x) for x in (limits if limits is not None else [None] * B)]
    eng.reset(seeds=[int(s) for s in seeds], options=[{"time_limit": x} for x in limits])
    live = [True] * B
    k = 0
    while any(live):
        v = eng.host_views()
        f = eng.decima_features_np()
        si, ne = np.full(B, -1, dtype=np.int32), np.ones(B, dtype=np.int32)
        for e in range(B):
            if not live[e]:
                continue
            c = v["counts"][e]
            need = [int(arena.cursor[e, 0]) + 1, int(arena.cursor[e, 1]) + int(c[_abi.OC_NUM_NODES]),
                    int(arena.cursor[e, 2]) + int(c[_abi.OC_NUM_EDGES]),
                    int(arena.cursor[e, 3]) + int(c[_abi.OC_NUM_JOBS])]
            if any(n > cap for n, cap in zip(need, arena.caps)):  # the kernel's full flag and needs
                arena.cursor[e, _abi.CUR_FULL] = 1
                arena.cursor[e, _abi.CUR_NEED_NODES] = int(c[_abi.OC_NUM_NODES])
                arena.cursor[e, _abi.CUR_NEED_EDGES] = int(c[_abi.OC_NUM_EDGES])
                arena.cursor[e, _abi.CUR_NEED_DAGS] = int(c[_abi.OC_NUM_JOBS])
                arena.grow(arena.cursor.numpy())
            cs = int(arena.cursor[e, 0])
            fill_arena_like_kernel(arena, e, v, f)
            p = greedy_policy(sd, decima_obs_dict(v, f, e, N), N)
            si[e], ne[e] = p.s_win, p.e_win + 1
            words = arena.rec[e, cs]
            words[I32["stage_idx"]], words[I32["job_idx"]] = p.s_win, p.job
            words[I32["exec_idx"]], words[I32["num_exec"]] = p.e_win, p.e_win + 1
            words.view(torch.float32)[_abi.SAMPLE_LGPROB] = _lgprob(p, p.s_win, p.e_win)
            words.view(torch.float64)[_abi.SAMPLE_WALL] = float(v["wall_time"][e])
        eng.step(si, ne)
        v = eng.host_views()
        for e in range(B):
            if not live[e]:
                continue
            c = v["counts"][e]
            assert int(c[_abi.OC_ERR]) == 0, f"env{e} decision {k}: engine error bits {int(c[_abi.OC_ERR]):#x}"
            cs = int(arena.cursor[e, 0])
            arena.rec[e, cs - 1].view(torch.float64)[_abi.SAMPLE_REWARD] = float(v["reward"][e])
            live[e] = not (bool(c[_abi.OC_TERMINATED]) or float(v["wall_time"][e]) >= limits[e])
        k += 1
    return arena
