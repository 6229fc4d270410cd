"""TEST INFRASTRUCTURE ONLY — audits a filled sample arena of the persistent Decima rollout (ssim_decima_rollout,
csrc/decima_rollout.h), sampled or greedy (SSIM_ROLLOUT_GREEDY, csrc/decima_policy.h kGreedy), against the CPU oracle:
the env (oracle/restatement.py), the Decima observation wrapper (oracle/decima.py), the per-observation fp32 GNN policy
(oracle/decima_gnn.py) and a numpy restatement of the device sampling stream (csrc/policy.h splitmix64,
csrc/decima_policy.h dp_gumbel).

The replay tests show the engine is right GIVEN the rollout's actions; this module checks what the rollout computed
to choose them. ONE walk (_walk_env) drives the oracle through an arena's samples and checks every recorded
observation row, wall time, reward, the record's consistency and the log-probability of the recorded action; a CHOICE
RULE supplies only what differs between the two kinds of rollout:

  Sampled  the oracle's scores plus the device stream's Gumbel noise; the Gumbel-max winner must be the recorded choice
           wherever it leads the runner-up by more than the score margin, draws inside the margin are SKIPPED and
           counted (more than MAX_SKIP_SHARE of them fails); the policy checks run on every `every`-th sample.
  Greedy   no noise, and REGRET instead of skipping: with the noise at zero the skipping rule skips too much (2.7-3.3%
           of an untrained policy's decisions lie inside the margin, up to 96% once the tanh layers saturate). Every
           recorded choice must be numerically indistinguishable from the best: ss[stage_idx] >= max(ss) - s_margin and
           es[exec_idx] >= max(es) - e_margin, on every sample. Where the oracle's winner leads by more than the margin
           this forces the recorded choice to be the winner; elsewhere it accepts only choices within the margin of the
           best. A decision is DECISIVE when both leads exceed their margins.

The margins are 2 (SCORE_ATOL + SCORE_RTOL max|score|), per score vector.

  gumbel_np           the device's Gumbel noise for (seed, env, counter, item), stage or exec draw
  host_arena          numpy copies of a DecimaSampleArena (any device)
  sample_observation  the reference-format Decima observation of one recorded sample
  policy              the oracle's scores of one observation, winners (arg-max, first maximal index), leads and margins
  audit               the checks, per env; raises parity.Mismatch, returns per-sample sizes and path classes
  reference_rollout   the same walk with the reference's own winners as actions (what a correct kernel records)
  collect_reference   a sample arena filled on the host build of the engine, actions from the oracle policy
Helpers of the tests that use the auditor: policy_state, replanned, gpu_collect, arenas_equal.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import parity
from oracle import decima_gnn as G
from oracle.decima import decima_observation
from oracle.restatement import SparkSchedOracle
from spark_sched_sim import _abi
from spark_sched_sim.engine import GraphInstance

M64 = (1 << 64) - 1
EXEC_DRAW_KEY = 0xE7037ED1A0B428DB  # decima_policy.h: the exec draw's key is the decision's key ^ this
LGPROB_ATOL = LGPROB_RTOL = 1e-4    # cases.case_decima_fused's bar for the fused kernel's log-probability
SCORE_ATOL, SCORE_RTOL = 1e-5, 1e-4  # cases.case_decima_fused's bar per score
MAX_SKIP_SHARE = 0.02
LDS_PLAN_DAGS = 16   # decima_policy.h kDpLdsDags
HELP_WAVES, SPEC_CAND, TILE = 4, 3, 16  # decima_policy.h kDpHelpWaves, kDpSpecCand, rows per exec-score tile
I32 = {name: i for i, name in enumerate(_abi.SAMPLE_I32)}


# ------------------------------------------------------------------------------------------ the sampling stream
def _splitmix64(x: int) -> int:
    """policy.h:17 on a python int."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _splitmix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def decision_key(seed: int, env: int, counter: int) -> int:
    """decima_policy.h:780: key = splitmix64(seed ^ splitmix64(eid * 0x9E3779B97F4A7C15 + counter))."""
    return _splitmix64((seed & M64) ^ _splitmix64((env * 0x9E3779B97F4A7C15 + counter) & M64))


def gumbel_np(seed: int, env: int, counter: int, items, exec_draw: bool = False) -> np.ndarray:
    """dp_gumbel(key, item) for every item (node index for the stage draw, exec action k for the exec draw), as float32:
    r = splitmix64(key ^ splitmix64(item + 0x632BE59BD9B4E019)), u = ((r >> 11) + 0.5) / 2^53, -log(-log(u)) in float64,
    rounded to float32. `counter` is the launch's counter plus the decision's index in its episode."""
    key = decision_key(seed, env, counter) ^ (EXEC_DRAW_KEY if exec_draw else 0)
    it = np.asarray(items, dtype=np.uint64).reshape(-1)
    with np.errstate(over="ignore"):
        r = _splitmix64_np(np.uint64(key) ^ _splitmix64_np(it + np.uint64(0x632BE59BD9B4E019)))
    u = ((r >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    return (-np.log(-np.log(u))).astype(np.float32)


# ------------------------------------------------------------------------------------------ arena access
def host_arena(arena) -> SimpleNamespace:
    """Host (numpy) copies of a DecimaSampleArena's cursor, records and node / edge / DAG rows."""
    def np_(t):
        return t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.array(t)

    return SimpleNamespace(cursor=np_(arena.cursor), rec=np_(arena.rec), nodes=np_(arena.nodes),
                           edges=np_(arena.edges), dags=np_(arena.dags))


def sample_record(arena, env: int, k: int) -> dict:
    """Sample k of env as a dict: the int32 fields (_abi.SAMPLE_I32), lgprob, wall_before, reward."""
    words = np.ascontiguousarray(arena.rec[env, k])
    r = {name: int(words[i]) for name, i in I32.items()}
    r["lgprob"] = float(words.view(np.float32)[_abi.SAMPLE_LGPROB])
    r["wall_before"] = float(words.view(np.float64)[_abi.SAMPLE_WALL])
    r["reward"] = float(words.view(np.float64)[_abi.SAMPLE_REWARD])
    return r


def sample_observation(arena, env: int, k: int, num_executors: int) -> dict:
    """The reference-format Decima observation (schedulers/decima/env_wrapper.py:98-104) of sample k of env, from
    its arena rows, as engine.decima_obs_dict builds it from the obs arena and the feature arrays."""
    r = sample_record(arena, env, k)
    n, ne, nj, depth = r["num_nodes"], r["num_edges"], r["num_dags"], r["depth"]
    rows = np.array(arena.nodes[env, r["node_off"]: r["node_off"] + n], dtype=np.float32).reshape(n, 6)
    ed = np.asarray(arena.edges[env, r["edge_off"]: r["edge_off"] + ne]).reshape(ne, 4)
    dg = np.asarray(arena.dags[env, r["dag_off"]: r["dag_off"] + nj]).reshape(nj, 2)
    words = ed[:, 2].astype(np.int64).astype(np.uint32)
    levels = np.arange(max(depth - 1, 0), dtype=np.uint32)
    return {
        "dag_batch": GraphInstance(np.ascontiguousarray(rows[:, :5]), np.zeros(ne, dtype=np.int64),
                                   ed[:, :2].astype(np.int64).reshape(ne, 2)),
        "dag_ptr": [0] + [int(x) for x in np.cumsum(dg[:, 0].astype(np.int64))],
        "stage_mask": rows[:, 5] != 0,
        "exec_mask": np.arange(num_executors)[None, :] < dg[:, 1].astype(np.int64)[:, None],
        "edge_masks": ((words[None, :] >> levels[:, None]) & 1).astype(bool),
    }


# ------------------------------------------------------------------------------------------ path classification
def classify(dobs: dict, job_idx: int, num_executors: int, plan_cap: int, helper: bool) -> tuple[str, str]:
    """Which paths of the rollout a decision on this observation takes, from the observation alone.
    plan (decima_rollout.h:193): "lds" if n <= plan_cap and nj <= 16, else "global".
    exec_path, helper units only (decima_policy.h:803-824 and :923; "" otherwise): with at most 64 schedulable nodes,
    the distinct DAGs of the schedulable nodes in node order; "spec" if they are at most 3 and their caps, clamped to
    [0, N], need 1..3 tiles of 16 exec actions in all; else "many" if the chosen DAG's cap exceeds 16, else "single"."""
    n = dobs["stage_mask"].shape[0]
    ptr = np.asarray(dobs["dag_ptr"], dtype=np.int64)
    nj = len(ptr) - 1
    plan = "lds" if n <= plan_cap and nj <= LDS_PLAN_DAGS else "global"
    if not helper:
        return plan, ""
    caps = np.clip(np.asarray(dobs["exec_mask"], dtype=bool).sum(axis=1), 0, num_executors)
    sched = np.flatnonzero(dobs["stage_mask"])
    spec = False
    if len(sched) <= 64:
        dags, tiles, over = [], 0, False
        for g in np.searchsorted(ptr, sched, side="right") - 1:
            if g in dags:
                continue
            if len(dags) == SPEC_CAND:
                over = True
                break
            dags.append(int(g))
            tiles += (int(caps[g]) + TILE - 1) // TILE
        spec = not over and 0 < tiles < HELP_WAVES
    if spec:
        return plan, "spec"
    return plan, "many" if int(caps[job_idx]) > TILE else "single"


# ------------------------------------------------------------------------------------------ scores and choice rules
def _lead(x: np.ndarray, win: int) -> float:
    return float(x[win] - np.partition(x, -2)[-2]) if x.size > 1 else np.inf


def policy(sd: dict, dobs: dict, num_executors: int, stage_of=None, noise=None, dtype=torch.float32) -> SimpleNamespace:
    """The oracle policy on one observation: stage scores `ss` over the schedulable stages, their winner (arg-max,
    first maximal index) and its lead over the runner-up; then, for the DAG of stage `stage_of` (default: the winner),
    the same for the exec scores `es`. Scores are the oracle's at `dtype` (float32, or float64 for the cases with a
    derived lgprob bar). `noise(items, exec_draw)`, if given, is added to them in float32 as the kernel adds it, before
    winners and leads are taken (a rule's `noise`)."""
    enc = G.encode(sd, dobs, dtype=dtype)
    ss = G.stage_scores(sd, dobs, enc, dtype=dtype)
    s = ss.numpy().astype(np.float32)
    if noise is not None:
        s = s + noise(np.flatnonzero(np.asarray(dobs["stage_mask"], dtype=bool)), False)
    s_win = int(np.argmax(s))
    job = G.job_of_stage(dobs, s_win if stage_of is None else stage_of)
    es = G.exec_scores(sd, dobs, enc, job, num_executors, dtype=dtype)
    e = es.numpy().astype(np.float32)
    if noise is not None:
        e = e + noise(np.arange(es.numel()), True)
    e_win = int(np.argmax(e)) if e.size else 0
    p = SimpleNamespace(ss=ss, es=es, job=job, s_win=s_win, s_lead=_lead(s, s_win), e_win=e_win, e_lead=_lead(e, e_win),
                        s_margin=2.0 * (SCORE_ATOL + SCORE_RTOL * float(ss.abs().max())),
                        e_margin=2.0 * (SCORE_ATOL + SCORE_RTOL * float(es.abs().max())) if es.numel() else 0.0)
    p.decisive = bool(p.s_lead > p.s_margin and p.e_lead > p.e_margin)
    return p


def _lgprob(p, si: int, ei: int) -> float:
    return float(torch.log_softmax(p.ss, 0)[si] + torch.log_softmax(p.es, 0)[ei])


class Sampled:
    """The sampled rollout's rule for the launch parameters (seed, counter): Gumbel-max draws of the device stream,
    policy checks on every `every`-th sample. stage_key_exec: the stage draw keyed with the exec draw's constant (a
    wrong stream: the mutation test)."""

    def __init__(self, seed: int, counter: int, every: int = 1, stage_key_exec: bool = False):
        self.seed, self.counter, self.every, self.stage_key_exec = seed, counter, every, stage_key_exec

    def noise(self, env: int, k: int):
        return lambda items, exec_draw: gumbel_np(self.seed, env, (self.counter + k) & M64, items,
                                                  exec_draw=exec_draw or self.stage_key_exec)

    def checks(self, k: int) -> bool:
        return k % self.every == 0

    @staticmethod
    def check_choice(where: str, p, si: int, ei: int) -> None:
        if p.s_lead > p.s_margin and p.s_win != si:
            raise parity.Mismatch(f"{where}: stage draw: recorded {si}, the reference's Gumbel-max winner is "
                                  f"{p.s_win} by {p.s_lead:.3e} (margin {p.s_margin:.3e})")
        if p.e_lead > p.e_margin and p.e_win != ei:
            raise parity.Mismatch(f"{where}: exec draw: recorded {ei}, the reference's Gumbel-max winner is "
                                  f"{p.e_win} by {p.e_lead:.3e} (margin {p.e_margin:.3e})")

    @staticmethod
    def columns(p) -> dict:
        """`p`: the sample's scores, None where the policy checks skipped the sample."""
        return dict(audited=p is not None, skipped=p is not None and not p.decisive)

    @staticmethod
    def summarise(rep: dict, rows: int, what: str) -> None:
        aud = int(rep["audited"].sum()) if rows else 0
        skp = int((rep["audited"] & rep["skipped"]).sum()) if rows else 0
        rep["audited_draws"], rep["skipped_draws"] = aud, skp
        rep["skip_share"] = skp / aud if aud else 0.0
        if rep["skip_share"] > MAX_SKIP_SHARE:
            raise parity.Mismatch(f"{what}: {skp} of {aud} audited draws inside the score margin "
                                  f"({rep['skip_share']:.1%} > {MAX_SKIP_SHARE:.0%})")


class Greedy:
    """The greedy rollout's rule: no noise, every sample checked, the recorded choice within the margin of the best."""

    @staticmethod
    def noise(env: int, k: int):
        return None

    @staticmethod
    def checks(k: int) -> bool:
        return True

    @staticmethod
    def check_choice(where: str, p, si: int, ei: int) -> None:
        s_best, s_got = float(p.ss.max()), float(p.ss[si])
        if not s_got >= s_best - p.s_margin:
            raise parity.Mismatch(f"{where}: stage choice: recorded {si} scores {s_got!r}, the oracle's best ("
                                  f"{p.s_win}) {s_best!r}: regret {s_best - s_got:.3e} > margin {p.s_margin:.3e}")
        e_best, e_got = float(p.es.max()), float(p.es[ei])
        if not e_got >= e_best - p.e_margin:
            raise parity.Mismatch(f"{where}: exec choice: recorded {ei} scores {e_got!r}, the oracle's best ("
                                  f"{p.e_win}) {e_best!r}: regret {e_best - e_got:.3e} > margin {p.e_margin:.3e}")

    @staticmethod
    def columns(p) -> dict:
        return dict(decisive=p.decisive, s_win=p.s_win, e_win=p.e_win)

    @staticmethod
    def summarise(rep: dict, rows: int, what: str) -> None:
        if rows:
            d = rep["decisive"]
            rep["decisions"] = rows
            rep["decisive_share"] = float(d.mean())
            rep["decisive_exec_nonzero"] = int((d & (rep["e_win"] > 0)).sum())      # exec winner k > 0
            rep["decisive_stage_nonfirst"] = int((d & (rep["s_win"] > 0)).sum())    # not the first schedulable stage


# ------------------------------------------------------------------------------------------ the walk
def lgprob_bar_of(want: float, lgprob_bar=None) -> float:
    """The bar on a recorded lgprob: 1e-4 + 1e-4 |want|, or the case's derived absolute bar where that is smaller."""
    std = LGPROB_ATOL + LGPROB_RTOL * abs(want)
    return std if lgprob_bar is None else min(std, lgprob_bar)


def _walk_env(env_cfg, dataset, env, env_seed, limit, sd, rule, arena, plan_cap, helper, complete, max_decisions,
              ref):
    """One env: the oracle from reset(env_seed, limit) through the recorded samples (arena given: every check of
    `audit`), or through the reference's own winners under `rule` (arena None), at most max_decisions of them.
    `ref`: the oracle's dtype, the derived lgprob bar (or None) and `observe` (or None), called with (env, k, the
    Decima observation, stage_idx, exec_idx) of every decision. Returns the per-sample rows of the report and whether
    the oracle's episode is over."""
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
            # record consistency
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
            si, ei, lg = r["stage_idx"], r["exec_idx"], r["lgprob"]
        p = None
        if arena is None:
            p = policy(sd, dobs, N, noise=rule.noise(env, k), dtype=ref.dtype)
            si, ei, job = p.s_win, p.e_win, p.job
            cap = int(dobs["commit_caps"][job])
            lg = _lgprob(p, si, ei)
        elif rule.checks(k):
            p = policy(sd, dobs, N, stage_of=si, noise=rule.noise(env, k), dtype=ref.dtype)
            rule.check_choice(where, p, si, ei)
            want = _lgprob(p, si, ei)
            bar = lgprob_bar_of(want, ref.lgprob_bar)
            if not abs(lg - want) <= bar:
                raise parity.Mismatch(f"{where}: lgprob {lg!r} vs oracle {want!r} (diff {abs(lg - want):.3e}, bar "
                                      f"{bar:.3e})")
        if ref.observe is not None:
            ref.observe(env, k, dobs, int(si), int(ei))
        plan, exec_path = classify(dobs, job, N, plan_cap, helper)
        rows.append(dict(env=env, k=k, nodes=int(dobs["stage_mask"].shape[0]), dags=len(dobs["dag_ptr"]) - 1,
                         sched=nsch, cap=cap, plan=plan, exec_path=exec_path, stage_idx=si, exec_idx=ei, job_idx=job,
                         lgprob=lg, **rule.columns(p)))
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


def _walk(envs, env_cfg, dataset, seeds, limits, sd, rule, arena, plan_cap, helper, complete, max_decisions, what,
          dtype=torch.float32, lgprob_bar=None, observe=None):
    ref = SimpleNamespace(dtype=dtype, lgprob_bar=lgprob_bar, observe=observe)
    rows, over = [], []
    for e in envs:
        done = complete if isinstance(complete, bool) else bool(complete[e])
        r, ov = _walk_env(env_cfg, dataset, e, seeds[e], None if limits is None else limits[e], sd, rule, arena,
                          plan_cap, helper, done, max_decisions, ref)
        rows += r
        over.append(ov)
    rep = {key: np.array([r[key] for r in rows]) for key in rows[0]} if rows else {}
    rep["episode_over"] = over
    rep["plan_counts"] = {p: int((rep["plan"] == p).sum()) if rows else 0 for p in ("lds", "global")}
    rep["exec_path_counts"] = {p: int((rep["exec_path"] == p).sum()) if rows else 0 for p in ("spec", "many", "single")}
    rule.summarise(rep, len(rows), what)
    return rep


def audit(arena, env_cfg: dict, dataset, seeds, limits, sd: dict, rule, plan_cap: int = 0, helper: bool = False,
          complete=True, envs=None, **ref) -> dict:
    """Audits a filled sample arena (host copies: host_arena) of ONE collection (no auto-reset) that started with
    reset(seeds[e], limits[e]) and ran under `rule` (Sampled with the launch's seed and counter, or Greedy); `sd`: the
    policy's state_dict, fp32 on the CPU. Per env, raising parity.Mismatch on the first failure:

    Env and features, every sample: a SparkSchedOracle is driven through the recorded (stage_idx, num_exec); before each
    step its Decima observation equals sample_observation under parity.compare_decima (float32 features bit for bit,
    links, dag_ptr and the three masks equal), wall_before equals the oracle's wall time bit for bit, the reward passes
    parity.reward_close; after the last sample the oracle's episode is over (`complete`: a bool, or one per env; an
    env stopped by the launch's max_steps has not ended its episode).
    Record consistency, every sample: num_exec == exec_idx + 1, 0 <= exec_idx < the job's commit cap, job_idx the DAG of
    the stage, the row offsets the running sums of the earlier samples' counts, depth the oracle's edge-mask levels.
    Policy value, every sample the rule checks: lgprob within 1e-4 + 1e-4 |want| of log_softmax(stage scores)[stage_idx]
    + log_softmax(exec scores)[exec_idx] of oracle/decima_gnn.py. `ref`: dtype=torch.float64 takes the oracle in double,
    lgprob_bar=x an absolute bar x wherever it is below the standing one (the cases with a bar derived from the
    reference, tests/policy_strength.py), observe=f is called with (env, k, observation, stage_idx, exec_idx).
    Choice, the same samples. Sampled: the Gumbel-max winners of the oracle's scores plus gumbel_np equal the recorded
    choices wherever the winner leads the runner-up by more than 2 * (1e-5 + 1e-4 max|score|); decisions inside that
    margin are skipped and counted, more than 2% skipped fails. Greedy: the recorded stage's and exec action's scores
    are within that margin of the best.

    Returns the per-sample arrays env, k, nodes, dags, sched, cap (commit cap of the chosen job), plan, exec_path
    (classify), stage_idx, exec_idx, job_idx, lgprob, and episode_over (per env), plan_counts, exec_path_counts; under
    Sampled also audited, skipped and audited_draws, skipped_draws, skip_share; under Greedy decisive, s_win, e_win and
    decisions, decisive_share, decisive_exec_nonzero, decisive_stage_nonfirst."""
    return _walk(range(arena.cursor.shape[0]) if envs is None else envs, env_cfg, dataset, seeds, limits, sd, rule,
                 arena, plan_cap, helper, complete, 0, "audit", **ref)


def reference_rollout(env_cfg: dict, dataset, seeds, limits, sd: dict, rule, plan_cap: int = 0, helper: bool = False,
                      max_decisions: int = 10**9, **ref) -> dict:
    """The collection a correct kernel records, without an engine: per env the oracle from reset(seeds[e], limits[e])
    with the reference's own winners under `rule` as actions, until the episode ends or max_decisions. The report of
    `audit` (every decision counts as audited). `ref`: dtype and observe, as in `audit`."""
    return _walk(range(len(seeds)), env_cfg, dataset, seeds, limits, sd, rule, None, plan_cap, helper, True,
                 max_decisions, "reference rollout", **ref)


# ------------------------------------------------------------------------------------------ a host-filled arena
def fill_arena_like_kernel(arena, e, v, f):
    """What csrc/decima_rollout.h DecimaPolicy.act writes for env e's current observation (host views v, host
    features f): the node / edge / DAG rows after the env's cursor, and the record (action fields left 0)."""
    c = v["counts"][e]
    n, ne, nj = int(c[_abi.OC_NUM_NODES]), int(c[_abi.OC_NUM_EDGES]), int(c[_abi.OC_NUM_JOBS])
    cur = arena.cursor[e]
    cs, cn, ce, cg = (int(x) for x in cur[:4])
    arena.nodes[e, cn:cn + n, :5] = torch.from_numpy(np.asarray(f["node_feats"][e, :n]))
    arena.nodes[e, cn:cn + n, 5] = torch.from_numpy(np.asarray(v["nodes"][e, :n, 2]))
    links = np.asarray(v["edge_links"][e, :ne], dtype=np.int64)
    arena.edges[e, ce:ce + ne, 0] = torch.from_numpy(links[:, 0].astype(np.int32))
    arena.edges[e, ce:ce + ne, 1] = torch.from_numpy(links[:, 1].astype(np.int32))
    arena.edges[e, ce:ce + ne, 2] = torch.from_numpy(np.asarray(f["edge_mask"][e, :ne]).astype(np.int32))
    ptr = np.asarray(v["dag_ptr"][e, : nj + 1], dtype=np.int64)
    arena.dags[e, cg:cg + nj, 0] = torch.from_numpy((ptr[1:] - ptr[:-1]).astype(np.int32))
    arena.dags[e, cg:cg + nj, 1] = torch.from_numpy(np.asarray(f["commit_cap"][e, :nj]).astype(np.int32))
    rec = torch.zeros(16, dtype=torch.int32)
    rec[:7] = torch.tensor([n, ne, nj, int(f["depth"][e]), cn, ce, cg], dtype=torch.int32)
    arena.rec[e, cs] = rec
    cur[:4] = torch.tensor([cs + 1, cn + n, ce + ne, cg + nj], dtype=torch.int32)


def record_like_kernel(arena, e, v, f) -> list[int]:
    """Env e's current observation into the CPU arena the way the kernel and its host do it: where a region cannot
    hold it, the kernel's full flag and needs (DecimaPolicy can_act) and the host's growth; then the rows and the
    record (fill_arena_like_kernel). Returns what the observation needed per region (samples, nodes, edges, DAGs)."""
    c = v["counts"][e]
    obs = [1, int(c[_abi.OC_NUM_NODES]), int(c[_abi.OC_NUM_EDGES]), int(c[_abi.OC_NUM_JOBS])]
    need = [int(arena.cursor[e, i]) + obs[i] for i in range(4)]
    if any(n > cap for n, cap in zip(need, arena.caps)):
        arena.cursor[e, _abi.CUR_FULL] = 1
        arena.cursor[e, _abi.CUR_NEED_NODES] = obs[1]
        arena.cursor[e, _abi.CUR_NEED_EDGES] = obs[2]
        arena.cursor[e, _abi.CUR_NEED_DAGS] = obs[3]
        arena.grow(arena.cursor.numpy())
    fill_arena_like_kernel(arena, e, v, f)
    return need


def collect_reference(eng, arena, seeds, limits, sd: dict, rule):
    """One collection on the host build of the engine (hostsim.driver.HostEngine `eng`) into the CPU DecimaSampleArena
    `arena`, the way the kernel runs it: per env reset(seeds[e], limits[e]), then until the episode ends (terminated,
    or wall time >= the limit) the observation rows (record_like_kernel, the arena grown when a region is full), the
    oracle policy's winner under `rule` (oracle/decima_gnn.py on the engine's observation and features; Sampled: drawn
    with gumbel_np on (seed, env, counter + decision index), Greedy: the arg-max), its oracle log-probability, the wall
    time, and after the step the reward."""
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
            record_like_kernel(arena, e, v, f)
            p = policy(sd, decima_obs_dict(v, f, e, N), N, noise=rule.noise(e, k))
            si[e], ne[e] = p.s_win, p.e_win + 1
            words = arena.rec[e, int(arena.cursor[e, 0]) - 1]
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


# ------------------------------------------------------------------------------------------ helpers of the tests
def policy_state(num_executors: int, device="cpu", *, seed: int, noise: float, gains=(1.0, 1.0)):
    """A test policy: DecimaScheduler's random init at torch.manual_seed(seed) plus noise * randn on every parameter
    (as cases.case_decima_policy, so biases matter), drawn on the CPU so the CPU and GPU tests hold the same weights.
    `gains` = (g_enc, g_pol) then multiply every encoder.* parameter by g_enc and every parameter of the two policy
    networks by g_pol: the "spread" sets of tests/policy_strength.py. Returns (module on `device`, its state_dict in
    fp32 on the CPU)."""
    from spark_sched_sim.schedulers.decima import DecimaScheduler

    torch.manual_seed(seed)
    pol = DecimaScheduler(num_executors)
    for p in pol.parameters():
        p.data.add_(noise * torch.randn_like(p))
    for name, p in pol.named_parameters():
        g = gains[0] if name.startswith("encoder.") else gains[1]
        if g != 1.0:
            p.data.mul_(g)
    sd = {k: v.detach().cpu().float().clone() for k, v in pol.state_dict().items()}
    return pol.to(device), sd


def replanned(rep: dict, plan_cap: int) -> dict:
    """A reference collection's report for a unit without helper waves and with another plan cap that takes the same
    trajectories (dr_hbm50 from dr_lds50)."""
    rep = dict(rep)
    rep["plan"] = np.where((rep["nodes"] <= plan_cap) & (rep["dags"] <= LDS_PLAN_DAGS), "lds", "global")
    rep["plan_counts"] = {p: int((rep["plan"] == p).sum()) for p in ("lds", "global")}
    rep["exec_path_counts"] = {p: 0 for p in ("spec", "many", "single")}
    return rep


def gpu_collect(eng, params, arena, seed: int, counter: int, max_steps=None, budget: int = 0, flags: int = 0):
    """One collection of the device engine `eng` into `arena`: a launch to the end of every episode, relaunched after
    each arena growth; with `budget`, launches of that many decisions under SSIM_ROLLOUT_PREEMPT until nothing is added
    or pending; with `max_steps`, ONE launch of at most that many decisions per env, the arena left as it is. No env
    may end with error bits. Returns launches, grown (arena growths) and full (the last launch filled the arena)."""
    launches = grown = 0
    full = False
    if max_steps is not None:
        eng.decima_rollout(params, seed, counter, max_steps, flags=flags, samples=arena)
        launches = 1
        full = bool((arena.cursor[:, _abi.CUR_FULL] != 0).any())
    elif not budget:  # (the collectors' loop)
        _, launches, grown = arena.launch_until_fits(
            lambda: eng.decima_rollout(params, seed, counter, 10**6, flags=flags, samples=arena))
    else:
        prev = -1
        while True:
            eng.decima_rollout(params, seed, counter, 64, budget, flags=flags | _abi.SSIM_ROLLOUT_PREEMPT,
                               samples=arena)
            launches += 1
            cur = arena.cursor.cpu().numpy()
            full = bool((cur[:, _abi.CUR_FULL] != 0).any())
            if full:
                arena.grow(cur)
                grown += 1
                continue
            n = int(cur[:, _abi.CUR_SAMPLES].sum())
            pend = int(np.count_nonzero(eng.views["counts"][:, _abi.OC_ERR].cpu().numpy() & _abi.SSIM_ERR_PENDING))
            if n == prev and pend == 0:
                break
            prev = n
    torch.cuda.synchronize()
    err = eng.views["counts"][:, _abi.OC_ERR].cpu().numpy()
    assert not err.any(), [hex(int(x)) for x in err]
    return SimpleNamespace(launches=launches, grown=grown, full=full)


def arenas_equal(a, b) -> None:
    """Two host arenas (host_arena) hold the same collection: the cursors, and per env the used prefixes of the
    records, node rows (as bit patterns), edge rows and DAG rows."""
    assert np.array_equal(a.cursor, b.cursor)
    for i in range(a.cursor.shape[0]):
        ns, nn, ne, nd = (int(x) for x in a.cursor[i, :4])
        assert np.array_equal(a.rec[i, :ns], b.rec[i, :ns]), f"env {i} records"
        assert np.array_equal(a.nodes[i, :nn].view(np.uint32), b.nodes[i, :nn].view(np.uint32)), f"env {i} nodes"
        assert np.array_equal(a.edges[i, :ne], b.edges[i, :ne]), f"env {i} edges"
        assert np.array_equal(a.dags[i, :nd], b.dags[i, :nd]), f"env {i} dags"
