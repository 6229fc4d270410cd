"""Cases of the shortest-job-first schedulers (SJF / SJF-CP), shared by the CPU tests of the host build
(test_priority_schedulers.py) and the device tests (test_gpu_priority.py, `-m gpu`).

The reference of every case is the CPU oracle driven by the host scheduler `ShortestJobFirstScheduler` (the
specification of the two kinds). `oracle_episode` runs it once per (config, scheduler, seed) and the cases share the
result: the action of every decision, counts of the decisions that exercise each branch of the rule, and the oracle
at the end of the run.
"""

import functools
from types import SimpleNamespace

import numpy as np

import cases
from oracle.restatement import SparkSchedOracle, avg_job_duration
from spark_sched_sim import _abi
from spark_sched_sim.schedulers import ShortestJobFirstScheduler, find_stage, host_scheduler

KINDS = {"sjf": _abi.SSIM_POLICY_SJF, "sjf-cp": _abi.SSIM_POLICY_SJF_CP}
DEFAULT_SEEDS = (77, 78)           # run to termination
OVERLOADED_SEEDS = (31, 32, 33, 34)  # 300 decisions each (the lockstep cases use the first two)
OVERLOADED_DECISIONS = 300
TRACE_CAP = 20000


def overloaded(env_cfg: dict) -> dict:
    """Few executors and a fast arrival stream: the active jobs pile up past 64 (the device's multi-chunk path),
    many are untouched copies of one template (work ties), and the shortest one is rarely the first."""
    return dict(env_cfg, num_executors=5, job_arrival_cap=100, job_arrival_rate=1e-3)


@functools.lru_cache(maxsize=None)
def datasets(key: str = "default"):
    """"default": the synthetic set of the suite (at most 18 stages per job: the engine reads a job's DAG from the
    topology bit sets). "wide<N>": the same with queries 3 and 7 replaced by N-stage DAGs; above 32 stages the engine
    (and the hot-block view of SJF-CP) walks the child lists instead, above 64 SJF-CP is refused."""
    from spark_sched_sim.data_samplers import synthetic_tpch as T

    data = dict(T.generate(0))
    if key != "default":
        n = int(key[len("wide"):])
        for q in (3, 7):
            rng = np.random.Generator(np.random.PCG64([99, q, n]))
            adj = T._random_dag(rng, n)
            tasks = rng.integers(1, 12, size=n)
            for si, size in enumerate(T.QUERY_SIZES):
                data[(q, size)] = (adj.copy(), {s: T._stage_durations(rng, int(tasks[s]), T._SIZE_DUR_SCALE[si])
                                                for s in range(n)})
    return data


@functools.lru_cache(maxsize=None)
def _episode(cfg_items, name, seed, max_decisions, ds_key):
    cfg = dict(cfg_items)
    sched = host_scheduler(name, cfg["num_executors"])
    o = SparkSchedOracle(cfg, datasets(ds_key))
    o.trace = []
    ob, _ = o.reset(seed=seed)
    actions = []
    n = SimpleNamespace(multi_chunk=0, work_ties=0, not_first=0, cp_differs=0, max_job_rows=0)
    term, rew = False, None
    while not term and len(actions) < max_decisions:
        a, _ = sched.schedule(ob)
        if isinstance(sched, ShortestJobFirstScheduler):  # (schedule() has run preprocess_obs on ob)
            w = sched.row_work(ob)
            cand = [k for k in range(len(ob["dag_ptr"]) - 1) if find_stage(ob, k) != -1]
            ks = sched.choose_job(ob, w)
            works = {k: sched.job_work(ob, w, k) for k in cand}
            n.multi_chunk += len(ob["dag_ptr"]) - 1 > 64
            n.work_ties += any(k != ks and works[k] == works[ks] for k in cand)
            n.not_first += ks != cand[0]
            n.cp_differs += a["stage_idx"] != find_stage(ob, ks)
        n.max_job_rows = max(n.max_job_rows, int(np.diff(ob["dag_ptr"]).max(initial=0)))
        actions.append((int(a["stage_idx"]), int(a["num_exec"])))
        ob, rew, term, _, _ = o.step({"stage_idx": actions[-1][0], "num_exec": actions[-1][1]})
    return SimpleNamespace(oracle=o, last_obs=ob, last_reward=rew, terminated=bool(term), counts=n,
                           actions=np.array(actions, dtype=np.int32).reshape(-1, 2),
                           avg_job_duration=float(avg_job_duration(o)) * 1e-3 if term else None,
                           completed=sum(1 for j in o.jobs.values() if np.isfinite(j.t_completed)))


def oracle_episode(cfg: dict, name: str, seed: int, max_decisions: int = 10**9, ds_key: str = "default"):
    """The oracle driven by host scheduler `name` from reset(seed) for `max_decisions` decisions or to termination, on
    `datasets(ds_key)`. Cached: the returned object is shared, never modified by a case."""
    return _episode(tuple(sorted(cfg.items())), name, int(seed), int(max_decisions), ds_key)


def check_coverage(name: str, is_overloaded: bool, ep) -> None:
    """The run exercises what it is there for (counts from the oracle run alone)."""
    n = ep.counts
    if is_overloaded:
        assert n.multi_chunk >= 200, f"decisions with more than 64 active jobs: {n.multi_chunk}"
        assert n.work_ties >= 5, f"decisions with a work tie: {n.work_ties}"
        assert n.not_first >= 250, f"chosen job is not the first candidate: {n.not_first}"
        if name == "sjf-cp":
            assert n.cp_differs >= 100, f"critical-path stage differs from find_stage: {n.cp_differs}"
    else:
        assert ep.terminated
        assert n.not_first >= 600, f"chosen job is not the first candidate: {n.not_first}"
        if name == "sjf-cp":
            assert n.cp_differs >= 500, f"critical-path stage differs from find_stage: {n.cp_differs}"
    if name == "sjf":
        assert n.cp_differs == 0


def _runs(env_cfg, name, is_overloaded, seeds):
    cfg = overloaded(env_cfg) if is_overloaded else dict(env_cfg)
    limit = OVERLOADED_DECISIONS if is_overloaded else 10**9
    eps = [oracle_episode(cfg, name, s, limit) for s in seeds]
    for ep in eps:
        check_coverage(name, is_overloaded, ep)
    return cfg, eps


def case_policy_lockstep(make, dataset, env_cfg, name, is_overloaded, seeds):
    """ssim_policy(kind) on the engine's observation equals the host scheduler's action on the oracle's, at every
    decision (the engine is stepped with the device's own action)."""
    cfg, eps = _runs(env_cfg, name, is_overloaded, seeds)
    B = len(seeds)
    eng = make(cfg, B, dataset, 0)
    eng.reset(seeds=list(seeds))
    steps = max(len(ep.actions) for ep in eps)
    for k in range(steps):
        si, ne = eng.policy(KINDS[name])
        si, ne = np.array(eng.to_numpy(si)), np.array(eng.to_numpy(ne))
        for i, ep in enumerate(eps):
            if k < len(ep.actions):
                assert (int(si[i]), int(ne[i])) == tuple(ep.actions[k]), f"{name} env{i} (seed {seeds[i]}) step{k}"
        eng.step(si, ne)
    c = eng.host_views()["counts"]
    for i, ep in enumerate(eps):
        assert int(c[i][_abi.OC_ERR]) == 0
        assert bool(c[i][_abi.OC_TERMINATED]) == ep.terminated
        if ep.terminated or len(ep.actions) == steps:
            assert int(c[i][_abi.OC_DECISIONS]) == len(ep.actions)
    return eps


def case_fused_rollout(make, dataset, env_cfg, name, is_overloaded, seeds):
    """One fused rollout launch: the logged action of every decision is the host scheduler's on the oracle, and the
    engine ends where the oracle does (final observation, wall time, reward, decision count, job times, event
    trace), for every env of the batch."""
    cfg, eps = _runs(env_cfg, name, is_overloaded, seeds)
    B = len(seeds)
    K = OVERLOADED_DECISIONS if is_overloaded else max(len(ep.actions) for ep in eps) + 8
    eng = make(cfg, B, dataset, TRACE_CAP)
    eng.reset(seeds=list(seeds))
    log = eng.alloc_action_log(K)
    eng.rollout(KINDS[name], 0, K, log)
    log = np.asarray(eng.to_numpy(log))
    v = eng.host_views()
    ta, tc, _ = eng.job_times_np()
    for i, ep in enumerate(eps):
        dec = int(v["counts"][i][_abi.OC_DECISIONS])
        m = min(dec, len(ep.actions))
        diff = np.flatnonzero((log[:m, i] != ep.actions[:m]).any(axis=1))
        assert diff.size == 0, (f"{name} env{i} (seed {seeds[i]}): first differing decision {int(diff[0])}: logged "
                                f"{log[diff[0], i].tolist()}, host scheduler {ep.actions[diff[0]].tolist()}")
        assert dec == len(ep.actions), f"{name} env{i}: {dec} decisions, oracle {len(ep.actions)}"
        assert bool(v["counts"][i][_abi.OC_TERMINATED]) == ep.terminated
        cases.check_replayed_env(eng, v, ta, tc, i, ep.oracle, ep.last_obs, 1, dec, ep.last_reward,
                                 f"{name} rollout", trace=True)
    return eng


def case_evaluate(name, env_cfg, dataset, seeds, **kwargs):
    """evaluate_policy equals the oracle driven by the host scheduler of the same name."""
    from spark_sched_sim.evaluate import evaluate_policy

    out = evaluate_policy(env_cfg, name, seeds, dataset=dataset, **kwargs)
    eps = [oracle_episode(env_cfg, name, s) for s in seeds]
    assert all(ep.terminated for ep in eps)
    np.testing.assert_allclose(out["avg_job_duration"], [ep.avg_job_duration for ep in eps], rtol=1e-12, atol=0.0)
    assert out["decisions"].tolist() == [len(ep.actions) for ep in eps]
    assert out["completed_jobs"].tolist() == [ep.completed for ep in eps]
    assert out["wall_time"].tolist() == [float(ep.oracle.wall_time) for ep in eps]
    return out


WIDE = "wide40"  # two 40-stage queries: past the 32 stages of the topology bit sets, within SJF-CP's 64
WIDE_SEEDS = (5, 6)


def wide_cfg(env_cfg: dict) -> dict:
    return dict(env_cfg, job_arrival_cap=16)


def case_wide_jobs(make, env_cfg, name):
    """Jobs of 40 stages: the child-list topology path of the hot-block view, through `policy(kind)` in lockstep and
    through a fused rollout, to termination."""
    cfg = wide_cfg(env_cfg)
    eps = [oracle_episode(cfg, name, s, ds_key=WIDE) for s in WIDE_SEEDS]
    assert all(ep.terminated for ep in eps)
    # (the engine picks the child-list path from the data set's widest template; the episodes also hold such jobs)
    assert max(ep.counts.max_job_rows for ep in eps) == 40
    for via_rollout in (False, True):
        eng = make(cfg, len(eps), datasets(WIDE), TRACE_CAP)
        eng.reset(seeds=list(WIDE_SEEDS))
        K = max(len(ep.actions) for ep in eps)
        if via_rollout:
            log = eng.alloc_action_log(K)
            eng.rollout(KINDS[name], 0, K, log)
            log = np.asarray(eng.to_numpy(log))
        else:
            log = np.zeros((K, len(eps), 2), dtype=np.int32)
            for k in range(K):
                si, ne = eng.policy(KINDS[name])
                log[k, :, 0], log[k, :, 1] = np.array(eng.to_numpy(si)), np.array(eng.to_numpy(ne))
                eng.step(si, ne)
        v = eng.host_views()
        ta, tc, _ = eng.job_times_np()
        for i, ep in enumerate(eps):
            n = len(ep.actions)
            diff = np.flatnonzero((log[:n, i] != ep.actions).any(axis=1))
            assert diff.size == 0, f"{name} env{i} rollout={via_rollout}: first differing decision {int(diff[0])}"
            cases.check_replayed_env(eng, v, ta, tc, i, ep.oracle, ep.last_obs, 1, n, ep.last_reward,
                                     f"{name} wide", trace=True)
