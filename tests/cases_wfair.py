"""Cases of the weighted-fair schedulers (WFair(alpha), policy kinds `_abi.wfair_kind(alpha)`), shared by the CPU tests
of the host build (test_weighted_fair.py) and the device tests (test_gpu_weighted_fair.py, `-m gpu`).

The reference of every case is the CPU oracle driven by the host scheduler `WeightedFairScheduler` (the specification
of the kinds). `oracle_episode` runs it once per (config, alpha2, seed) and the cases share the result: the action of
every decision, counts of the decisions that exercise each branch of the rule (from the oracle run alone), and the
oracle at the end of the run.
"""

import functools
from types import SimpleNamespace

import numpy as np

import cases
import cases_priority as P
from oracle.restatement import SparkSchedOracle, avg_job_duration
from spark_sched_sim import _abi
from spark_sched_sim.schedulers import RoundRobinScheduler, WeightedFairScheduler, find_stage

ALPHA2S = tuple(range(-4, 5))
NONZERO = tuple(a for a in ALPHA2S if a != 0)
DEFAULT_SEEDS = (77, 78)  # run to termination
BUSY_SEEDS = (31, 32)     # 400 decisions each
BUSY_DECISIONS = 400
BUSY_ALPHA2S = (-4, -2, -1, 1, 2, 4)
TRACE_CAP = 20000


def kind_of(alpha2: int) -> int:
    return _abi.SSIM_POLICY_WFAIR_BASE + alpha2 + 4


def busy(env_cfg: dict) -> dict:
    """Many executors and a fast arrival stream: the active jobs pile up past 64 (more than one block of the sum)
    while the caps stay well above 1, so the weights decide who is served."""
    return dict(env_cfg, num_executors=40, job_arrival_cap=150, job_arrival_rate=1e-2)


def _tuple(a: dict):
    return int(a["stage_idx"]), int(a["num_exec"])


@functools.lru_cache(maxsize=None)
def _episode(cfg_items, alpha2, seed, max_decisions, ds_key):
    cfg = dict(cfg_items)
    N = cfg["num_executors"]
    sched = WeightedFairScheduler(N, alpha=alpha2 / 2)
    fair = RoundRobinScheduler(N)
    o = SparkSchedOracle(cfg, P.datasets(ds_key))
    o.trace = []
    ob, _ = o.reset(seed=seed)
    actions = []
    n = SimpleNamespace(differs=0, cap_binds=0, skipped=0, multi_block=0, first_block_differs=0, max_job_rows=0,
                        zero_work=0)
    term, rew = False, None
    while not term and len(actions) < max_decisions:
        a, _ = sched.schedule(ob)
        act = _tuple(a)
        # (schedule() has run preprocess_obs on ob) what the run exercises, from the observation and the rule's parts
        nj, src, sup = len(ob["exec_supplies"]), ob["source_job_idx"], ob["exec_supplies"]
        n.differs += act != _tuple(fair.schedule(ob)[0])
        n.multi_block += nj > 64
        n.max_job_rows = max(n.max_job_rows, int(np.diff(ob["dag_ptr"]).max(initial=0)))
        if not (src < nj and find_stage(ob, src) != -1):
            p = sched.weights(ob)
            total = sched.total(p)
            n.zero_work += any(float(x) == 0.0 for x in p)
            if total > 0.0:
                for k in range(nj):  # the walk of the rule: jobs passed over at their cap, and a cap that binds
                    if k == src:
                        continue
                    cap, s = sched.cap(p[k], total), find_stage(ob, k)
                    if sup[k] >= cap:
                        n.skipped += s != -1
                    elif s != -1:
                        n.cap_binds += cap - sup[k] < ob["num_committable_execs"]
                        break
                if nj > 64:
                    n.first_block_differs += _tuple(sched.other_jobs(ob, p, sched.total(p[:64]))) != act
        actions.append(act)
        ob, rew, term, _, _ = o.step({"stage_idx": act[0], "num_exec": act[1]})
    return SimpleNamespace(oracle=o, last_obs=ob, last_reward=rew, terminated=bool(term), counts=n,
                           actions=np.array(actions, dtype=np.int32).reshape(-1, 2),
                           avg_job_duration=float(avg_job_duration(o)) * 1e-3 if term else None,
                           completed=sum(1 for j in o.jobs.values() if np.isfinite(j.t_completed)))


def oracle_episode(cfg: dict, alpha2: int, seed: int, max_decisions: int = 10**9, ds_key: str = "default"):
    """The oracle driven by WeightedFairScheduler(alpha2 / 2) from reset(seed) for `max_decisions` decisions or to
    termination, on `cases_priority.datasets(ds_key)`. Cached: the returned object is shared, never modified."""
    return _episode(tuple(sorted(cfg.items())), int(alpha2), int(seed), int(max_decisions), ds_key)


def check_coverage(alpha2: int, is_busy: bool, ep) -> None:
    """The run exercises what it is there for (counts from the oracle run alone)."""
    n = ep.counts
    if is_busy:
        assert n.multi_block >= 300, f"decisions with more than 64 active jobs: {n.multi_block}"
        assert n.first_block_differs >= 10, f"actions that change with P over the first 64 jobs: {n.first_block_differs}"
    elif alpha2 != 0:
        assert ep.terminated
        assert n.differs >= 30, f"decisions that differ from fair's: {n.differs}"
        assert n.cap_binds >= 10, f"decisions where the cap binds: {n.cap_binds}"
        assert n.skipped >= 50, f"jobs skipped at their cap with a schedulable stage: {n.skipped}"
    else:
        assert ep.terminated and n.differs == 0


def runs(env_cfg, alpha2, is_busy, seeds):
    cfg = busy(env_cfg) if is_busy else dict(env_cfg)
    limit = BUSY_DECISIONS if is_busy else 10**9
    eps = [oracle_episode(cfg, alpha2, s, limit) for s in seeds]
    for ep in eps:
        check_coverage(alpha2, is_busy, ep)
    return cfg, eps


def case_policy_lockstep(make, dataset, env_cfg, alpha2, is_busy, seeds):
    """ssim_policy(kind) on the engine's observation equals the host scheduler's action on the oracle's, at every
    decision (the engine is stepped with the device's own action)."""
    cfg, eps = runs(env_cfg, alpha2, is_busy, seeds)
    eng = make(cfg, len(seeds), dataset, 0)
    eng.reset(seeds=list(seeds))
    steps = max(len(ep.actions) for ep in eps)
    for k in range(steps):
        si, ne = eng.policy(kind_of(alpha2))
        si, ne = np.array(eng.to_numpy(si)), np.array(eng.to_numpy(ne))
        for i, ep in enumerate(eps):
            if k < len(ep.actions):
                assert (int(si[i]), int(ne[i])) == tuple(ep.actions[k]), \
                    f"alpha2 {alpha2} env{i} (seed {seeds[i]}) step{k}"
        eng.step(si, ne)
    c = eng.host_views()["counts"]
    for i, ep in enumerate(eps):
        assert int(c[i][_abi.OC_ERR]) == 0
        assert bool(c[i][_abi.OC_TERMINATED]) == ep.terminated
        if ep.terminated or len(ep.actions) == steps:
            assert int(c[i][_abi.OC_DECISIONS]) == len(ep.actions)


def check_rollout(eng, log, eps, seeds, what):
    """A fused rollout's log and end state against the oracle runs `eps` (env i <-> eps[i]): the logged action of
    every decision, then final observation, wall time, reward, decision count, job times and event trace."""
    v = eng.host_views()
    ta, tc, _ = eng.job_times_np()
    for i, ep in enumerate(eps):
        dec = int(v["counts"][i][_abi.OC_DECISIONS])
        m = min(dec, len(ep.actions))
        diff = np.flatnonzero((log[:m, i] != ep.actions[:m]).any(axis=1))
        assert diff.size == 0, (f"{what} env{i} (seed {seeds[i]}): first differing decision {int(diff[0])}: logged "
                                f"{log[diff[0], i].tolist()}, host scheduler {ep.actions[diff[0]].tolist()}")
        assert dec == len(ep.actions), f"{what} env{i}: {dec} decisions, oracle {len(ep.actions)}"
        assert bool(v["counts"][i][_abi.OC_TERMINATED]) == ep.terminated
        cases.check_replayed_env(eng, v, ta, tc, i, ep.oracle, ep.last_obs, 1, dec, ep.last_reward, what, trace=True)


def case_fused_rollout(make, dataset, env_cfg, alpha2, is_busy, seeds, kind=None):
    """One fused rollout launch of the kind of `alpha2` (or of `kind`: fair, for alpha2 = 0) ends where the oracle
    driven by the host scheduler does, for every env of the batch."""
    cfg, eps = runs(env_cfg, alpha2, is_busy, seeds)
    K = BUSY_DECISIONS if is_busy else max(len(ep.actions) for ep in eps) + 8
    eng = make(cfg, len(seeds), dataset, TRACE_CAP)
    eng.reset(seeds=list(seeds))
    log = eng.alloc_action_log(K)
    eng.rollout(kind_of(alpha2) if kind is None else kind, 0, K, log)
    check_rollout(eng, np.asarray(eng.to_numpy(log)), eps, seeds, f"wfair alpha2 {alpha2} rollout")
    return eng


def case_wide_jobs(make, env_cfg, alpha2):
    """Jobs of 40 stages (the hot-block view's child-list data set) through W(k): `policy(kind)` in lockstep and a
    fused rollout, to termination."""
    cfg = P.wide_cfg(env_cfg)
    eps = [oracle_episode(cfg, alpha2, s, ds_key=P.WIDE) for s in P.WIDE_SEEDS]
    assert all(ep.terminated for ep in eps)
    assert max(ep.counts.max_job_rows for ep in eps) == 40
    K = max(len(ep.actions) for ep in eps)
    for via_rollout in (False, True):
        eng = make(cfg, len(eps), P.datasets(P.WIDE), TRACE_CAP)
        eng.reset(seeds=list(P.WIDE_SEEDS))
        if via_rollout:
            log = eng.alloc_action_log(K)
            eng.rollout(kind_of(alpha2), 0, K, log)
            log = np.asarray(eng.to_numpy(log))
        else:
            log = np.zeros((K, len(eps), 2), dtype=np.int32)
            for k in range(K):
                si, ne = eng.policy(kind_of(alpha2))
                log[k, :, 0], log[k, :, 1] = np.array(eng.to_numpy(si)), np.array(eng.to_numpy(ne))
                eng.step(si, ne)
        check_rollout(eng, log, eps, P.WIDE_SEEDS, f"wfair wide rollout={via_rollout}")


def case_evaluate(alpha2, env_cfg, dataset, seeds, **kwargs):
    """evaluate_policy(..., "wfair", alpha=) equals the oracle driven by the host scheduler (1e-12 relative)."""
    from spark_sched_sim.evaluate import evaluate_policy

    out = evaluate_policy(env_cfg, "wfair", seeds, dataset=dataset, alpha=alpha2 / 2, **kwargs)
    eps = [oracle_episode(env_cfg, alpha2, s) for s in seeds]
    assert all(ep.terminated for ep in eps)
    np.testing.assert_allclose(out["avg_job_duration"], [ep.avg_job_duration for ep in eps], rtol=1e-12, atol=0.0)
    assert out["decisions"].tolist() == [len(ep.actions) for ep in eps]
    assert out["completed_jobs"].tolist() == [ep.completed for ep in eps]
    assert out["wall_time"].tolist() == [float(ep.oracle.wall_time) for ep in eps]
    return out


# ------------------------------------------------------------------------------------------------- known answers
KAT_NS = (1, 63, 64, 65, 130, 200)
KAT_EXECUTORS = (5, 10, 40, 100)


@functools.lru_cache(maxsize=None)
def kat_values() -> np.ndarray:
    """Job works for the arithmetic KAT: 4,096 values log-uniform in [1e-3, 1e13], then perfect squares with their two
    float64 neighbours (where a mis-rounded square root shows), then a zero."""
    rng = np.random.Generator(np.random.PCG64(20240611))
    logu = 10.0 ** rng.uniform(-3.0, 13.0, size=4096)
    roots = np.concatenate([np.arange(1.0, 65.0), rng.integers(65, 3_000_000, size=192).astype(np.float64)])
    sq = roots * roots
    v = np.concatenate([logu, np.nextafter(sq, 0.0), sq, np.nextafter(sq, np.inf), [0.0]])
    v.setflags(write=False)
    return v


def kat_inputs(n: int, salt: int) -> np.ndarray:
    """`n` works drawn from a window of about two decades of the sorted kat_values() (jobs of comparable size, so the
    caps spread over 1..N instead of collapsing to 0 and N); for n = 130 and for one exponent of each n, one of the
    works is replaced by a zero."""
    v = np.sort(kat_values())
    rng = np.random.Generator(np.random.PCG64([7, n, salt]))
    width = len(v) // 8
    lo = int(rng.integers(1, len(v) - width))  # (v[0] is the zero)
    W = v[lo + rng.integers(0, width, size=n)]
    if salt % 8 == 7 or n == 130:
        W[rng.integers(0, n)] = 0.0
    return np.ascontiguousarray(W)


def kat_reference(W: np.ndarray, alpha2: int, N: int):
    """(p, P, cap) of the rule in numpy, through the host scheduler's own parts."""
    s = WeightedFairScheduler(N, alpha=alpha2 / 2)
    p = np.array([s.weight(w, alpha2) for w in W], dtype=np.float64)
    total = s.total(p)
    cap = np.array([s.cap(x, total) if total > 0.0 else 0 for x in p], dtype=np.int32)
    return p, np.float64(total), cap


def case_kat(run):
    """run(W float64 [n], alpha2, N) -> (p [n], P, cap [n]) of the code under test, bit for bit against numpy: every
    value of kat_values() through the weight for all nine exponents, then sums and caps for each n of KAT_NS, every
    exponent and every executor count of KAT_EXECUTORS."""
    v = kat_values()
    for alpha2 in ALPHA2S:
        p, _, _ = run(v[:4096], alpha2, 10)
        p2, _, _ = run(v[4096:], alpha2, 10)
        ref = kat_reference(v, alpha2, 10)[0]
        got = np.concatenate([p, p2])
        bad = np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))
        assert bad.size == 0, (f"alpha2 {alpha2}: {bad.size} weights differ, first W = {v[bad[0]]!r}: "
                               f"{got[bad[0]]!r} != {ref[bad[0]]!r}")
    for n in KAT_NS:
        for alpha2 in ALPHA2S:
            for N in KAT_EXECUTORS:
                W = kat_inputs(n, alpha2 + 4)
                p, total, cap = run(W, alpha2, N)
                rp, rt, rc = kat_reference(W, alpha2, N)
                what = f"n {n} alpha2 {alpha2} N {N}"
                assert (p.view(np.uint64) == rp.view(np.uint64)).all(), what
                assert np.float64(total).view(np.uint64) == rt.view(np.uint64), f"{what}: P {total!r} != {rt!r}"
                assert cap.tolist() == rc.tolist(), what
