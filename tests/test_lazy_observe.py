"""Deferred arena rows in the fused rollouts of the heuristic and priority policies (engine.h observe_parts /
flush_rows, rollout.h rollout_loop's exit): a decision of such a launch runs the observation's decision part and
writes the scalar words (acc, counts, reward, wall time); the row arrays (nodes, frontier, sched_rank, dag_ptr,
exec_supplies, edge_links) are written once, in full, when the env leaves the launch.

Launches of several decisions per env; after every launch each env's logged actions are replayed on the CPU oracle and
the whole observation is compared with the oracle's at the env's decision count (test_observe_delta's Replay and
_compare: rows bit for bit, counts, wall time, accumulators). The arena rows are poisoned between launches, so a row the
flush leaves out cannot compare equal, and the edge count every decision carries (JobRec::edges) is compared with the
oracle's through the counts and the edge accumulator. The shapes are test_observe_delta's: one 64-node chunk, and a
pile-up that passes 64, 128 and 192 active nodes.

  * lockstep launches of 3..6 decisions per env;
  * per-env step caps 0, 1, 2 and 4: a cap-0 env's rows keep the poison, a cap-1 env is compared;
  * budget launches with SSIM_ROLLOUT_PREEMPT | SSIM_ROLLOUT_AUTORESET (device only): non-pending envs are compared
    after every launch, every env after the closing one; a pending env's scalar words are those of its last completed
    decision (its rows are unspecified until a launch completes the step);
  * one shortest-job-first launch series (k_rollout_prio's driver).

The host cases run the same loop (hostsim_lazy.cpp) in both residency emulations. Host builds check() the carried edge
count against the edge pass's at every flush and in every full observation of an eager engine; a mismatch freezes the
env, and every case asserts that no env froze.
"""

import numpy as np
import pytest

from spark_sched_sim import _abi
from test_observe_delta import (CFG_ONE_CHUNK, POISON, SENT, SHAPES, Replay, _compare, _poison)

LOCKSTEP = (3, 4, 5, 6)  # decisions per launch, by (launch + env) % 4
CAPS = (0, 1, 2, 4)      # per-env step caps, likewise


def _assert_none_frozen(v, where):
    err = np.asarray(v["counts"])[:, _abi.OC_ERR].astype(np.int64)
    assert not np.any(err & _abi.SSIM_ERR_STICKY), f"{where}: frozen envs {np.nonzero(err & _abi.SSIM_ERR_STICKY)[0]}"


def _rows_poisoned(v, i):
    return all(bool(np.all(np.asarray(v[k][i]) == val)) for k, val in POISON.items())


def case_launches(make, dataset, cfg, classes, pattern, kind=_abi.SSIM_POLICY_RANDOM, B=16, decisions=120,
                  seed0=7300):
    """rollout_steps launches of pattern[(launch + env) % len] decisions, the arena rows poisoned before each."""
    eng = make(cfg, B, dataset, 0)
    seeds = [seed0 + i for i in range(B)]
    eng.reset(seeds=seeds)
    rep = [Replay(cfg, dataset, s, False) for s in seeds]
    kmax = max(pattern)
    compared = untouched = multi = launch = 0
    while any(not r.term and r.o.decisions < decisions for r in rep):
        steps = np.array([pattern[(launch + i) % len(pattern)] for i in range(B)], dtype=np.int32)
        log = eng.alloc_action_log(kmax)
        log[...] = SENT
        _poison(eng)
        eng.rollout_steps(kind, 17, steps, kmax, log)
        lg = np.asarray(eng.to_numpy(log))
        v = eng.host_views()
        _assert_none_frozen(v, f"launch{launch}")
        for i in range(B):
            r = rep[i]
            if r.term or steps[i] == 0:  # no decision part ran in this launch: nothing is flushed
                assert _rows_poisoned(v, i), f"env{i} launch{launch}: rows written without a decision"
                untouched += 1
                continue
            taken = 0
            for k in range(int(steps[i])):
                assert lg[k, i, 0] != SENT, f"env{i} launch{launch}: step {k} not logged"
                r.apply(lg[k, i])
                taken += 1
                if r.term:
                    break
            _compare(v, i, r, f"env{i} launch{launch} decision{r.o.decisions} ({taken} in the launch)")
            compared += 1
            multi += taken >= 2
        launch += 1
    sizes = np.array([n for r in rep for n in r.sizes])
    print(f"launches {launch}, compared {compared} ({multi} after two or more decisions), untouched {untouched}, "
          f"nodes up to {int(sizes.max())}")
    assert compared > 0 and multi > 0
    if 0 in pattern:
        assert untouched > 0
    if classes:  # every mask-chunk count and the recompute fallback occurred (from the oracle's observations alone)
        seen = [bool(np.any(sizes <= 64)), bool(np.any((sizes > 64) & (sizes <= 128))),
                bool(np.any((sizes > 128) & (sizes <= 192))), bool(np.any(sizes > 192))]
        assert all(seen), (seen, int(sizes.max()))
    eng.close()


def case_budget(make, dataset, cfg, B=16, launches=8, per_launch=3, seed0=7600):
    """test_observe_delta.case_preempt_autoreset's launches with the arena rows poisoned before each, plus the scalar
    words of the pending envs: those of the env's last completed decision."""
    eng = make(cfg, B, dataset, 0)
    seeds = [seed0 + i for i in range(B)]
    eng.reset(seeds=seeds)
    rep = [Replay(cfg, dataset, s, True) for s in seeds]
    flags = _abi.SSIM_ROLLOUT_PREEMPT | _abi.SSIM_ROLLOUT_AUTORESET
    K = 8 * per_launch
    actions = [[] for _ in range(B)]
    applied = [0] * B
    was_pending = [False] * B
    compared = pend_checked = idle = 0

    def check(tag, final, new):
        nonlocal compared, pend_checked, idle
        v = eng.host_views()
        _assert_none_frozen(v, tag)
        for i in range(B):
            c = v["counts"][i]
            if not final and not was_pending[i] and new[i] == 0:  # the budget ran out before the env's first claim
                assert _rows_poisoned(v, i), f"env{i} {tag}: rows written without a decision"
                idle += 1
                continue
            done = int(v["acc"][i][_abi.ACC_DECISIONS])
            pending = bool(int(c[_abi.OC_ERR]) & _abi.SSIM_ERR_PENDING)
            assert done == len(actions[i]) - (1 if pending else 0), f"env{i} {tag}"
            while applied[i] < done:
                rep[i].apply(actions[i][applied[i]])
                applied[i] += 1
            r = rep[i]
            was_pending[i] = pending
            if not pending:
                _compare(v, i, r, f"env{i} {tag}")
                compared += 1
                continue
            assert not final
            assert int(c[_abi.OC_ERR]) == _abi.SSIM_ERR_PENDING, f"env{i} {tag}"
            if r.term:  # the launch reset the finished episode before the pending step: the words are the reset's,
                continue  # which the replay reaches with the env's next action
            where = f"env{i} {tag} (pending)"
            n, ne, nj = (r.ob["dag_batch"].nodes.shape[0], r.ob["dag_batch"].edge_links.shape[0],
                         len(r.ob["dag_ptr"]) - 1)
            assert (int(c[_abi.OC_NUM_NODES]), int(c[_abi.OC_NUM_EDGES]), int(c[_abi.OC_NUM_JOBS])) == (n, ne, nj), where
            assert int(c[_abi.OC_DECISIONS]) == r.o.decisions, where
            assert int(c[_abi.OC_STEP_EVENTS]) == r.step_events, where
            assert int(c[_abi.OC_EPISODE]) == r.episode, where
            assert not bool(c[_abi.OC_TERMINATED]), where
            assert float(v["wall_time"][i]) == float(r.o.wall_time), where
            assert [int(x) for x in v["acc"][i][:6]] == [int(x) for x in r.acc], where
            pend_checked += 1

    for launch in range(launches):
        log = eng.alloc_action_log(K)
        log[...] = SENT
        _poison(eng)
        eng.rollout_budget(_abi.SSIM_POLICY_RANDOM, 17, K, B * per_launch, log, flags=flags)
        lg = np.asarray(eng.to_numpy(log))
        new = [0] * B
        for i in range(B):
            rows = lg[:, i, 0] != SENT
            new[i] = int(rows.sum())
            actions[i] += [(int(a), int(b)) for a, b in lg[rows, i]]
        check(f"launch{launch}", False, new)
    # (not poisoned: the closing launch starts no step, so an env with none pending keeps the rows it has)
    eng.rollout(_abi.SSIM_POLICY_RANDOM, 17, 0, flags=_abi.SSIM_ROLLOUT_AUTORESET)
    check("closing launch", True, [0] * B)
    print(f"compared {compared}, pending envs checked {pend_checked}, without a decision {idle}")
    assert compared >= B * launches // 2
    assert pend_checked > 0
    eng.close()


@pytest.fixture(scope="module", params=[False, True], ids=["hbm", "lds"])
def make_host(request):
    from hostsim.lazy_driver import LazyHostEngine

    def _make(cfg, B, ds, trace_cap):
        return LazyHostEngine(cfg, B, ds, trace_cap=trace_cap, resident=request.param)

    return _make


@pytest.fixture
def make_device(gpu_device):
    from spark_sched_sim.engine import DeviceEngine

    def _make(cfg, B, ds, trace_cap):
        return DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap)

    return _make


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_lockstep_host(make_host, dataset, shape):
    cfg, classes = SHAPES[shape]
    case_launches(make_host, dataset, cfg, classes, LOCKSTEP)


def test_step_caps_host(make_host, dataset):
    case_launches(make_host, dataset, CFG_ONE_CHUNK, False, CAPS, decisions=60)


def test_priority_host(make_host, dataset):
    case_launches(make_host, dataset, CFG_ONE_CHUNK, False, LOCKSTEP, kind=_abi.SSIM_POLICY_SJF, decisions=60)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_lockstep_device(make_device, dataset, shape):
    cfg, classes = SHAPES[shape]
    case_launches(make_device, dataset, cfg, classes, LOCKSTEP)


@pytest.mark.gpu
def test_step_caps_device(make_device, dataset):
    case_launches(make_device, dataset, CFG_ONE_CHUNK, False, CAPS, decisions=60)


@pytest.mark.gpu
def test_budget_device(make_device, dataset):
    case_budget(make_device, dataset, CFG_ONE_CHUNK)


@pytest.mark.gpu
def test_priority_device(make_device, dataset):
    case_launches(make_device, dataset, CFG_ONE_CHUNK, False, LOCKSTEP, kind=_abi.SSIM_POLICY_SJF, decisions=60)
