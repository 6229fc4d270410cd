"""The per-decision tail of the fused rollout (engine.h scan_sched / observe, rollout.h rollout_loop): one predicate
pass per decision handed to observe() as ballot masks, delta observations on round-continuing decisions, the header
kept in registers across a launch.

Short launches of 1, 2 and 3 decisions per env (offset by env index, so every decision index ends a launch in some
env both as the launch's first — always full — observation and as a later, possibly delta, one). After every launch
each env's actions so far are replayed on the CPU oracle and the obs arena is compared with the oracle's observation:
node features, edge links, dag_ptr, supplies, committable and source index bit for bit (parity.compare_obs), the
counts, the wall time and the accumulators.

Two shapes, the smallest at which each path can go wrong: one 64-node mask chunk (the common case), and a pile-up of
jobs whose observations pass 64, 128 and 192 active nodes (two and three mask chunks, then observe()'s own predicate
pass). The host build runs the plain launches; the device runs them too, with the arena poisoned between launches
(the first observation of a launch must be full) and once through preemptible auto-reset budget launches (the
deferred header store and the once-read pending mark across launch and episode boundaries). The host driver's
rollout has no budget launches and checks the obs-arena policy view against the hot-block one before every step, so
a poisoned arena or a budget launch cannot be put through it.
"""

import numpy as np
import pytest

import parity
from oracle.restatement import SparkSchedOracle
from spark_sched_sim import _abi
from spark_sched_sim.engine import obs_dict

# (i) one chunk: 10 executors, 6 jobs, the bench's arrival rate
CFG_ONE_CHUNK = dict(num_executors=10, job_arrival_cap=6, job_arrival_rate=4.0e-5, moving_delay=2000.0,
                     warmup_delay=1000.0)
# (ii) jobs pile up on 5 executors: observations of <= 64, 65..128, 129..192 and > 192 active nodes
CFG_PILE_UP = dict(num_executors=5, job_arrival_cap=14, job_arrival_rate=1.0e-3, moving_delay=2000.0,
                   warmup_delay=1000.0)
SHAPES = {"one_chunk": (CFG_ONE_CHUNK, False), "pile_up": (CFG_PILE_UP, True)}
SENT = -99
EVENT_KINDS = (1, 2, 3)  # job arrival, task completion, executor ready (the other trace kinds are no events)
POISON = {"nodes": -777.0, "edge_links": -12345, "dag_ptr": -12345, "frontier": 0xAB, "sched_rank": -12345,
          "exec_supplies": -12345}


def _sizes(ob):
    return ob["dag_batch"].nodes.shape[0], ob["dag_batch"].edge_links.shape[0], len(ob["dag_ptr"]) - 1


class Replay:
    """One env's oracle, advanced action by action, with the accumulators the engine must show (EnvAcc: every
    observation, the reset's included, adds its node / edge / job counts and the step's events)."""

    def __init__(self, cfg, dataset, seed, autoreset):
        self.o = SparkSchedOracle(cfg, dataset)
        self.o.trace = []
        self.autoreset = autoreset
        self.ob, _ = self.o.reset(seed=seed)
        self.acc = np.zeros(6, dtype=np.int64)
        self.acc[:3] += _sizes(self.ob)
        self.term = False
        self.step_events = 0
        self.episode = 1
        self.sizes = [_sizes(self.ob)[0]]

    def apply(self, a):
        if self.term:  # the engine resets a finished episode in place once it holds the next decision
            assert self.autoreset
            self.o.trace = []
            self.ob, _ = self.o.reset(seed=None)
            self.acc[:3] += _sizes(self.ob)
            self.acc[_abi.ACC_EPISODES] += 1
            self.episode += 1
            self.sizes.append(_sizes(self.ob)[0])
        t0 = len(self.o.trace)
        self.ob, _, self.term, _, self.info = self.o.step({"stage_idx": int(a[0]), "num_exec": int(a[1])})
        self.step_events = sum(1 for r in self.o.trace[t0:] if r[1] in EVENT_KINDS)
        self.acc[:3] += _sizes(self.ob)
        self.acc[_abi.ACC_EVENTS] += self.step_events
        self.acc[_abi.ACC_DECISIONS] += 1
        self.sizes.append(_sizes(self.ob)[0])


def _compare(v, i, r, where):
    c = v["counts"][i]
    assert int(c[_abi.OC_ERR]) == 0, f"{where}: error bits {int(c[_abi.OC_ERR]):#x}"
    parity.compare_obs(r.ob, obs_dict(v, i), where)
    n, ne, nj = _sizes(r.ob)
    assert (int(c[_abi.OC_NUM_NODES]), int(c[_abi.OC_NUM_EDGES]), int(c[_abi.OC_NUM_JOBS])) == (n, ne, nj), where
    assert bool(c[_abi.OC_TERMINATED]) == bool(r.term), where
    assert int(c[_abi.OC_DECISIONS]) == r.o.decisions, where
    assert int(c[_abi.OC_STEP_EVENTS]) == r.step_events, where
    assert int(c[_abi.OC_EPISODE]) == r.episode, where
    assert float(v["wall_time"][i]) == float(r.o.wall_time), where
    assert [int(x) for x in v["acc"][i][:6]] == [int(x) for x in r.acc], f"{where}: acc {v['acc'][i][:6]} != {r.acc}"


def _poison(eng):
    for k, val in POISON.items():
        eng.views[k][...] = val


def case_short_launches(make, dataset, cfg, classes, B=16, decisions=120, poison=False, seed0=7300):
    eng = make(cfg, B, dataset, 0)
    seeds = [seed0 + i for i in range(B)]
    eng.reset(seeds=seeds)
    rep = [Replay(cfg, dataset, s, False) for s in seeds]
    v = eng.host_views()
    for i in range(B):
        _compare(v, i, rep[i], f"env{i} reset")
    compared = delta = 0
    launch = 0
    while any(not r.term and r.o.decisions < decisions for r in rep):
        steps = np.array([1 + (launch + i) % 3 for i in range(B)], dtype=np.int32)
        log = eng.alloc_action_log(3)
        log[...] = SENT
        if poison:
            _poison(eng)
        eng.rollout_steps(_abi.SSIM_POLICY_RANDOM, 17, steps, 3, log)
        lg = np.asarray(eng.to_numpy(log))
        v = eng.host_views()
        for i in range(B):
            r = rep[i]
            if r.term:  # (no auto-reset: a finished env takes no more steps and its rows are not rewritten)
                continue
            taken = 0
            for k in range(int(steps[i])):
                assert lg[k, i, 0] != SENT, f"env{i} launch{launch}: step {k} not logged"
                r.apply(lg[k, i])
                taken += 1
                if r.term:
                    break
            _compare(v, i, r, f"env{i} launch{launch} decision{r.o.decisions}")
            compared += 1
            if r.step_events == 0 and taken >= 2:  # a round that continued on a later step of the launch: delta
                delta += 1
        launch += 1
    sizes = np.array([n for r in rep for n in r.sizes])
    print(f"launches {launch}, compared {compared}, through the delta path {delta}, decisions per env "
          f"{min(r.o.decisions for r in rep)}..{max(r.o.decisions for r in rep)}, nodes up to {int(sizes.max())}")
    assert compared > 0 and delta >= 0.10 * compared, (delta, compared)
    if classes:  # from the oracle's observations alone: every mask-chunk count and the recompute fallback occurred
        seen = [bool(np.any(sizes <= 64)), bool(np.any((sizes > 64) & (sizes <= 128))),
                bool(np.any((sizes > 128) & (sizes <= 192))), bool(np.any(sizes > 192))]
        assert all(seen), (seen, int(sizes.max()))
    eng.close()


def case_preempt_autoreset(make, dataset, cfg, B=16, launches=8, per_launch=3, seed0=7400):
    """Budget launches with SSIM_ROLLOUT_PREEMPT | SSIM_ROLLOUT_AUTORESET (the shape of cases.case_rollout_preempt):
    after every launch the envs with no step pending are compared as above on the decisions they completed; a
    closing launch of 0 new steps completes the pending ones."""
    eng = make(cfg, B, dataset, 0)
    seeds = [seed0 + i for i in range(B)]
    eng.reset(seeds=seeds)
    rep = [Replay(cfg, dataset, s, True) for s in seeds]
    flags = _abi.SSIM_ROLLOUT_PREEMPT | _abi.SSIM_ROLLOUT_AUTORESET
    K = 8 * per_launch
    actions = [[] for _ in range(B)]
    applied = [0] * B
    compared = 0

    def check(tag, final):
        nonlocal compared
        v = eng.host_views()
        for i in range(B):
            done = int(v["acc"][i][_abi.ACC_DECISIONS])
            pending = bool(int(v["counts"][i][_abi.OC_ERR]) & _abi.SSIM_ERR_PENDING)
            assert done == len(actions[i]) - (1 if pending else 0), f"env{i} {tag}"
            while applied[i] < done:
                rep[i].apply(actions[i][applied[i]])
                applied[i] += 1
            if pending:  # its rows are the observation before the pending step (or a reset's): compared next launch
                assert not final
                continue
            _compare(v, i, rep[i], f"env{i} {tag}")
            compared += 1

    for launch in range(launches):
        log = eng.alloc_action_log(K)
        log[...] = SENT
        eng.rollout_budget(_abi.SSIM_POLICY_RANDOM, 17, K, B * per_launch, log, flags=flags)
        lg = np.asarray(eng.to_numpy(log))
        for i in range(B):
            rows = lg[:, i, 0] != SENT
            actions[i] += [(int(a), int(b)) for a, b in lg[rows, i]]
        check(f"launch{launch}", False)
    eng.rollout(_abi.SSIM_POLICY_RANDOM, 17, 0, flags=_abi.SSIM_ROLLOUT_AUTORESET)
    check("closing launch", True)
    assert compared >= B * launches // 2
    eng.close()


@pytest.fixture(scope="module", params=[False, True], ids=["hbm", "lds"])
def make_host(request):
    from hostsim.driver import HostEngine

    def _make(cfg, B, ds, trace_cap):
        return HostEngine(cfg, B, ds, trace_cap=trace_cap, resident=request.param)

    return _make


@pytest.fixture
def make_device(gpu_device):
    from spark_sched_sim.engine import DeviceEngine

    def _make(cfg, B, ds, trace_cap):
        return DeviceEngine(cfg, B, ds, device=gpu_device, trace_cap=trace_cap)

    return _make


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_short_launches_host(make_host, dataset, shape):
    cfg, classes = SHAPES[shape]
    case_short_launches(make_host, dataset, cfg, classes)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_short_launches_device(make_device, dataset, shape, poison):
    cfg, classes = SHAPES[shape]
    case_short_launches(make_device, dataset, cfg, classes, poison=poison)


@pytest.mark.gpu
def test_preempt_autoreset_device(make_device, dataset):
    case_preempt_autoreset(make_device, dataset, CFG_ONE_CHUNK)
