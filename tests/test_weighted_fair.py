"""Weighted-fair schedulers (WFair(alpha)) on the CPU: the host scheduler on hand-made observations, the arithmetic of
csrc/policy.h compiled for the host against numpy bit for bit, then the device policy code through the test-only host
build (both views: the obs arena's `policy(kind)` and the hot block's fused rollout, which the host build also checks
against each other at every decision) against the oracle driven by the host scheduler (cases_wfair.py). The gfx950
kernels run the same cases in test_gpu_weighted_fair.py."""

import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import cases_priority as P
import cases_wfair as C
from spark_sched_sim import _abi
from spark_sched_sim.engine import GraphInstance
from spark_sched_sim.schedulers import (RoundRobinScheduler, WeightedFairScheduler, host_scheduler, make_scheduler)

N = 10


def _obs(nodes, dag_ptr, supplies=None, committable=3, src=None):
    """A reference-format observation without edges: nodes = (remaining tasks, most recent duration, schedulable) per
    row; `src` defaults to "no source job" (= the number of jobs)."""
    nj = len(dag_ptr) - 1
    return {"dag_batch": GraphInstance(np.array(nodes, dtype=np.float32).reshape(-1, 3), np.zeros(0, dtype=np.int64),
                                       np.zeros((0, 2), dtype=np.int64)),
            "dag_ptr": list(dag_ptr), "num_committable_execs": committable, "source_job_idx": nj if src is None else src,
            "exec_supplies": list(supplies) if supplies is not None else [0] * nj}


def _act(obs, alpha, n=N):
    a, info = WeightedFairScheduler(n, alpha=alpha).schedule(obs)
    assert info == {}
    return int(a["stage_idx"]), int(a["num_exec"])


def _fair(obs, n=N):
    a, _ = RoundRobinScheduler(n).schedule(obs)
    return int(a["stage_idx"]), int(a["num_exec"])


def _many_jobs(n, seed):
    rng = np.random.Generator(np.random.PCG64([3, n, seed]))
    nodes = [(int(rng.integers(1, 40)), float(rng.uniform(50.0, 5e4)), 1) for _ in range(n)]
    return _obs(nodes, list(range(n + 1)), supplies=[int(x) for x in rng.integers(0, 3, size=n)], committable=5)


# job 0: work 100, job 1: work 1 (one schedulable row each: ranks 0 and 1)
BIG_SMALL = [(10, 10, 1), (1, 1, 1)]
HAND_MADE = [
    _obs(BIG_SMALL, [0, 1, 2], supplies=[5, 0]),
    _obs(BIG_SMALL, [0, 1, 2], supplies=[1, 0]),
    _obs(BIG_SMALL, [0, 1, 2], supplies=[0, 0]),
    _obs(BIG_SMALL, [0, 1, 2], supplies=[9, 9], src=1),
    _obs([(0, 5, 1), (2, 2, 1)], [0, 1, 2]),
    _obs([(0, 5, 1), (0, 2, 1)], [0, 1, 2]),
    _obs([(1, 1, 0), (2, 2, 0)], [0, 1, 2]),
    _obs([], [0]),
    _obs([(3, 0.1, 1)], [0, 1], supplies=[4], committable=8),
    _many_jobs(65, 0),
    _many_jobs(130, 1),
]


@pytest.mark.parametrize("i", range(len(HAND_MADE)))
def test_alpha_zero_is_fair(i):
    assert _act(HAND_MADE[i], 0.0) == _fair(HAND_MADE[i])
    assert _act(HAND_MADE[i], 0.0, n=40) == _fair(HAND_MADE[i], n=40)


def test_served_job_differs_from_fair():
    # supplies (5, 0): fair's cap is 5, job 0 is at it, job 1 is served
    obs = HAND_MADE[0]
    assert _fair(obs) == (1, 3)
    # alpha 1: p = (100, 1), P = 101, cap 0 = ceil(1000 / 101) = 10: job 0 is still under its cap
    assert _act(obs, 1.0) == (0, 3)
    # supplies (1, 0): fair serves job 0; alpha -1: p = (0.01, 1), cap 0 = ceil(0.1 / 1.01) = 1: job 0 is at its cap
    obs = HAND_MADE[1]
    assert _fair(obs) == (0, 3)
    assert _act(obs, -1.0) == (1, 3)
    # half-integer exponents: p = (10, 1) and (0.1, 1); caps (ceil(100 / 11), ceil(10 / 11)) and (ceil(1 / 1.1), 10)
    assert _act(HAND_MADE[0], 0.5) == (0, 3)
    assert _act(HAND_MADE[1], -0.5) == (1, 3)


def test_cap_binds():
    # supplies (0, 0), alpha -1: job 0's cap is 1 < 3 committable
    assert _fair(HAND_MADE[2]) == (0, 3)
    assert _act(HAND_MADE[2], -1.0) == (0, 1)
    # alpha 2: p = (1e4, 1), cap 0 = 10, cap 1 = ceil(10 / 10001) = 1; job 0 takes min(3, 10 - 0)
    assert _act(HAND_MADE[2], 2.0) == (0, 3)
    obs = _obs(BIG_SMALL, [0, 1, 2], supplies=[10, 0])
    assert _act(obs, 2.0) == (1, 1)


def test_source_job_keeps_its_executors():
    # the source job (1) is far over any cap and still gets every committable executor
    for alpha in (-2.0, -0.5, 0.0, 1.5):
        assert _act(HAND_MADE[3], alpha) == (1, 3)
    # a source job with nothing schedulable falls through to the others
    obs = _obs([(10, 10, 1), (1, 1, 0)], [0, 1, 2], supplies=[0, 0], src=1)
    assert _act(obs, 1.0) == (0, 3)


def test_job_without_work():
    # job 0 has a schedulable row and no work: weight 0 (cap 0) unless alpha = 0
    obs = HAND_MADE[4]
    assert _act(obs, 0.0) == (0, 3)
    for alpha in (-1.0, -0.5, 1.0, 2.0):
        assert _act(obs, alpha) == (1, 3)
    s = WeightedFairScheduler(N, alpha=-1.0)
    assert [float(x) for x in s.weights(obs)] == [0.0, 0.25]
    # no job has work: P = 0, no candidate
    assert _act(HAND_MADE[5], 0.0) == (0, 3)
    for alpha in (-1.0, 1.5):
        assert _act(HAND_MADE[5], alpha) == (-1, 3)


@pytest.mark.parametrize("alpha", [-2.0, -0.5, 0.0, 1.0])
def test_no_candidate(alpha):
    assert _act(HAND_MADE[6], alpha) == (-1, 3)
    assert _act(HAND_MADE[7], alpha) == (-1, 3)


@pytest.mark.parametrize("alpha2", C.ALPHA2S)
def test_single_job_is_clamped_to_all_executors(alpha2):
    # one active job: p / P = 1 up to rounding, the cap is N whichever way (N * p) / P rounds
    s = WeightedFairScheduler(N, alpha=alpha2 / 2)
    assert _act(HAND_MADE[8], alpha2 / 2) == (0, 6)
    for w in (0.3, 3.0 * float(np.float32(0.1)), 7.0, 1e13 / 3.0):
        p = s.weight(w, alpha2)
        assert s.cap(p, s.total([p])) == N
    assert s.cap(1.0, 0.25) == N and s.cap(0.0, 0.25) == 0  # far over, and a job without weight


def _fold_halves(p):
    total = 0.0
    for b in range(0, len(p), 64):
        x = [float(v) for v in p[b:b + 64]]
        x += [0.0] * (64 - len(x))
        for half in (32, 16, 8, 4, 2, 1):
            for i in range(half):
                x[i] = x[i] + x[i + half]
        total = total + x[0]
    return total


@pytest.mark.parametrize("alpha2", C.NONZERO)
@pytest.mark.parametrize("i", [9, 10], ids=["65", "130"])
def test_sum_order(i, alpha2):
    obs = HAND_MADE[i]
    s = WeightedFairScheduler(40, alpha=alpha2 / 2)
    p = s.weights(obs)
    assert len(p) in (65, 130)
    want = _fold_halves(p)
    assert float(s.total(p)) == want
    # the action is the first job under the cap that this P gives
    caps = [min(40, int(np.ceil((40.0 * float(x)) / want))) for x in p]
    first = next(k for k in range(len(p)) if obs["exec_supplies"][k] < caps[k])
    assert _act(obs, alpha2 / 2, n=40) == (first, min(5, caps[first] - obs["exec_supplies"][first]))


def test_sum_order_matters():
    # (the order is part of the rule: on these weights a left-to-right sum gives another float64; reciprocals, since
    # sums of the works themselves, float32 x small integers, are exact in float64 in any order)
    s = WeightedFairScheduler(40, alpha=-1.0)
    seen = 0
    for i in (9, 10):
        p = s.weights(HAND_MADE[i])
        seq = 0.0
        for x in p:
            seq += float(x)
        seen += seq != float(s.total(p))
    assert seen >= 1


def test_names_and_factories():
    s = make_scheduler({"agent_cls": "WeightedFairScheduler", "num_executors": 7, "alpha": 1.5})
    assert isinstance(s, WeightedFairScheduler) and s.name == "WFair(1.5)" and (s.num_executors, s.alpha2) == (7, 3)
    s = WeightedFairScheduler(3)
    assert (s.name, s.alpha, s.kind) == ("WFair(-1)", -1.0, 0x102)
    assert host_scheduler("wfair", 10).name == "WFair(-1)" and host_scheduler("wfair", 10, alpha=2).alpha2 == 4
    for bad in (0.3, 2.5, -2.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            WeightedFairScheduler(10, alpha=bad)
    with pytest.raises(ValueError):
        host_scheduler("sjf", 10, alpha=1.0)
    assert "wfair" not in _abi.POLICY_KINDS


def test_kind_round_trip():
    assert _abi.SSIM_POLICY_WFAIR_BASE == 0x100
    assert [_abi.wfair_kind(a) for a in _abi.WFAIR_ALPHAS] == list(range(0x100, 0x109))
    assert _abi.WFAIR_ALPHAS == (-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0)
    for a in _abi.WFAIR_ALPHAS:
        assert _abi.wfair_alpha(_abi.wfair_kind(a)) == a
    assert _abi.wfair_kind(1) == 0x106 and _abi.wfair_kind(-0.5) == 0x103
    for bad in (0.3, 2.5, -2.25, float("nan"), None):
        with pytest.raises(ValueError):
            _abi.wfair_kind(bad)
    for bad in (0xFF, 0x109, 1, 5):
        with pytest.raises(ValueError):
            _abi.wfair_alpha(bad)


def test_examples_accepts_wfair(capsys):
    from spark_sched_sim import examples

    with pytest.raises(SystemExit):
        examples.main(["--sched", "wfair", "--alpha", "0.3"])
    assert "half-integer" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        examples.main(["--sched", "sjf", "--alpha", "1"])
    assert "wfair" in capsys.readouterr().err


# ----------------------------------------------------------------------------- the arithmetic of policy.h on the host
@pytest.fixture(scope="module")
def kat_lib(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    so = str(tmp_path_factory.mktemp("wfair_kat") / "wfair_kat.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", f"-I{os.path.join(repo, 'include')}",
                    f"-I{os.path.join(repo, 'gym-sparksched_amd', 'csrc')}",
                    os.path.join(here, "hostsim", "wfair_kat.cpp"), "-o", so], check=True)
    lib = ct.CDLL(so)
    lib.wk_run.argtypes = [ct.c_void_p, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    return lib


def test_arithmetic_kat(kat_lib):
    def run(W, alpha2, n_exec):
        W = np.ascontiguousarray(W, dtype=np.float64)
        p, total, cap = np.zeros(len(W)), np.zeros(1), np.zeros(len(W), dtype=np.int32)
        assert kat_lib.wk_run(W.ctypes.data, len(W), alpha2, n_exec, p.ctypes.data, total.ctypes.data,
                              cap.ctypes.data) == 0
        return p, total[0], cap

    C.case_kat(run)


def test_unit_rule(kat_lib):
    """units.h: the weighted-fair kinds run the run-time-shape unit of the residency, whatever the shape."""
    from spark_sched_sim._abi import SsimLayout

    kat_lib.wk_unit_name.restype = ct.c_char_p
    kat_lib.wk_unit_name.argtypes = [ct.POINTER(SsimLayout), ct.c_int, ct.c_int]
    for n_exec, jobs, cap in ((10, 50, 900), (50, 200, 3600), (100, 200, 3600), (20, 30, 540)):
        for generic in (0, 1):
            L = SsimLayout(num_executors=n_exec, job_cap=jobs, stage_cap=cap, lds_resident=1)
            assert kat_lib.wk_unit_name(ct.byref(L), 1, generic) == b"wfair_lds"
            L.lds_resident = 0
            assert kat_lib.wk_unit_name(ct.byref(L), 0, generic) == b"wfair_hbm"


def test_kat_inputs_reach_the_edges():
    """What the KAT is there for: perfect squares with both neighbours, caps next to an integer boundary."""
    v = C.kat_values()
    assert len(v) == 4096 + 3 * 256 + 1 and v[:4096].min() >= 1e-3 and v[:4096].max() <= 1e13
    r = np.sqrt(v[4096 + 256:4096 + 512])
    assert (r == np.round(r)).all() and (r * r == v[4096 + 256:4096 + 512]).all()
    spread = set()
    for n in C.KAT_NS:
        for alpha2 in C.NONZERO:
            spread.update(C.kat_reference(C.kat_inputs(n, alpha2 + 4), alpha2, 40)[2].tolist())
    # (a job without weight, a lone job's clamp, and shares in between: with 63..200 jobs of 40 executors, small ones)
    assert {0, 1, 2, 3, 40} <= spread, sorted(spread)


# ------------------------------------------------------------------------------------ the host build of the engine
@pytest.fixture(scope="module", params=[False, True], ids=["hbm", "lds"])
def make(request):
    """As test_hostsim_parity.py: `lds` emulates the device's LDS residency on a poisoned working copy."""
    from hostsim.driver import HostEngine

    def _make(cfg, B, ds, trace_cap):
        return HostEngine(cfg, B, ds, trace_cap=trace_cap, resident=request.param)

    return _make


def test_alpha_zero_rollout_is_fair(make, dataset, env_cfg):
    """Both kinds end where the oracle driven by WFair(0) does (whose actions the case checks to be fair's)."""
    assert C.kind_of(0) == 0x104
    for kind in (0x104, _abi.SSIM_POLICY_FAIR):
        C.case_fused_rollout(make, dataset, env_cfg, 0, False, C.DEFAULT_SEEDS, kind=kind)


def test_alpha_zero_logs_equal_fair_logs(make, dataset, env_cfg):
    out = []
    for kind in (0x104, _abi.SSIM_POLICY_FAIR):
        eng = make(env_cfg, 2, dataset, 0)
        eng.reset(seeds=list(C.DEFAULT_SEEDS))
        log = eng.alloc_action_log(1200)
        log[:] = -7
        eng.rollout(kind, 0, 1200, log)
        assert (eng.host_views()["counts"][:, _abi.OC_TERMINATED] != 0).all()
        out.append(np.asarray(eng.to_numpy(log)).copy())
    assert (out[0] == out[1]).all()


@pytest.mark.parametrize("alpha2", [-2, 1])
def test_policy_lockstep_default(make, dataset, env_cfg, alpha2):
    C.case_policy_lockstep(make, dataset, env_cfg, alpha2, False, C.DEFAULT_SEEDS)


@pytest.mark.parametrize("alpha2", C.NONZERO)
def test_fused_rollout_default(make, dataset, env_cfg, alpha2):
    C.case_fused_rollout(make, dataset, env_cfg, alpha2, False, C.DEFAULT_SEEDS)


@pytest.mark.parametrize("alpha2", [-2, 2])
def test_policy_lockstep_busy(make, dataset, env_cfg, alpha2):
    C.case_policy_lockstep(make, dataset, env_cfg, alpha2, True, C.BUSY_SEEDS)


@pytest.mark.parametrize("alpha2", C.BUSY_ALPHA2S)
def test_fused_rollout_busy(make, dataset, env_cfg, alpha2):
    C.case_fused_rollout(make, dataset, env_cfg, alpha2, True, C.BUSY_SEEDS)


def test_wide_jobs(make, env_cfg):
    C.case_wide_jobs(make, env_cfg, -2)


def _host_factory(cfg, B, ds):
    from hostsim.driver import HostEngine

    return HostEngine(cfg, B, ds)


@pytest.mark.parametrize("alpha2", [-2, 3])
def test_evaluate_policy(dataset, env_cfg, alpha2):
    out = C.case_evaluate(alpha2, env_cfg, dataset, C.DEFAULT_SEEDS, engine_factory=_host_factory)
    assert out["launches"] >= 4 and (out["completed_jobs"] == env_cfg["job_arrival_cap"]).all()


def test_tune_weighted_fair(dataset, env_cfg):
    from spark_sched_sim.evaluate import evaluate_policy, tune_weighted_fair

    alphas = [1.0, -1.0, 0.0]
    got = tune_weighted_fair(env_cfg, C.DEFAULT_SEEDS, alphas=alphas, dataset=dataset, engine_factory=_host_factory)
    assert list(got["mean_avg_job_duration"]) == alphas and list(got["per_seed"]) == alphas
    for a in alphas:
        one = evaluate_policy(env_cfg, "wfair", C.DEFAULT_SEEDS, dataset=dataset, alpha=a,
                              engine_factory=_host_factory)["avg_job_duration"]
        assert (got["per_seed"][a] == one).all()
        assert got["mean_avg_job_duration"][a] == float(np.mean(one))
        ref = [C.oracle_episode(env_cfg, int(2 * a), s).avg_job_duration for s in C.DEFAULT_SEEDS]
        np.testing.assert_allclose(one, ref, rtol=1e-12, atol=0.0)
    mean = got["mean_avg_job_duration"]
    assert got["alpha"] == min(alphas, key=lambda a: (mean[a], abs(a), a))


def test_tune_weighted_fair_ties_and_default_grid(monkeypatch):
    from spark_sched_sim import evaluate

    calls = []

    def fake(env_cfg, kind, seeds, alpha=None, **kw):
        calls.append((kind, alpha, kw))
        return {"avg_job_duration": np.array([2.0, 4.0]) + (1.0 if abs(alpha) == 2.0 else 0.0)}

    monkeypatch.setattr(evaluate, "evaluate_policy", fake)
    got = evaluate.tune_weighted_fair({}, [1, 2], device="cuda:0")
    assert [c[1] for c in calls] == list(_abi.WFAIR_ALPHAS) and all(c[0] == "wfair" for c in calls)
    assert calls[0][2] == {"device": "cuda:0"}
    assert got["alpha"] == 0.0 and got["mean_avg_job_duration"][2.0] == 4.0  # all of -1.5..1.5 tie: the smallest |alpha|
    assert evaluate.tune_weighted_fair({}, [1, 2], alphas=[1.0, -1.0, 2.0])["alpha"] == -1.0  # then the smaller alpha
    with pytest.raises(ValueError):
        evaluate.tune_weighted_fair({}, [1, 2], alphas=[0.3])


def test_evaluate_policy_arguments(dataset, env_cfg):
    from spark_sched_sim.evaluate import evaluate_policy, policy_kind

    for bad in (0.3, 2.5):
        with pytest.raises(ValueError, match="half-integer"):
            evaluate_policy(env_cfg, "wfair", [77], dataset=dataset, alpha=bad, engine_factory=_host_factory)
    with pytest.raises(ValueError, match="wfair"):
        evaluate_policy(env_cfg, "sjf", [77], dataset=dataset, alpha=1.0, engine_factory=_host_factory)
    with pytest.raises(ValueError):
        evaluate_policy(env_cfg, _abi.SSIM_POLICY_FAIR, [77], dataset=dataset, alpha=0.0,
                        engine_factory=_host_factory)
    for bad in ("wfair", 0x104, 0x109):  # (policy_kind is the named kinds' alone, as before)
        with pytest.raises(ValueError):
            policy_kind(bad)


def test_run_episode_wfair_matches_oracle(dataset, env_cfg):
    """The facade episode of `examples.py --sched wfair --alpha -1` (one step per call, the host scheduler choosing)."""
    from hostsim.driver import HostEngine
    from spark_sched_sim.examples import run_episode

    got = run_episode(env_cfg, host_scheduler("wfair", env_cfg["num_executors"], alpha=-1.0), seed=77, dataset=dataset,
                      _engine_factory=lambda cfg, ds: HostEngine(cfg, 1, ds))
    assert np.isclose(got, C.oracle_episode(env_cfg, -2, 77).avg_job_duration, rtol=1e-12)
