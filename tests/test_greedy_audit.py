"""The GREEDY persistent Decima rollout (ssim_decima_rollout with SSIM_ROLLOUT_GREEDY; csrc/k_drg_*.hip) audited
against the CPU oracle by regret (tests/decima_audit.py, the Greedy rule), per kernel unit (drg_lds50, drg_hbm50,
drg_lds, drg_hbm) on test_decima_audit.CASES' envs, seeds, limits, config flags and plans, at most 400 decisions per
env.

The policy of every case: DecimaScheduler's init at torch.manual_seed(6) plus 0.1 * randn on every parameter. With the
sampled audit's policy (seed 5, noise 0.05) the greedy exec choice is k = 0 on every decision, so the exec arg-max
would not be exercised; noise of 0.3-0.5 saturates the tanh layers and leaves up to 96% of decisions inside the
score margin. What a case must contain is asserted from the reference alone (test_gpu_case_reference_collection): at
least 75% of decisions decisive (both leads above their margins), at least 100 decisive decisions with an exec winner
k > 0, at least 100 with a stage winner that is not the first schedulable stage.

CPU-measured per case (reference_rollout under Greedy; every episode ends before the 400-decision cap):
  case          decisions (per env)          decisive   exec winner k > 0   stage winner > 0   plan lds / global
  dr_lds_n10    871 (169 / 279 / 268 / 155)  94.8%      718                 748                871 / 0
  dr_lds50      690 (175 / 97 / 217 / 201)   89.1%      576                 569                553 / 137
  dr_hbm50      the same trajectories
  dr_lds_n20    277 (127 / 150)              87.7%      213                 239                190 / 87
  dr_hbm_n127   284 (137 / 147)              83.5%      227                 193                211 / 73  (cap > 64: 69)
  dr_hbm_n3     581 (226 / 191 / 164)        93.5%      411                 527                49 / 532
(the two winner columns count decisive decisions only); dr_lds50's helper paths: spec 238, many 169, single 283.

Spread cases (SPREAD_CASES; see test_decima_audit.py): the same draw times SPREAD_GAINS = (1, 1.5), 2 envs, the oracle
in float64, the lgprob held to the bar derived from the case's reference collection, the same three content
conditions. The drg_hbm shape is dr_hbm_n3: within dr_hbm_n127's first 160 decisions only a third are decisive at any
gains tried. CPU-measured (the fp32 figures move by about a quarter between hosts):
  case               decisions (per env)  decisive  exec k > 0  stage > 0  |fp32 - fp64|  |dp_tanh - fp64|  bar
  dr_lds50_spread    256 (111 / 145)      89.8%     116         214        7.93e-7        1.02e-6           1.64e-5
                     lds 256; spec 106, many 58, single 92
  dr_hbm_n3_spread   248 (142 / 106)      96.4%     174         232        8.75e-7        7.24e-7           1.40e-5
                     lds 13, global 235; 210 samples above 64 nodes
"""

import copy
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import decima_audit as A
import parity
from conftest import ENV_CFG_SMALL
from spark_sched_sim import _abi
from test_decima_audit import (CASES, DENSE50, MUT_CFG, MUT_LIMITS, MUT_SEEDS, decisions_range, seen_paths,
                               spread_reference)

POLICY_SEED, POLICY_NOISE, MAX_DECISIONS = 6, 0.1, 400
MIN_DECISIVE_SHARE, MIN_EXEC_NONZERO, MIN_STAGE_NONFIRST = 0.75, 100, 100


def greedy_unit(case: dict) -> str:
    return "drg_" + case["unit"][len("dr_"):]


policy_state = functools.partial(A.policy_state, seed=POLICY_SEED, noise=POLICY_NOISE)  # (module docstring)

# "Spread" cases (module docstring): a case of test_decima_audit.CASES with 2 envs, limits under which each env records
# 60..150 decisions, the parameters times SPREAD_GAINS, the oracle in float64 and the lgprob bar derived from the
# reference's own collection (tests/policy_strength.py).
SPREAD_GAINS = (1.0, 1.5)
SPREAD_CASES = {
    "dr_lds50_spread": dict(CASES["dr_lds50"], seeds=[700, 701], limits=[4.0e4, 3.5e4], gains=SPREAD_GAINS,
                            must=("plan_lds", "spec", "many", "single")),
    "dr_hbm_n3_spread": dict(CASES["dr_hbm_n3"], seeds=[700, 701], limits=[4.0e5, 5.0e5], gains=SPREAD_GAINS),
}
ALL_CASES = {**CASES, **SPREAD_CASES}


# ------------------------------------------------------------------------------------------ the auditor on a host arena
@pytest.fixture(scope="module")
def faithful(dataset):
    from hostsim.driver import HostEngine
    from spark_sched_sim.trainers.rollouts import DecimaSampleArena

    _, sd = policy_state(MUT_CFG["num_executors"])
    eng = HostEngine(MUT_CFG, len(MUT_SEEDS), dataset)
    arena = DecimaSampleArena(len(MUT_SEEDS), "cpu", cap_samples=8, cap_nodes=64, cap_edges=64, cap_dags=8)
    A.collect_reference(eng, arena, MUT_SEEDS, MUT_LIMITS, sd, A.Greedy())
    assert arena.caps[0] > 8 and arena.caps[1] > 64  # the regions grew
    arena = A.host_arena(arena)
    rep = A.audit(arena, MUT_CFG, dataset, MUT_SEEDS, MUT_LIMITS, sd, A.Greedy(), plan_cap=30)
    return arena, sd, rep


def test_audit_passes_on_a_faithful_arena(faithful, dataset):
    """An arena filled on the host build of the engine with the oracle's arg-max actions and log-probabilities: the
    audit passes on every sample and agrees with the engine-free reference rollout."""
    arena, sd, rep = faithful
    n = int(arena.cursor[:, _abi.CUR_SAMPLES].sum())
    assert n > 100 and rep["decisions"] == n
    ref = A.reference_rollout(MUT_CFG, dataset, MUT_SEEDS, MUT_LIMITS, sd, A.Greedy(), plan_cap=30)
    for key in ("env", "k", "stage_idx", "exec_idx", "job_idx", "nodes", "cap", "plan", "decisive"):
        assert np.array_equal(ref[key], rep[key]), key
    assert np.array_equal(ref["lgprob"].astype(np.float32), rep["lgprob"].astype(np.float32))
    assert np.array_equal(rep["stage_idx"], rep["s_win"]) and np.array_equal(rep["exec_idx"], rep["e_win"])


def _sample_scores(arena, sd, e, k):
    dobs = A.sample_observation(arena, e, k, MUT_CFG["num_executors"])
    r = A.sample_record(arena, e, k)
    return r, A.policy(sd, dobs, MUT_CFG["num_executors"], stage_of=r["stage_idx"])


def _first(arena, sd, rep, want):
    """(env, k, record, policy, target) of the first sample (past each env's start) for which want(record, policy)
    returns a target."""
    for i in range(len(rep["k"])):
        e, k = int(rep["env"][i]), int(rep["k"][i])
        if k < 5:
            continue
        r, p = _sample_scores(arena, sd, e, k)
        t = want(r, p)
        if t is not None:
            return e, k, r, p, t
    raise AssertionError("no sample to mutate")


def _mut_exec(arena, sd, rep):
    """The exec choice moved to a k whose oracle score is below the best by more than the margin."""
    def want(r, p):
        es = p.es.numpy()
        low = np.flatnonzero(es < es.max() - 1.5 * p.e_margin)
        return int(low[0]) if low.size else None

    e, k, r, p, t = _first(arena, sd, rep, want)
    arena.rec[e, k, A.I32["exec_idx"]] = t
    arena.rec[e, k, A.I32["num_exec"]] = t + 1


def _mut_stage(arena, sd, rep):
    """The stage choice moved to a stage of the SAME job (so job_idx and the exec scores stay consistent) whose oracle
    score is below the best by more than the margin."""
    from oracle import decima_gnn as G

    N = MUT_CFG["num_executors"]

    def want(r, p):
        ss = p.ss.numpy()
        dobs = A.sample_observation(arena, want.e, want.k, N)
        for s in np.flatnonzero(ss < ss.max() - 1.5 * p.s_margin):
            if G.job_of_stage(dobs, int(s)) == r["job_idx"]:
                return int(s)
        return None

    for i in range(len(rep["k"])):
        want.e, want.k = int(rep["env"][i]), int(rep["k"][i])
        if want.k < 5:
            continue
        r, p = _sample_scores(arena, sd, want.e, want.k)
        t = want(r, p)
        if t is not None:
            arena.rec[want.e, want.k, A.I32["stage_idx"]] = t
            return
    raise AssertionError("no sample to mutate")


def _mut_lgprob(arena, sd, rep):
    e, k = int(rep["env"][7]), int(rep["k"][7])
    r = A.sample_record(arena, e, k)
    arena.rec[e, k].view(np.float32)[_abi.SAMPLE_LGPROB] = np.float32(r["lgprob"] + 3e-4 * (1 + abs(r["lgprob"])))


def _mut_feature(arena, sd, rep):
    for i in range(len(rep["k"])):
        e, k = int(rep["env"][i]), int(rep["k"][i])
        r = A.sample_record(arena, e, k)
        if k >= 5 and r["num_nodes"] >= 3:
            arena.nodes[e, r["node_off"] + 2].view(np.uint32)[3] += 1  # one ulp on remaining tasks / scale
            return
    raise AssertionError("no sample to mutate")


MUTATIONS = {
    "exec_idx": (_mut_exec, "exec choice"),
    "stage_idx": (_mut_stage, "stage choice"),
    "lgprob": (_mut_lgprob, "lgprob"),
    "node_feature_ulp": (_mut_feature, "node features differ"),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_audit_fails_on_a_single_mutation(faithful, dataset, name):
    """One recorded value changed (an exec or a stage choice moved to one whose oracle score is below the margin, a
    log-probability by three times its tolerance, a feature by one ulp): the audit fails and names it."""
    arena, sd, rep = faithful
    bad = copy.deepcopy(arena)
    mutate, message = MUTATIONS[name]
    mutate(bad, sd, rep)
    with pytest.raises(parity.Mismatch, match=message):
        A.audit(bad, MUT_CFG, dataset, MUT_SEEDS, MUT_LIMITS, sd, A.Greedy())


# ------------------------------------------------------------------------------------------ the GPU cases, on the CPU
@functools.lru_cache(maxsize=None)
def _reference(name: str):
    from spark_sched_sim.data_samplers.synthetic_tpch import generate

    c = ALL_CASES[name]
    if name == "dr_hbm50":  # dr_lds50's trajectories, re-planned
        return A.replanned(_reference("dr_lds50"), c["plan_cap"])
    if "gains" in c:
        return spread_reference(c, A.Greedy(), policy=lambda N, gains: policy_state(N, gains=gains),
                                max_decisions=MAX_DECISIONS)
    _, sd = policy_state(c["env"]["num_executors"])
    return A.reference_rollout(c["env"], generate(0), c["seeds"], c["limits"], sd, A.Greedy(), plan_cap=c["plan_cap"],
                               helper=c["waves"] > 1, max_decisions=MAX_DECISIONS)


def describe(name: str, rep: dict) -> str:
    per_env = [int((rep["env"] == e).sum()) for e in sorted(set(rep["env"].tolist()))]
    return (f"{name}: decisions {rep['decisions']} {per_env}, decisive {rep['decisive_share']:.1%}, decisive with exec "
            f"winner k > 0 {rep['decisive_exec_nonzero']}, with stage winner > 0 {rep['decisive_stage_nonfirst']}, "
            f"paths {seen_paths(rep)}")


def check_case_content(c: dict, rep: dict):
    assert rep["decisive_share"] >= MIN_DECISIVE_SHARE, rep["decisive_share"]
    assert rep["decisive_exec_nonzero"] >= MIN_EXEC_NONZERO, rep["decisive_exec_nonzero"]
    assert rep["decisive_stage_nonfirst"] >= MIN_STAGE_NONFIRST, rep["decisive_stage_nonfirst"]
    seen = seen_paths(rep)
    assert all(seen[m] > 0 for m in c["must"]), seen


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_gpu_case_reference_collection(name):
    """What a correct greedy kernel records for a GPU case, from the reference alone: the three content conditions of
    the module docstring, and every path the case demands (both plans, the three helper paths, caps above 64). A
    spread case: 60..150 decisions per env, and a derived lgprob bar between its floor and the standing bar's 1e-4."""
    c = ALL_CASES[name]
    rep = _reference(name)
    print(describe(name, rep))
    check_case_content(c, rep)
    if "gains" in c:
        print(f"{name}: lgprob |fp32 - fp64| {rep['lg_err_fp32']:.3e}, |restated dp_tanh - fp64| "
              f"{rep['lg_err_act']:.3e}, derived bar {rep['lgprob_bar']:.3e}")
        assert 2e-6 <= rep["lgprob_bar"] < A.LGPROB_ATOL
        lo, hi = decisions_range(c)
        per_env = [int((rep["env"] == e).sum()) for e in range(len(c["seeds"]))]
        assert all(lo <= n <= hi for n in per_env), per_env


# ------------------------------------------------------------------------------------------ the GPU cases
def _greedy_collect(eng, params, arena, seed, counter, max_steps=None):
    """A.gpu_collect under SSIM_ROLLOUT_GREEDY; with max_steps the arena must hold the one launch. Returns the
    growths."""
    got = A.gpu_collect(eng, params, arena, seed, counter, max_steps=max_steps, flags=_abi.SSIM_ROLLOUT_GREEDY)
    assert max_steps is None or not got.full, "a capped collection's arena must not fill"
    return got.grown


def _engine(c, dataset, gpu_device, check_plan=True):
    from spark_sched_sim import native
    from spark_sched_sim.engine import DeviceEngine

    eng = DeviceEngine(c["env"], len(c["seeds"]), dataset, device=gpu_device, config_flags=c["flags"])
    name = native.lib().ssim_debug_kernel_name(eng.handle, _abi.SSIM_DEBUG_DECIMA_GREEDY).decode()
    assert name == greedy_unit(c), name
    assert native.lib().ssim_debug_kernel_name(eng.handle, _abi.SSIM_DEBUG_DECIMA).decode() == c["unit"]
    if check_plan:  # the sibling unit's plan cap and waves
        cap, waves = ct.c_int32(), ct.c_int32()
        native.check(native.lib().ssim_debug_decima_plan(eng.handle, ct.byref(cap), ct.byref(waves)), "plan")
        assert (cap.value, waves.value) == (c["plan_cap"], c["waves"])
    eng.reset_sampled(_abi.SSIM_RESET_SEED, seeds=c["seeds"], time_limits=np.array(c["limits"], dtype=np.float64))
    return eng


def _small_arena(B, device):
    from spark_sched_sim.trainers.rollouts import DecimaSampleArena

    return DecimaSampleArena(B, device, cap_samples=32, cap_nodes=1 << 10, cap_edges=1 << 10, cap_dags=1 << 7)


def _roomy_arena(B, device, samples):  # (never fills within `samples` decisions of these envs)
    from spark_sched_sim.trainers.rollouts import DecimaSampleArena

    return DecimaSampleArena(B, device, cap_samples=samples, cap_nodes=1 << 16, cap_edges=1 << 17, cap_dags=1 << 13)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_greedy_rollout_audit_gpu(gpu_device, dataset, name):
    """One SSIM_ROLLOUT_GREEDY collection of the case's unit into a small sample arena (it grows at least once), then
    the regret audit of every sample; the unit's name, the plan, the case's content and paths are asserted. A spread
    case: the oracle in float64 and the lgprob bar derived from the reference's collection of the case."""
    c = ALL_CASES[name]
    B, N = len(c["seeds"]), c["env"]["num_executors"]
    pol, sd = policy_state(N, gpu_device, gains=c.get("gains", (1.0, 1.0)))
    ref = dict(dtype=torch.float64, lgprob_bar=_reference(name)["lgprob_bar"]) if "gains" in c else {}
    eng = _engine(c, dataset, gpu_device)
    arena = _small_arena(B, eng.device)
    grown = _greedy_collect(eng, pol.packed_params(gpu_device), arena, 9, 77)
    assert grown > 0
    a = A.host_arena(arena)
    assert int(a.cursor[:, _abi.CUR_SAMPLES].max()) <= MAX_DECISIONS  # (as the reference's: the episodes end first)
    rep = A.audit(a, c["env"], dataset, c["seeds"], c["limits"], sd, A.Greedy(), plan_cap=c["plan_cap"],
                  helper=c["waves"] > 1, **ref)
    print(describe(f"{name} ({greedy_unit(c)})", rep))
    check_case_content(c, rep)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dr_lds_n10", "dr_lds50"])
def test_greedy_ignores_seed_and_counter_gpu(gpu_device, dataset, name):
    """Two greedy collections from the same resets with different (seed, counter): bit-equal arenas."""
    c = CASES[name]
    pol, _ = policy_state(c["env"]["num_executors"], gpu_device)
    params = pol.packed_params(gpu_device)
    arenas = []
    for seed, counter in ((9, 77), (123456789, 2**40 + 5)):
        eng = _engine(c, dataset, gpu_device, check_plan=False)
        arena = _roomy_arena(len(c["seeds"]), eng.device, 96)
        _greedy_collect(eng, params, arena, seed, counter, max_steps=96)
        arenas.append(A.host_arena(arena))
    assert (arenas[0].cursor[:, _abi.CUR_SAMPLES] == 96).all()
    A.arenas_equal(arenas[0], arenas[1])


def _tied_policy(num_executors, device):
    """Every score equals its bias on the device and on the oracle alike: the last linear layer's weight of the stage
    and exec score MLPs zeroed."""
    pol, _ = policy_state(num_executors)
    with torch.no_grad():
        pol.stage_policy_network.mlp_score[-1].weight.zero_()
        pol.exec_policy_network.mlp_score[-1].weight.zero_()
    return pol.to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [dict(ENV_CFG_SMALL), DENSE50], ids=["n10", "dense50"])
def test_greedy_exact_ties_gpu(gpu_device, dataset, env):
    """All-equal scores: every recorded action is (stage_idx 0, exec_idx 0), lgprob = -log(#schedulable) - log(cap)
    within 1e-4, and the trajectory equals the oracle driven with (0, 1). 4 envs, 100 decisions; DENSE50's commit caps
    exceed 16 (several exec tiles, the helper waves)."""
    from oracle.decima import decima_observation
    from oracle.restatement import SparkSchedOracle
    from spark_sched_sim.engine import DeviceEngine

    B, K, N = 4, 100, env["num_executors"]
    seeds = [700, 701, 702, 703]
    pol = _tied_policy(N, gpu_device)
    eng = DeviceEngine(env, B, dataset, device=gpu_device)
    eng.reset_sampled(_abi.SSIM_RESET_SEED, seeds=seeds)
    arena = _roomy_arena(B, eng.device, K)
    _greedy_collect(eng, pol.packed_params(gpu_device), arena, 1, 2, max_steps=K)
    a = A.host_arena(arena)
    assert (a.cursor[:, _abi.CUR_SAMPLES] == K).all()
    caps_seen = []
    for e in range(B):
        o = SparkSchedOracle(env, dataset)
        obs, _ = o.reset(seed=seeds[e], options={"time_limit": float("inf")})
        for k in range(K):
            where = f"env{e} sample{k}"
            r = A.sample_record(a, e, k)
            assert (r["stage_idx"], r["exec_idx"], r["num_exec"]) == (0, 0, 1), (where, r)
            dobs = decima_observation(obs, N)
            parity.compare_decima(dobs, A.sample_observation(a, e, k, N), where)
            assert np.float64(r["wall_before"]).tobytes() == np.float64(o.wall_time).tobytes(), where
            nsch = int(np.count_nonzero(dobs["stage_mask"]))
            cap = int(dobs["commit_caps"][r["job_idx"]])
            caps_seen.append(cap)
            assert abs(r["lgprob"] - (-np.log(nsch) - np.log(cap))) <= 1e-4, (where, r["lgprob"], nsch, cap)
            obs, rew, term, _, _ = o.step({"stage_idx": 0, "num_exec": 1})
            assert parity.reward_close(r["reward"], float(rew), o.beta, len(o.jobs)), where
            assert not term
    if N > 16:
        assert max(caps_seen) > 16


@pytest.mark.gpu
def test_greedy_flag_handling_gpu(gpu_device, dataset, env_cfg):
    """SSIM_ROLLOUT_GREEDY fails with SSIM_E_ARG and a message naming the flag: with each excluded flag, through
    ssim_decima_rollout_timed, and through ssim_rollout_ex. No launch happens: the envs stay at their reset."""
    from spark_sched_sim import native
    from spark_sched_sim.engine import DeviceEngine
    from spark_sched_sim.trainers import DeviceAsyncRolloutCollector
    from test_timed_rollouts import SMALL

    GR = _abi.SSIM_ROLLOUT_GREEDY
    cfg = dict(env_cfg, **SMALL["cfg"])
    eng = DeviceEngine(cfg, SMALL["B"], dataset, device=gpu_device)
    pol, _ = policy_state(cfg["num_executors"], gpu_device)
    col = DeviceAsyncRolloutCollector(eng, pol, SMALL["duration"], SMALL["bases"], SMALL["step"],
                                      mean_time_limit=SMALL["mean"], seed=5)
    col._reset(np.arange(SMALL["B"]))
    col._fill_schedule()
    params = pol.packed_params(gpu_device)
    for other in (_abi.SSIM_ROLLOUT_AUTORESET, _abi.SSIM_ROLLOUT_PREEMPT, _abi.SSIM_ROLLOUT_WARMUP,
                  _abi.SSIM_ROLLOUT_TEST_REJECT):
        with pytest.raises(native.NativeError, match=r"\(-1\).*SSIM_ROLLOUT_GREEDY"):
            eng.decima_rollout(params, 1, 2, 8, 16 if other == _abi.SSIM_ROLLOUT_PREEMPT else 0, flags=GR | other)
    with pytest.raises(native.NativeError, match=r"\(-1\).*ssim_rollout_ex.*SSIM_ROLLOUT_GREEDY"):
        eng.rollout(_abi.SSIM_POLICY_FAIR, 0, 8, flags=GR)
    with pytest.raises(native.NativeError, match=r"\(-1\).*ssim_decima_rollout_timed.*SSIM_ROLLOUT_GREEDY"):
        eng.decima_rollout_timed(params, 1, 2, 8, samples=col.arena, timed=col._timed(), flags=GR)
    torch.cuda.synchronize()
    assert (eng.views["counts"][:, _abi.OC_DECISIONS].cpu().numpy() == 0).all()
