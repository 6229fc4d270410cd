"""Teacher rollouts on the device (`-m gpu`): ssim_teacher_rollout's two kernel units (tr_lds, tr_hbm) audited against
the oracle (tests/teacher_audit.py), compared bit for bit with the host build of the same driver
(tests/hostsim/teacher.cpp) and with the plain heuristic rollout; the refused arguments; one behaviour-cloning
minibatch on the device against the CPU learner; BehaviourCloning end to end.

Cases: `small` = ENV_CFG_SMALL with 8 jobs (test_teacher_rollouts.py's env, seeds and limits), `n20` = test_decima_
audit.py's dr_lds_n20 env (20 executors, 30 jobs at 2e-4 jobs / ms, 2 envs, limits 1e5 ms), whose observations pass 64
nodes and 16 DAGs: both placements of the features' scratch and the multi-round loops over more than 64 nodes occur
there (asserted from the recorded sizes). Arena of 32 samples / 1024 node rows / 1024 edge rows / 128 DAG rows per env:
it grows.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

import cases_priority as P
import decima_audit as A
import teacher_audit as T
from conftest import ENV_CFG_SMALL
from spark_sched_sim import _abi

pytestmark = pytest.mark.gpu

TPCH = dict(job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
SMALL = dict(ENV_CFG_SMALL, job_arrival_cap=8)
N20 = dict(TPCH, num_executors=20, job_arrival_cap=30, job_arrival_rate=2.0e-4)
HBM = _abi.SSIM_CFG_FORCE_HBM
LAUNCH_SEED = 7
ENVS = {"small": (SMALL, [11, 12], [2.0e5, None]), "n20": (N20, [700, 701], [1.0e5, 1.0e5])}
# (unit, config flags, env, teacher, alpha)
CASES = {
    "tr_lds-small-fair": ("tr_lds", 0, "small", "fair", None),
    "tr_lds-small-random": ("tr_lds", 0, "small", "random", None),
    "tr_hbm-small-sjf-cp": ("tr_hbm", HBM, "small", "sjf-cp", None),
    "tr_hbm-small-wfair": ("tr_hbm", HBM, "small", "wfair", -1.0),
    "tr_lds-n20-wfair": ("tr_lds", 0, "n20", "wfair", -1.0),
    "tr_lds-n20-sjf-cp": ("tr_lds", 0, "n20", "sjf-cp", None),
    "tr_hbm-n20-fair": ("tr_hbm", HBM, "n20", "fair", None),
    "tr_hbm-n20-random": ("tr_hbm", HBM, "n20", "random", None),
}


def _engine(device, env, B, dataset, flags):
    from spark_sched_sim.engine import DeviceEngine

    return DeviceEngine(env, B, dataset, device=device, config_flags=flags)


def _arena(B, device):
    from spark_sched_sim.trainers.rollouts import DecimaSampleArena

    return DecimaSampleArena(B, device, cap_samples=32, cap_nodes=1 << 10, cap_edges=1 << 10, cap_dags=1 << 7)


def _plan(eng):
    from spark_sched_sim import native

    cap, dags = ct.c_int32(), ct.c_int32()
    native.check(native.lib().ssim_debug_teacher_plan(eng.handle, ct.byref(cap), ct.byref(dags)), "teacher plan")
    assert dags.value == A.LDS_PLAN_DAGS
    return cap.value


def _unit(eng) -> str:
    from spark_sched_sim import native

    return native.lib().ssim_debug_kernel_name(eng.handle, _abi.SSIM_DEBUG_TEACHER).decode()


@pytest.mark.parametrize("name", list(CASES))
def test_teacher_rollout_audit_gpu(gpu_device, dataset, name):
    """One launch per growth step into a small arena, then the audit of tests/teacher_audit.py: every observation row
    bit for bit, wall times, rewards, the action and no-op encoding, the mask-validity condition, offsets and counts,
    and for the deterministic teachers the host scheduler's action at every decision. The unit is asserted; on the n20
    env both scratch placements and observations of more than 64 nodes occur."""
    unit, flags, env_name, teacher, alpha = CASES[name]
    env, seeds, limits = ENVS[env_name]
    eng = _engine(gpu_device, env, len(seeds), dataset, flags)
    assert _unit(eng) == unit
    cap = _plan(eng)
    arena = _arena(len(seeds), eng.device)
    got = T.collect_logged(eng, arena, T.kind_of(teacher, alpha), LAUNCH_SEED, seeds, limits)
    torch.cuda.synchronize()
    assert got.grown > 0 and got.launches == got.grown + 1, got
    rep = T.audit(A.host_arena(arena), env, dataset, seeds, limits, got.actions, teacher, alpha, plan_cap=cap)
    per_env = [int((rep["env"] == e).sum()) for e in range(len(seeds))]
    placed = {p: int((rep["scratch"] == p).sum()) for p in ("lds", "global")}
    print(f"{name}: decisions per env {per_env}, no-ops {int(rep['noop'].sum())}, plan cap {cap}, scratch {placed}, "
          f"largest observation {int(rep['nodes'].max())} nodes / {int(rep['dags'].max())} DAGs, launches {got.launches}")
    assert all(n >= 40 for n in per_env)
    if env_name == "n20":
        assert placed["lds"] > 0 and placed["global"] > 0, placed
        assert int((rep["nodes"] > 64).sum()) > 0 and int(rep["dags"].max()) > A.LDS_PLAN_DAGS
    if teacher == "fair":
        assert rep["noop"].sum() >= 1


@pytest.mark.parametrize("name", ["tr_lds-n20-wfair", "tr_hbm-n20-random"])
def test_device_arena_equals_host_build(gpu_device, dataset, name):
    """The device arena equals the arena of the host build of the same driver (one-lane wave) bit for bit
    (decima_audit.arenas_equal), one case per residency. Every record word but the reward is asserted equal first, and
    the differing words and the rewards' distance are printed.

    The reward is the one field whose bits depend on the wave's width: the engine adds a step's job times per lane and
    then over the 64 lanes on the device (engine.h jobtime, W::sum_d), serially on a one-lane wave. The host build
    therefore records the reward in the device's summation order (tests/hostsim/teacher.cpp wave_order_reward: the same
    terms, lane partial sums, the xor butterfly). With the serial order, one of the 401 rewards of tr_lds-n20-wfair
    differed from the device's, by 1 ulp."""
    from hostsim.teacher_driver import TeacherHostEngine

    unit, flags, env_name, teacher, alpha = CASES[name]
    env, seeds, limits = ENVS[env_name]
    kind = T.kind_of(teacher, alpha)
    eng = _engine(gpu_device, env, len(seeds), dataset, flags)
    assert _unit(eng) == unit
    dev_arena = _arena(len(seeds), eng.device)
    dev = T.collect_logged(eng, dev_arena, kind, LAUNCH_SEED, seeds, limits)
    host_eng = TeacherHostEngine(env, len(seeds), dataset, resident=flags == 0, plan_cap=_plan(eng))
    host_arena = _arena(len(seeds), "cpu")
    host = T.collect_logged(host_eng, host_arena, kind, LAUNCH_SEED, seeds, limits)
    for a, b in zip(dev.actions, host.actions):
        assert np.array_equal(a, b)
    da, ha = A.host_arena(dev_arena), A.host_arena(host_arena)
    assert np.array_equal(da.cursor, ha.cursor)
    # the figures first: which record words differ, and by how much where it is the reward
    for e in range(len(seeds)):
        ns = int(da.cursor[e, _abi.CUR_SAMPLES])
        diff = np.argwhere(da.rec[e, :ns] != ha.rec[e, :ns])
        words = sorted(set(diff[:, 1].tolist()))
        rd = da.rec[e, :ns].view(np.float64)[:, _abi.SAMPLE_REWARD]
        rh = ha.rec[e, :ns].view(np.float64)[:, _abi.SAMPLE_REWARD]
        ulps = np.abs(rd.view(np.int64) - rh.view(np.int64))
        print(f"{name} env {e}: {len(set(diff[:, 0].tolist()))} of {ns} records differ, in words {words} (reward = "
              f"words {2 * _abi.SAMPLE_REWARD}, {2 * _abi.SAMPLE_REWARD + 1}); rewards differ in {int((ulps > 0).sum())} "
              f"samples, by at most {int(ulps.max(initial=0))} ulp")
        other = [w for w in words if w not in (2 * _abi.SAMPLE_REWARD, 2 * _abi.SAMPLE_REWARD + 1)]
        assert not other, f"env {e}: record words {other} differ"
    A.arenas_equal(da, ha)


def _obs_arenas_equal(a, b, where):
    """Two engines' obs arenas hold the same observations: per env every scalar word (the 16 counts, reward, wall time,
    the accumulators) and every LIVE row of every row array (nodes, frontier, sched_rank over the env's num_nodes,
    edge_links over num_edges, dag_ptr over num_jobs + 1, exec_supplies over num_jobs), all as bit patterns. Rows past an
    env's live counts are not part of its observation: an eager engine (the teacher's, which rewrites rows at every
    decision) and a lazy one (the plain rollout's, which writes them once when the env leaves the launch) leave
    different stale rows of EARLIER observations there, so the raw bytes of the two arenas differ by design."""
    va, vb = a.host_views(), b.host_views()
    for key in ("counts", "acc"):
        assert np.array_equal(va[key], vb[key]), f"{where}: {key}"
    for key in ("reward", "wall_time"):
        assert np.array_equal(va[key].view(np.int64), vb[key].view(np.int64)), f"{where}: {key}"
    for e in range(a.num_envs):
        c = va["counts"][e]
        n, ne, nj = int(c[_abi.OC_NUM_NODES]), int(c[_abi.OC_NUM_EDGES]), int(c[_abi.OC_NUM_JOBS])
        for key, m in (("nodes", n), ("frontier", n), ("sched_rank", n), ("edge_links", ne), ("dag_ptr", nj + 1),
                       ("exec_supplies", nj)):
            x, y = np.ascontiguousarray(va[key][e, :m]), np.ascontiguousarray(vb[key][e, :m])
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{where}: env {e} {key}"
    return [int(va["counts"][e][_abi.OC_NUM_NODES]) for e in range(a.num_envs)]


MID = 30  # decisions per env of the first launch: every episode is still running (they take 96 or more)


@pytest.mark.parametrize("flags", [0, HBM], ids=["lds", "hbm"])
@pytest.mark.parametrize("teacher,alpha", [("fair", None), ("sjf-cp", None), ("wfair", -1.0), ("random", None)])
def test_actions_equal_the_plain_rollout(gpu_device, dataset, flags, teacher, alpha):
    """The teacher launch takes the decisions eng.rollout(kind) takes from the same reset on a fresh engine: the action
    logs are identical and the obs arenas hold the same observations (_obs_arenas_equal), after a first launch of 30
    decisions per env (observations in mid-episode) and after a second to the end of every episode, where the job tables
    are identical too."""
    from spark_sched_sim.trainers.rollouts import DecimaSampleArena

    env, seeds, _ = ENVS["small"]
    B = len(seeds)
    kind = T.kind_of(teacher, alpha)
    eng = _engine(gpu_device, env, B, dataset, flags)
    plain = _engine(gpu_device, env, B, dataset, flags)
    arena = DecimaSampleArena(B, eng.device)  # (large enough for these episodes: no launch stops on a full arena)
    for e_ in (eng, plain):
        e_.reset_sampled(_abi.SSIM_RESET_SEED, seeds=np.asarray(seeds, dtype=np.uint64))
    # first launch: MID decisions per env
    tlog, plog = eng.alloc_action_log(MID), plain.alloc_action_log(MID)
    eng.teacher_rollout(kind, LAUNCH_SEED, MID, arena, action_log=tlog)
    plain.rollout(kind, LAUNCH_SEED, MID, plog)
    torch.cuda.synchronize()
    assert arena.cursor[:, _abi.CUR_SAMPLES].tolist() == [MID] * B and not arena.cursor[:, _abi.CUR_FULL].any()
    assert np.array_equal(tlog.cpu().numpy(), plog.cpu().numpy())
    live = _obs_arenas_equal(eng, plain, "mid-episode")
    assert all(n > 0 for n in live), live
    # second launch: to the end of every episode
    tlog, plog = eng.alloc_action_log(T.LOG_STEPS), plain.alloc_action_log(T.LOG_STEPS)
    eng.teacher_rollout(kind, LAUNCH_SEED, T.LOG_STEPS, arena, action_log=tlog)
    torch.cuda.synchronize()
    assert not arena.cursor[:, _abi.CUR_FULL].any()
    counts = (arena.cursor[:, _abi.CUR_SAMPLES].cpu().numpy() - MID).tolist()
    assert all(10 <= n < T.LOG_STEPS for n in counts), counts
    plain.rollout_steps(kind, LAUNCH_SEED, counts, T.LOG_STEPS, plog)
    torch.cuda.synchronize()
    tl, pl = tlog.cpu().numpy(), plog.cpu().numpy()
    for e, n in enumerate(counts):
        assert np.array_equal(tl[:n, e], pl[:n, e]), f"env {e}"
    for a, b in zip(eng.job_times_np(), plain.job_times_np()):
        assert np.array_equal(a, b)
    _obs_arenas_equal(eng, plain, "end of episode")
    assert (eng.host_views()["counts"][:, _abi.OC_TERMINATED] != 0).all()


def test_refused_arguments(gpu_device, dataset):
    """Each refused argument returns SSIM_E_ARG with its message and leaves the obs arena and the sample arena
    untouched."""
    from spark_sched_sim import native

    env, seeds, _ = ENVS["small"]
    eng = _engine(gpu_device, env, len(seeds), dataset, 0)
    eng.reset_sampled(_abi.SSIM_RESET_SEED, seeds=np.asarray(seeds, dtype=np.uint64))
    arena = _arena(len(seeds), eng.device)
    st = arena.struct()
    ws = eng.decima_workspace()
    L = native.lib()
    before = eng.snapshot_obs()

    def call(kind=_abi.SSIM_POLICY_FAIR, flags=0, samples=st, ws_bytes=None, h=eng.handle):
        return L.ssim_teacher_rollout(h, kind, 0, 200.0, 1e5, 16, flags, ws.data_ptr(),
                                      ws.numel() if ws_bytes is None else ws_bytes,
                                      None if samples is None else ct.byref(samples), None, eng._stream())

    for flag in (_abi.SSIM_ROLLOUT_AUTORESET, _abi.SSIM_ROLLOUT_PREEMPT, _abi.SSIM_ROLLOUT_WARMUP,
                 _abi.SSIM_ROLLOUT_GREEDY):
        assert call(flags=flag) == -1
        assert b"flags must be 0" in L.ssim_last_error()
    assert call(kind=6) == -1
    assert L.ssim_last_error() == b"ssim_rollout: unknown policy 6"
    assert L.ssim_rollout(eng.handle, 6, 0, 4, None, eng._stream()) == -1
    assert L.ssim_last_error() == b"ssim_rollout: unknown policy 6"  # (the same message)
    assert call(kind=_abi.SSIM_POLICY_WFAIR_BASE + 9) == -1
    assert b"weighted fair is 0x100..0x108" in L.ssim_last_error()
    assert call(samples=None) == -1
    assert b"needs a sample arena" in L.ssim_last_error()
    assert call(ws_bytes=16) == -1
    assert b"ssim_decima_workspace_bytes" in L.ssim_last_error()
    with pytest.raises(native.NativeError, match="flags must be 0"):
        eng.teacher_rollout(_abi.SSIM_POLICY_FAIR, 0, 16, arena, flags=_abi.SSIM_ROLLOUT_AUTORESET)
    torch.cuda.synchronize()
    assert (eng.snapshot_obs() == before).all() and int(arena.cursor.abs().sum()) == 0
    # more than 32 stages per job: the edge-mask word (as ssim_decima_features); SJF-CP keeps its own refusal
    wide = _engine(gpu_device, P.wide_cfg(dict(ENV_CFG_SMALL)), 2, P.datasets("wide70"), 0)
    assert wide.cfg.max_stages == 70
    wide.reset(seeds=[5, 6])
    wws = wide.decima_workspace()
    before = wide.snapshot_obs()

    def wcall(kind):
        return L.ssim_teacher_rollout(wide.handle, kind, 0, 200.0, 1e5, 16, 0, wws.data_ptr(), wws.numel(), ct.byref(st),
                                      None, wide._stream())

    assert wcall(_abi.SSIM_POLICY_FAIR) == -1
    assert b"max_stages 70 > 32 (edge-mask word)" in L.ssim_last_error()
    assert wcall(_abi.SSIM_POLICY_SJF_CP) == -1
    assert b"at most 64 stages" in L.ssim_last_error()
    torch.cuda.synchronize()
    assert (wide.snapshot_obs() == before).all() and int(arena.cursor.abs().sum()) == 0


def _batch_to(b, device):
    import dataclasses

    return type(b)(**{f.name: (getattr(b, f.name).to(device) if isinstance(getattr(b, f.name), torch.Tensor)
                               else getattr(b, f.name)) for f in dataclasses.fields(b)})


def test_bc_minibatch_matches_cpu_learner(gpu_device, dataset):
    """One behaviour-cloning minibatch on the device from a device-collected arena, and the same minibatch on the CPU
    from the same arena copied to the host, from the same parameters: the losses agree within 1e-5 relative and every
    parameter's gradient within 1e-4 of the tensor's gradient scale, floored at 1e-2 of the largest gradient (the bar
    of test_trainers.py::test_gpu_learner_matches_cpu_learner for the first minibatch)."""
    from spark_sched_sim.schedulers.decima import DecimaScheduler, select_envs
    from spark_sched_sim.trainers.imitation import BehaviourCloning, drop_noops

    env, seeds, _ = ENVS["n20"]
    cfg = dict(teacher="fair", num_envs=2, seeds=seeds, seed=3, num_epochs=1, num_batches=3, lr=1e-3, max_grad_norm=0.5)
    bc = BehaviourCloning({"embed_dim": 16}, env, cfg, dataset=dataset, device=gpu_device)
    buf = bc.collector.collect(seeds, [1.0e5, 1.0e5])
    obs, acts, _, noops = drop_noops(*buf.samples())
    n = obs.num_envs
    assert n > 100 and noops > 0
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1000))[: n // 3 + 1]
    cpu = DecimaScheduler(env["num_executors"], embed_dim=16)
    cpu.load_state_dict({k: v.detach().cpu().clone() for k, v in bc.scheduler.state_dict().items()})
    gpu_sched = bc.scheduler
    gpu_sched.train()
    cpu.train()
    di = idx.to(obs.x.device)
    lg = bc._loss(select_envs(obs, di), {k: v[di] for k, v in acts.items()})
    gpu_sched.zero_grad()
    lg.backward()
    bc.scheduler = cpu
    obs_c, acts_c = _batch_to(obs, "cpu"), {k: v.cpu() for k, v in acts.items()}
    lc = bc._loss(select_envs(obs_c, idx), {k: v[idx] for k, v in acts_c.items()})
    cpu.zero_grad()
    lc.backward()
    assert abs(float(lg) - float(lc)) <= 1e-5 * max(1.0, abs(float(lc))), (float(lg), float(lc))
    G = max(float(p.grad.abs().max()) for p in cpu.parameters())
    worst = 0.0
    for (pname, pg), (_, pc) in zip(gpu_sched.named_parameters(), cpu.named_parameters()):
        a, b = pg.grad.detach().cpu(), pc.grad.detach()
        rel = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-2 * G)
        worst = max(worst, rel)
        assert rel <= 1e-4, f"{pname} gradient: max |gpu - cpu| / scale = {rel:.2e}"
    print(f"BC minibatch of {idx.numel()} of {n} samples: loss gpu {float(lg):.6f} cpu {float(lc):.6f}, gradients worst "
          f"{worst:.2e}")


def test_behaviour_cloning_end_to_end(gpu_device, dataset):
    """BehaviourCloning with 4 envs and one iteration on the small env, then evaluate_policy with the clone on 4 seeds:
    it terminates with no error bits (evaluate_policy raises on any) and all jobs completed. No claim about the
    score."""
    from spark_sched_sim.evaluate import evaluate_policy
    from spark_sched_sim.trainers.imitation import BehaviourCloning

    cfg = dict(teacher="wfair", alpha=-1.0, num_envs=4, seed=11, num_iterations=1, num_epochs=2, num_batches=4, lr=3e-3,
               max_grad_norm=0.5)
    bc = BehaviourCloning({"embed_dim": 16}, SMALL, cfg, dataset=dataset, device=gpu_device)
    (rec,) = bc.train(log=None)
    print(rec)
    assert rec["samples"] > 100 and rec["adam_steps"] == 8 and np.isfinite(rec["nll_after"])
    assert rec["nll_after"] < rec["nll_before"]
    out = evaluate_policy(SMALL, "decima", [31, 32, 33, 34], device=gpu_device, dataset=dataset, policy=bc.scheduler)
    assert (out["completed_jobs"] == SMALL["job_arrival_cap"]).all()
    assert np.isfinite(out["avg_job_duration"]).all()
