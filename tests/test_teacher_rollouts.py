"""Teacher rollouts and behaviour cloning on the CPU: the host build of csrc/teacher_rollout.h's driver
(tests/hostsim/teacher.cpp, one-lane wave) records a heuristic's decisions as Decima samples; tests/teacher_audit.py
audits the arena against the oracle; trainers/imitation.py clones the teacher; PPO starts from the clone. The device
tests of the same driver are in test_gpu_teacher_rollouts.py (`-m gpu`).

Env: test_decima_audit.py's MUT_CFG (TPC-H timing, 10 executors, 8 jobs), 2 envs, seeds 11 / 12, limits 2e5 ms / none,
an arena of 8 samples / 64 node rows / 64 edge rows / 8 DAG rows per env, so every region grows. Chosen from the
reference walk alone (teacher_audit.reference_walk: the oracle under the host scheduler; test_reference_walk_counts
asserts them), decisions per env / no-op decisions:
  fair            96 / 185    8 no-ops
  sjf-cp         117 / 229    0
  wfair a = -1   111 / 184    3
  random         128 / 239    0   (no host reference: its stream is the device's; counted on the host build)
The features' scratch is in the emulated LDS up to 30 nodes (plan_cap=30): both placements occur in every case
(e.g. fair: 237 decisions in the LDS, 44 in the global workspace; 46 nodes at most).

Behaviour cloning (test_behaviour_cloning_learns_the_teacher): the sjf-cp collection above (346 samples), 16 Adam steps
(4 epochs x 4 minibatches, lr 3e-3, clip 0.5, torch seed 3); held out: seeds 21 / 22 without limits (414 samples).
Measured here: mean NLL on the collection 3.0685 before, 2.1061 after; held-out stage agreement 0.285 untrained,
0.659 trained (held-out NLL 3.275 -> 2.258, exec agreement 0.068 -> 1.000). The test asserts half the drop and half
the gain (fp32 figures move by about a quarter between hosts).
"""

import copy

import numpy as np
import pytest
import torch

import decima_audit as A
import parity
import teacher_audit as T
from spark_sched_sim import _abi

TPCH = dict(job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
MUT_CFG = dict(TPCH, num_executors=10, job_arrival_cap=8)  # test_decima_audit.MUT_CFG
SEEDS, LIMITS = [11, 12], [2.0e5, None]
HELD_SEEDS = [21, 22]
PLAN_CAP = 30
LAUNCH_SEED = 7
TEACHERS = {"fair": ("fair", None), "sjf-cp": ("sjf-cp", None), "wfair": ("wfair", -1.0), "random": ("random", None)}
COUNTS = {"fair": ([96, 185], 8), "sjf-cp": ([117, 229], 0), "wfair": ([111, 184], 3), "random": ([128, 239], 0)}
BC_NLL = (3.0685, 2.1061)      # measured: mean NLL on the collection before / after the 16 Adam steps
BC_HELD_STAGE = (0.285, 0.659)  # measured: held-out stage agreement, untrained / trained


def _engine(cfg, n, ds, **kw):
    from hostsim.teacher_driver import TeacherHostEngine

    return TeacherHostEngine(cfg, n, ds, plan_cap=PLAN_CAP, **kw)


def _small_arena():
    from spark_sched_sim.trainers.rollouts import DecimaSampleArena

    return DecimaSampleArena(len(SEEDS), "cpu", cap_samples=8, cap_nodes=64, cap_edges=64, cap_dags=8)


_cache = {}


def collection(dataset, name, resident=False):
    """The host collection of a teacher and its audit report, once per module: (torch arena, host copy, logged actions,
    report)."""
    key = (name, resident)
    if key not in _cache:
        teacher, alpha = TEACHERS[name]
        arena = _small_arena()
        got = T.collect_logged(_engine(MUT_CFG, len(SEEDS), dataset, resident=resident), arena,
                               T.kind_of(teacher, alpha), LAUNCH_SEED, SEEDS, LIMITS)
        assert got.grown > 0 and arena.caps[0] > 8 and arena.caps[1] > 64 and arena.caps[3] > 8  # the regions grew
        host = A.host_arena(arena)
        rep = T.audit(host, MUT_CFG, dataset, SEEDS, LIMITS, got.actions, teacher, alpha, plan_cap=PLAN_CAP)
        _cache[key] = (arena, host, got.actions, rep)
    return _cache[key]


@pytest.mark.parametrize("name", [n for n in TEACHERS if n != "random"])
def test_reference_walk_counts(dataset, name):
    """The module docstring's counts, from the oracle under the host scheduler alone: every env records between 40 and
    400 decisions, and fair's collection holds no-op decisions."""
    teacher, alpha = TEACHERS[name]
    rep = T.reference_walk(MUT_CFG, dataset, SEEDS, LIMITS, teacher, alpha, plan_cap=PLAN_CAP)
    per_env = [int((rep["env"] == e).sum()) for e in range(len(SEEDS))]
    print(name, per_env, int(rep["noop"].sum()))
    assert all(40 <= n <= 400 for n in per_env) and all(rep["episode_over"])
    assert (per_env, int(rep["noop"].sum())) == COUNTS[name]
    if name == "fair":
        assert rep["noop"].sum() >= 1


@pytest.mark.parametrize("resident", [False, True], ids=["hbm", "lds"])
@pytest.mark.parametrize("name", list(TEACHERS))
def test_audit_passes_for_each_teacher(dataset, name, resident):
    """The host build's collection passes the audit (the observation rows, times, rewards, the action encoding, the
    no-op encoding, the mask-validity condition, and for the deterministic teachers the host scheduler's action at every
    decision), with the hot block in place and in the emulated LDS residency; both placements of the features' scratch
    occur; the recorded counts are the reference walk's."""
    arena, host, actions, rep = collection(dataset, name, resident)
    per_env = [int((rep["env"] == e).sum()) for e in range(len(SEEDS))]
    assert (per_env, int(rep["noop"].sum())) == COUNTS[name]
    assert all(40 <= n <= 400 for n in per_env)
    assert (rep["scratch"] == "lds").any() and (rep["scratch"] == "global").any()
    assert np.array_equal(host.cursor[:, _abi.CUR_SAMPLES], per_env)
    if resident:
        A.arenas_equal(host, collection(dataset, name, False)[1])


def _pick(host, rep, cond):
    for i in range(len(rep["k"])):
        e, k = int(rep["env"][i]), int(rep["k"][i])
        r = A.sample_record(host, e, k)
        if k >= 5 and cond(i, r):
            return e, k, r
    raise AssertionError("no sample to mutate")


def _mut_job(host, rep):
    e, k, r = _pick(host, rep, lambda i, r: not rep["noop"][i] and r["num_dags"] >= 2)
    host.rec[e, k, A.I32["job_idx"]] = (r["job_idx"] + 1) % r["num_dags"]


def _mut_exec(host, rep):
    e, k, r = _pick(host, rep, lambda i, r: not rep["noop"][i])
    host.rec[e, k, A.I32["exec_idx"]] = r["exec_idx"] + 1


def _mut_noop(host, rep):
    e, k, r = _pick(host, rep, lambda i, r: bool(rep["noop"][i]) and rep["sched"][i] >= 1)
    host.rec[e, k, A.I32["stage_idx"]] = 0
    host.rec[e, k, A.I32["job_idx"]] = 0


def _mut_feature(host, rep):
    e, k, r = _pick(host, rep, lambda i, r: r["num_nodes"] >= 3)
    host.nodes[e, r["node_off"] + 2].view(np.uint32)[3] += 1  # one ulp on remaining tasks / scale


def _mut_cap(host, rep):
    e, k, r = _pick(host, rep, lambda i, r: 0 < host.dags[rep["env"][i], r["dag_off"], 1] < MUT_CFG["num_executors"])
    host.dags[e, r["dag_off"], 1] += 1


MUTATIONS = {
    "job_idx_other_dag": (_mut_job, "job_idx"),
    "exec_idx_plus_one": (_mut_exec, "exec_idx"),
    "noop_given_a_stage": (_mut_noop, "no-op recorded as"),
    "node_feature_ulp": (_mut_feature, "node features differ"),
    "commit_cap": (_mut_cap, "exec_mask differ"),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_audit_fails_on_a_single_mutation(dataset, name):
    """One recorded value of fair's collection changed: the audit fails and names the field."""
    _, host, actions, rep = collection(dataset, "fair")
    bad = copy.deepcopy(host)
    mutate, message = MUTATIONS[name]
    mutate(bad, rep)
    with pytest.raises(parity.Mismatch, match=message):
        T.audit(bad, MUT_CFG, dataset, SEEDS, LIMITS, actions, "fair", None, plan_cap=PLAN_CAP)


@pytest.mark.parametrize("name", list(TEACHERS))
def test_every_sample_is_expressible_under_decimas_masks(dataset, name):
    """The mask-validity condition the trainer checks before its first update (trainers.imitation.first_invalid: the
    chosen node schedulable, exec_idx < exec_cap[job_idx]) holds on every recorded non-no-op sample of every case, on the
    learner's own view of the arena (ArenaRolloutBuffer.samples), and fails on a sample pushed past its cap."""
    from spark_sched_sim.trainers.imitation import drop_noops, first_invalid

    arena, _, _, rep = collection(dataset, name)
    buf = arena.buffer(torch.zeros(len(SEEDS), dtype=torch.float64))
    obs, acts, keep, noops = drop_noops(*buf.samples())
    assert noops == int(rep["noop"].sum()) and obs.num_envs == len(rep["k"]) - noops
    assert np.array_equal(acts["stage_idx"].numpy(), rep["stage_idx"][~rep["noop"]])
    assert np.array_equal(acts["job_idx"].numpy(), rep["job_idx"][~rep["noop"]])
    assert first_invalid(obs, acts) == -1
    bad = {k: v.clone() for k, v in acts.items()}
    bad["exec_idx"][7] = int(rep["cap"][~rep["noop"]][7])
    assert first_invalid(obs, bad) == 7
    bad = {k: v.clone() for k, v in acts.items()}
    bad["stage_idx"][9] = int(rep["sched"][~rep["noop"]][9])
    assert first_invalid(obs, bad) == 9
    # trajectories() is complete: the no-ops keep their place, times and rewards
    times, rewards, lengths, sample = buf.trajectories()
    assert lengths.tolist() == COUNTS[name][0] and int((sample >= 0).sum()) == len(rep["k"])


def _bc(dataset, **train):
    from spark_sched_sim.trainers.imitation import BehaviourCloning

    cfg = dict(teacher="sjf-cp", num_envs=2, seeds=SEEDS, seed=3, num_iterations=1, num_epochs=4, num_batches=4,
               lr=3e-3, max_grad_norm=0.5, **train)
    return BehaviourCloning({"embed_dim": 16}, MUT_CFG, cfg, engine_factory=_engine, dataset=dataset, device="cpu")


def test_behaviour_cloning_learns_the_teacher(dataset, tmp_path):
    """16 Adam steps on the host-collected sjf-cp episodes of seeds 11 / 12 (module docstring): the mean NLL on the
    collection drops by at least half the measured drop, and the stage agreement on the held-out seeds 21 / 22 rises by
    at least half the measured gain. The clone survives save / load bit for bit."""
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers.imitation import drop_noops

    bc = _bc(dataset)
    held = bc.collector.collect(HELD_SEEDS)
    obs, acts, _, _ = drop_noops(*held.samples())
    untrained = bc.evaluate(obs, acts)
    (rec,) = bc.train(log=None)
    trained = bc.evaluate(obs, acts)
    print(f"nll {rec['nll_before']:.4f} -> {rec['nll_after']:.4f} over {rec['samples']} samples (+{rec['noop_samples']} "
          f"no-ops), {rec['adam_steps']} Adam steps; held out ({obs.num_envs} samples): stage agreement "
          f"{untrained['stage_agreement']:.3f} -> {trained['stage_agreement']:.3f}, exec agreement "
          f"{untrained['exec_agreement']:.3f} -> {trained['exec_agreement']:.3f}, nll {untrained['nll']:.3f} -> "
          f"{trained['nll']:.3f}")
    assert rec["adam_steps"] == 16 and rec["samples"] == sum(COUNTS["sjf-cp"][0]) and rec["noop_samples"] == 0
    for key in ("nll_before", "nll_after", "stage_agreement", "exec_agreement", "samples", "noop_samples",
                "seconds_collect", "seconds_learn"):
        assert key in rec
    assert rec["nll_before"] - rec["nll_after"] >= 0.5 * (BC_NLL[0] - BC_NLL[1])
    assert trained["stage_agreement"] - untrained["stage_agreement"] >= 0.5 * (BC_HELD_STAGE[1] - BC_HELD_STAGE[0])
    path = tmp_path / "clone.pt"
    bc.scheduler.save(path)
    again = DecimaScheduler.load(path)
    assert torch.equal(again.packed_params("cpu"), bc.scheduler.packed_params("cpu"))


def test_loss_refuses_noop_samples(dataset):
    """A loss taken over the no-op rows too is caught by the explicit check of BehaviourCloning._loss (evaluate_actions
    itself would index job_idx = -1 into the previous sample's DAGs without an error); with the no-ops dropped the same
    call returns the NLL. A trainer fed an arena with an action outside Decima's masks raises, naming env and sample."""
    from spark_sched_sim.trainers.imitation import drop_noops

    arena, _, _, rep = collection(dataset, "fair")
    buf = arena.buffer(torch.zeros(len(SEEDS), dtype=torch.float64))
    obs_all, acts_all = buf.samples()
    bc = _bc(dataset)
    first = int(np.flatnonzero(rep["noop"])[0])
    with pytest.raises(ValueError, match=f"sample {first} is a no-op"):
        bc._loss(obs_all, acts_all)
    obs, acts, _, noops = drop_noops(obs_all, acts_all)
    assert noops == COUNTS["fair"][1] and torch.isfinite(bc._loss(obs, acts))
    bad = copy.deepcopy(arena)
    e, k = 1, 20
    assert not rep["noop"][(rep["env"] == e) & (rep["k"] == k)][0]
    bad.rec[e, k, A.I32["exec_idx"]] = MUT_CFG["num_executors"]
    with pytest.raises(ValueError, match=f"env {e} sample {k} .*not expressible"):
        bc.train_on_buffer(bad.buffer(torch.zeros(len(SEEDS), dtype=torch.float64)))


def test_ppo_starts_from_the_saved_clone(dataset, tmp_path):
    """agent_cfg["init_checkpoint"]: a PPO built from a saved clone holds the clone's parameters bit for bit before its
    first update, and differs from a PPO without it."""
    from spark_sched_sim.trainers import PPO

    bc = _bc(dataset, )
    bc.train(log=None)
    path = tmp_path / "clone.pt"
    bc.scheduler.save(path)
    train = dict(num_sequences=1, num_rollouts=2, seed=5, num_epochs=1, num_batches=2, beta_discount=5e-3,
                 opt_kwargs={"lr": 3e-4}, max_grad_norm=0.5)
    env = dict(MUT_CFG, mean_time_limit=4e5)
    ppo = PPO({"embed_dim": 16, "init_checkpoint": str(path)}, env, train, engine_factory=_engine, dataset=dataset,
              device="cpu")
    for (name, p), (_, q) in zip(ppo.scheduler.named_parameters(), bc.scheduler.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), name
    plain = PPO({"embed_dim": 16}, env, train, engine_factory=_engine, dataset=dataset, device="cpu")
    assert not torch.equal(plain.scheduler.packed_params("cpu"), ppo.scheduler.packed_params("cpu"))
    hist = ppo.train(1, log=None)  # and it trains from there
    assert len(hist) == 1 and np.isfinite(hist[0]["policy loss"])
    assert not torch.equal(ppo.scheduler.packed_params("cpu"), bc.scheduler.packed_params("cpu"))


def test_sample_arena_known_answers():
    """csrc/sample_arena.h (the one writer behind the Decima and teacher rollouts) on the one-lane wave, no engine:
    room check, push, reward write-back and take-back on env 1 of a hand-made two-env observation arena (3 nodes,
    2 edges, 2 DAGs; row caps 4 / 3 / 3) and a sample arena of 2 samples / 6 node / 4 edge / 3 DAG rows per env."""
    import ctypes as ct

    from hostsim import teacher_driver
    from spark_sched_sim.trainers.rollouts import DecimaSampleArena

    B, S, E, J = 2, 4, 3, 3
    counts = np.zeros((B, _abi.NUM_COUNTS), np.int32)
    nodes, links = np.zeros((B, S, 3), np.float32), np.zeros((B, E, 2), np.int64)
    dag_ptr, reward = np.zeros((B, J + 1), np.int32), np.zeros(B, np.float64)
    feats, ccap = np.zeros((B, S, 5), np.float32), np.zeros((B, J), np.int32)
    emask, depth = np.zeros((B, E), np.uint32), np.zeros(B, np.int32)
    obs_parts = [counts, nodes, links, dag_ptr, reward]  # (every part a multiple of 8 bytes: the offsets stay aligned)
    ob = np.cumsum([0] + [p.nbytes for p in obs_parts[:-1]]).astype(np.int64)
    caps = np.array([S, E, J], np.int32)
    arena = DecimaSampleArena(B, "cpu", cap_samples=2, cap_nodes=6, cap_edges=4, cap_dags=3)
    ptr = lambda a: a.ctypes.data  # noqa: E731

    def observe(base):  # env 1's observation, every value marked by `base`
        counts[1, [_abi.OC_NUM_NODES, _abi.OC_NUM_EDGES, _abi.OC_NUM_JOBS]] = 3, 2, 2
        nodes[1, :3] = [[base + 1, base + 2, 1.0], [base + 3, base + 4, 0.0], [base + 5, base + 6, 1.0]]
        links[1, :2] = [[0, 1], [2, 0]] if base else [[0, 1], [1, 2]]
        dag_ptr[1, :3] = [0, 2, 3] if base else [0, 1, 3]
        feats[1, :3] = base + 10.0 * np.arange(3)[:, None] + np.arange(5)[None, :]
        ccap[1, :2] = [base + 4, base + 7]
        emask[1, :2] = [base + 1, base + 2]
        depth[1] = 2 + (base != 0)

    def op(code, eid=1, act=(0, 0, 0, 0), lgprob=0.0, wall=0.0):
        obs = np.frombuffer(b"".join(p.tobytes() for p in obs_parts), np.uint8)
        st, a = arena.struct(), np.array(act, np.int32)
        return teacher_driver.lib().hs_arena_op(code, ct.byref(st), eid, ptr(obs), ptr(ob), ptr(caps), ptr(feats),
                                                ptr(ccap), ptr(emask), ptr(depth), ptr(a), lgprob, wall)

    def cursor(e=1):
        return arena.cursor[e].tolist()

    def record(k, e=1):
        r = arena.rec[e, k]
        f = {name: int(r[i]) for i, name in enumerate(_abi.SAMPLE_I32)}
        f64 = r.view(torch.float64)
        return f, float(r[_abi.SAMPLE_LGPROB:_abi.SAMPLE_LGPROB + 1].view(torch.float32)), \
            float(f64[_abi.SAMPLE_WALL]), float(f64[_abi.SAMPLE_REWARD])

    def rows_of(base, links_, sizes):  # the node, edge and DAG rows arena_push writes for observe(base)
        x = np.concatenate([base + 10.0 * np.arange(3)[:, None] + np.arange(5)[None, :], [[1.0], [0.0], [1.0]]], axis=1)
        ed = [[links_[0][0], links_[0][1], base + 1, 0], [links_[1][0], links_[1][1], base + 2, 0]]
        return x.astype(np.float32), np.array(ed, np.int32), np.array([[sizes[0], base + 4], [sizes[1], base + 7]], np.int32)

    def check_rows(at, want):
        cn, ce, cg = at
        assert np.array_equal(arena.nodes[1, cn:cn + 3].numpy(), want[0])  # the 5 feature columns, the flag column
        assert np.array_equal(arena.edges[1, ce:ce + 2].numpy(), want[1])  # links, the edge mask word, 0
        assert np.array_equal(arena.dags[1, cg:cg + 2].numpy(), want[2])   # DAG sizes, executor caps

    # 1. the first push
    observe(0)
    assert op(0) == 1 and cursor() == [0] * 8
    op(1, act=(1, 0, 2, 3), lgprob=-0.5, wall=10.0)
    assert cursor() == [1, 3, 2, 2, 0, 0, 0, 0]
    first = ({"num_nodes": 3, "num_edges": 2, "num_dags": 2, "depth": 2, "node_off": 0, "edge_off": 0, "dag_off": 0,
              "stage_idx": 1, "job_idx": 0, "exec_idx": 2, "num_exec": 3}, -0.5, 10.0, 0.0)
    got = record(0)
    assert {k: got[0][k] for k in first[0]} == first[0] and got[1:] == first[1:]
    rows0 = rows_of(0, [[0, 1], [1, 2]], [1, 2])
    check_rows((0, 0, 0), rows0)
    # 2. the second observation does not fit (2 + 2 DAG rows > 3): the full mark and the needs, nothing else moves
    observe(100)
    assert op(0) == 0
    assert cursor() == [1, 3, 2, 2, 1, 3, 2, 2]
    assert DecimaSampleArena.required(arena.cursor.numpy()) == [2, 6, 4, 4]
    # 3. the DAG region grown to exactly what is needed: the push fills every region to its cap
    arena.dags, arena.caps[3] = DecimaSampleArena._grown(arena.dags, 4), 4
    arena.cursor[:, _abi.CUR_FULL:] = 0
    assert op(0) == 1 and cursor() == [1, 3, 2, 2, 0, 0, 0, 0]
    op(1, act=(-1, -1, 0, 5), lgprob=0.0, wall=20.0)
    assert cursor() == [2, 6, 4, 4, 0, 0, 0, 0]
    got = record(1)
    assert (got[0]["node_off"], got[0]["edge_off"], got[0]["dag_off"], got[0]["depth"]) == (3, 2, 2, 3)
    assert (got[0]["stage_idx"], got[0]["job_idx"], got[0]["exec_idx"], got[0]["num_exec"]) == (-1, -1, 0, 5)
    assert got[1:] == (0.0, 20.0, 0.0)
    check_rows((3, 2, 2), rows_of(100, [[0, 1], [2, 0]], [2, 1]))
    check_rows((0, 0, 0), rows0)
    assert op(0) == 0 and cursor() == [2, 6, 4, 4, 1, 3, 2, 2]  # (no third sample)
    arena.cursor[:, _abi.CUR_FULL:] = 0
    # 4. the reward lands in the last record only
    reward[1] = -7.25
    op(2)
    assert record(1)[3] == -7.25 and record(0)[3] == 0.0
    # 5. the take-back restores the cursor after the first push; record 0 and its rows stay
    op(3)
    assert cursor() == [1, 3, 2, 2, 0, 0, 0, 0]
    got = record(0)
    assert {k: got[0][k] for k in first[0]} == first[0] and got[1:] == first[1:]
    check_rows((0, 0, 0), rows0)
    # 6. a take-back on an empty cursor is a no-op; env 0 was never written
    op(3, eid=0)
    assert cursor(0) == [0] * 8
    assert not arena.rec[0].any() and not arena.nodes[0].any() and not arena.edges[0].any() and not arena.dags[0].any()
