"""The layers above the greedy kernel, on the CPU: DecimaScheduler.schedule(greedy=True) (the batched torch path),
checkpoints (DecimaScheduler.save / load) and `examples --sched decima`."""

import numpy as np
import pytest
import torch

from spark_sched_sim.schedulers import decima as D
from spark_sched_sim.schedulers.decima import DecimaScheduler


def _policy(num_executors=10, seed=6, noise=0.1):
    torch.manual_seed(seed)
    pol = DecimaScheduler(num_executors)
    for p in pol.parameters():
        p.data.add_(noise * torch.randn_like(p))
    return pol


def _observations(dataset, env_cfg, count, seed=31):
    """`count` Decima observations of the one-env facade (host build), the env driven by the fair scheduler."""
    from hostsim.driver import HostEngine
    from spark_sched_sim.decima import DecimaObsWrapper
    from spark_sched_sim.env import SparkSchedSimEnv
    from spark_sched_sim.schedulers import host_scheduler

    env = SparkSchedSimEnv(env_cfg, dataset, _engine_factory=lambda cfg, ds: HostEngine(cfg, 1, ds))
    wrap = DecimaObsWrapper(env)
    sched = host_scheduler("fair", env_cfg["num_executors"])
    obs, _ = env.reset(seed=seed, options=None)
    out = []
    while len(out) < count:
        out.append(wrap.observation(obs))
        action, _ = sched.schedule(obs)
        obs, _, term, trunc, _ = env.step(action)
        assert not (term or trunc)
    env.close()
    return out


def _scores(pol, b):
    """schedule's own scores: stage scores of the schedulable rows, and the exec scores of a DAG."""
    with torch.no_grad():
        h = pol.encoder(b, per_obs_no_mp=True)
        ss = pol.stage_policy_network.scores_all(b, h)

        def exec_scores(dag):
            es, valid = pol.exec_policy_network.scores_grid(b, h, torch.tensor([dag]), torch.tensor([0]))
            return es[0].detach(), valid[0]

    return ss.detach(), exec_scores


def test_schedule_greedy_is_the_argmax_of_its_scores(dataset, env_cfg):
    """On 50 observations of the N = 10 env: schedule(greedy=True) returns the first arg-max of schedule's own stage
    scores over the schedulable stages and of the exec scores below the chosen DAG's commit cap, with lgprob the
    log-softmax at that pair; a sampled call returns the same keys."""
    pol = _policy(env_cfg["num_executors"])
    picked_exec = set()
    for obs in _observations(dataset, env_cfg, 50):
        b = D.batch_from_obs(obs)
        out = pol.schedule(b, greedy=True)
        ss, exec_scores = _scores(pol, b)
        sched = torch.nonzero(b.stage_mask).squeeze(1)
        si = int(torch.argmax(ss[sched]))
        assert int(out["stage_idx"][0]) == si
        dag = int(b.node_dag[sched[si]])
        assert int(out["job_idx"][0]) == dag
        es, valid = exec_scores(dag)
        ei = int(torch.argmax(torch.where(valid, es, torch.full_like(es, -torch.inf))))
        assert int(out["exec_idx"][0]) == ei and int(out["num_exec"][0]) == ei + 1
        picked_exec.add(ei)
        want = torch.log_softmax(ss[sched], 0)[si] + torch.log_softmax(es[valid], 0)[ei]
        assert abs(float(out["lgprob"][0]) - float(want)) <= 1e-5
        assert set(pol.schedule(b, generator=torch.Generator().manual_seed(1))) == set(out)
        action, info = pol.schedule_obs(obs, greedy=True)
        assert action == {"stage_idx": si, "num_exec": ei} and info["job_idx"] == dag
    assert len(picked_exec) > 1  # (the exec arg-max is not always k = 0 with this policy)


def test_schedule_greedy_ties_take_index_zero(dataset, env_cfg):
    """All-equal scores (the score MLPs' last weights zeroed): stage_idx 0 and exec_idx 0, for one env and for a batch."""
    pol = _policy(env_cfg["num_executors"])
    with torch.no_grad():
        pol.stage_policy_network.mlp_score[-1].weight.zero_()
        pol.exec_policy_network.mlp_score[-1].weight.zero_()
    for obs in _observations(dataset, env_cfg, 12)[3:]:
        b = D.batch_from_obs(obs)
        out = pol.schedule(b, greedy=True)
        assert (int(out["stage_idx"][0]), int(out["exec_idx"][0]), int(out["num_exec"][0])) == (0, 0, 1)
        nsch = int(b.stage_mask.sum())
        cap = int(b.exec_cap[int(out["job_idx"][0])])
        assert abs(float(out["lgprob"][0]) + np.log(nsch) + np.log(cap)) <= 1e-5
    b3 = D.cat_batches([D.batch_from_obs(o) for o in _observations(dataset, env_cfg, 8)[5:]])
    out = pol.schedule(b3, greedy=True)
    assert out["stage_idx"].tolist() == [0, 0, 0] and out["exec_idx"].tolist() == [0, 0, 0]


def test_argmax_pick_first_maximum_and_empty_segments():
    s = torch.tensor([1.0, 3.0, 3.0, 2.0, 5.0, 5.0, 7.0])
    mask = torch.tensor([True, True, True, True, True, True, False])
    seg = torch.tensor([0, 0, 0, 0, 2, 2, 3])
    assert D.argmax_pick(s, mask, seg, 4).tolist() == [1, -1, 4, -1]


# ------------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip(tmp_path):
    """save / load: bit-equal parameters and packed_params, num_executors kept, and the file is a plain dict that loads
    with weights_only=True."""
    pol = _policy(50)
    path = tmp_path / "decima.pt"
    pol.save(path)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"format_version", "num_executors", "arch", "state_dict"}
    assert ck["format_version"] == D.CHECKPOINT_VERSION and ck["num_executors"] == 50
    back = DecimaScheduler.load(path)
    assert back.num_executors == 50
    a, b = pol.state_dict(), back.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert torch.equal(pol.packed_params("cpu"), back.packed_params("cpu"))
    assert back.packed_params("cpu").numel() == D.DECIMA_PARAMS
    assert DecimaScheduler.load(str(path), device="cpu").device.type == "cpu"


def test_checkpoint_refuses_other_versions_and_architectures(tmp_path):
    pol = _policy(10)
    path = tmp_path / "decima.pt"
    pol.save(path)
    ck = torch.load(path, weights_only=True)
    torch.save(dict(ck, format_version=D.CHECKPOINT_VERSION + 1), tmp_path / "v2.pt")
    with pytest.raises(ValueError, match="format version"):
        DecimaScheduler.load(tmp_path / "v2.pt")
    torch.save({"state_dict": ck["state_dict"]}, tmp_path / "bare.pt")
    with pytest.raises(ValueError, match="format_version"):
        DecimaScheduler.load(tmp_path / "bare.pt")
    wide = DecimaScheduler(10, embed_dim=8)  # another architecture than the fused kernels'
    wide.save(tmp_path / "wide.pt")
    with pytest.raises(ValueError, match=f"{D.DECIMA_PARAMS}"):
        DecimaScheduler.load(tmp_path / "wide.pt")


# ------------------------------------------------------------------------------------------ examples --sched decima
def test_examples_decima_needs_a_model(capsys):
    from spark_sched_sim import examples

    with pytest.raises(SystemExit) as ex:
        examples.main(["--sched", "decima"])
    assert ex.value.code == 2
    assert "--sched decima needs --model" in capsys.readouterr().err


def test_examples_decima_episode_on_the_host_build(tmp_path, dataset, env_cfg):
    """`examples --sched decima`'s scheduler on the facade (host build): a loaded checkpoint drives one short episode
    to termination through DecimaEnvWrapper, greedy and sampled."""
    from hostsim.driver import HostEngine
    from spark_sched_sim.examples import DecimaHostScheduler, run_episode

    cfg = dict(env_cfg, job_arrival_cap=6)
    _policy(cfg["num_executors"]).save(tmp_path / "m.pt")
    model = DecimaScheduler.load(tmp_path / "m.pt")
    got = [run_episode(cfg, DecimaHostScheduler(model, sample=sample), seed=77, dataset=dataset,
                       _engine_factory=lambda c, ds: HostEngine(c, 1, ds)) for sample in (False, False, True)]
    assert all(np.isfinite(g) and g > 0 for g in got) and got[0] == got[1]
