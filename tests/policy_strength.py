"""TEST INFRASTRUCTURE ONLY — how strong a comparison with the Decima oracle is at a given parameter set, measured
from the reference alone (oracle/decima_gnn.py; no kernel, no GPU).

A test that compares a policy kernel's stage scores, exec scores and log-probability with the oracle can only see a
defect that moves one of those by more than its bar. At nearly flat parameters (PyTorch's init plus a little noise) a
whole layer can be 1% wrong below the bars. This module measures, for a state dict and a list of samples
(observation, stage_idx, exec_idx):

  measure        per sample, the three compared quantities from the fp64 oracle, the fp32 oracle and the fp32 oracle
                 with the score MLPs' Tanh restated as csrc/decima_policy.h dp_tanh (G.dp_tanh_f32); the mean
                 within-observation stage-score spread and the share of Tanh hidden units with |output| > 0.99
  derived_lgprob_bar   the rollout cases' lgprob bar: 16 x the larger of max |lgprob fp32 - fp64| and max |lgprob
                 restated dp_tanh - fp64|, floored at 2e-6 (a few f32 ulps of an lgprob of order 1), never above the
                 standing 1e-4 + 1e-4 |want| (applied per sample: decima_audit.lgprob_bar_of). The 16 allows for the
                 kernel's other summation order over at most a few hundred terms and for one-ulp hardware exp2 / rcp /
                 expf / logf; it is a margin over the reference's number, not a measurement of a kernel.
  ratios         the largest movement of each quantity relative to its bar between two evaluations
  layer_sweep    per nn.Linear weight, `ratios` when that weight alone is multiplied by 1.01 (fp64 against fp64)
  accept         the acceptance rule (a)-(e) of a "spread" parameter set

The score bar is the fused kernel's 1e-5 + 1e-4 |score| per score (decima_audit.SCORE_ATOL / SCORE_RTOL).
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import decima_audit as A
from oracle import decima_gnn as G

BAR_FACTOR, BAR_FLOOR = 16.0, 2e-6
MIN_LAYER_RATIO, MAX_FP32_SHARE, MAX_ACT_SHARE, MAX_SATURATED, MIN_SPREAD = 4.0, 0.25, 0.5, 0.2, 0.2
LAYER_SCALE = 1.01


def linear_weights(sd: dict) -> list[str]:
    return [k for k in sd if k.endswith(".weight")]


def evaluate(sd: dict, sample, num_executors: int, dtype=torch.float32, pol_act=None):
    """(stage scores, exec scores of the chosen stage's job, lgprob of the action) of one sample, as float64 numpy."""
    dobs, si, ei = sample
    enc = G.encode(sd, dobs, dtype=dtype)
    ss = G.stage_scores(sd, dobs, enc, dtype=dtype, pol_act=pol_act)
    es = G.exec_scores(sd, dobs, enc, G.job_of_stage(dobs, si), num_executors, dtype=dtype, pol_act=pol_act)
    lg = float(torch.log_softmax(ss, 0)[si] + torch.log_softmax(es, 0)[ei])
    return ss.double().numpy(), es.double().numpy(), lg


def evaluate_all(sd: dict, samples, num_executors: int, dtype=torch.float32, pol_act=None) -> list:
    with torch.no_grad():
        return [evaluate(sd, s, num_executors, dtype, pol_act) for s in samples]


def argmax_samples(sd: dict, observations, num_executors: int) -> list:
    """(observation, stage_idx, exec_idx) with the fp64 oracle's arg-max action, for observations without one."""
    out = []
    for dobs in observations:
        p = A.policy(sd, dobs, num_executors, dtype=torch.float64)
        out.append((dobs, p.s_win, p.e_win))
    return out


def ratios(got: list, ref: list, lgprob_bar=None) -> dict:
    """The largest |got - ref| relative to the bar, over the samples: per stage score and per exec score (1e-5 + 1e-4
    |ref score|), and for the lgprob (decima_audit.lgprob_bar_of). lg_abs: the largest |lgprob difference| itself."""
    r = dict(stage=0.0, exec=0.0, lgprob=0.0, lg_abs=0.0)
    for (gs, ge, gl), (rs, re_, rl) in zip(got, ref):
        r["stage"] = max(r["stage"], float((np.abs(gs - rs) / (A.SCORE_ATOL + A.SCORE_RTOL * np.abs(rs))).max()))
        if re_.size:
            r["exec"] = max(r["exec"], float((np.abs(ge - re_) / (A.SCORE_ATOL + A.SCORE_RTOL * np.abs(re_))).max()))
        r["lgprob"] = max(r["lgprob"], abs(gl - rl) / A.lgprob_bar_of(rl, lgprob_bar))
        r["lg_abs"] = max(r["lg_abs"], abs(gl - rl))
    return r


def measure(sd: dict, samples, num_executors: int) -> SimpleNamespace:
    """The fp64, fp32 and restated-dp_tanh evaluations of every sample, the mean stage-score spread (max - min within
    an observation, fp64) and the share of the score MLPs' Tanh outputs with |output| > 0.99 (fp64)."""
    hidden = []

    def tanh_seen(x):
        y = torch.tanh(x)
        hidden.append(y.abs().reshape(-1))
        return y

    ref = evaluate_all(sd, samples, num_executors, torch.float64, tanh_seen)
    h = torch.cat(hidden)
    return SimpleNamespace(
        ref=ref, fp32=evaluate_all(sd, samples, num_executors),
        act=evaluate_all(sd, samples, num_executors, pol_act=G.dp_tanh_f32),
        spread=float(np.mean([s.max() - s.min() for s, _, _ in ref])),
        saturated=float((h > 0.99).double().mean()))


def derived_lgprob_bar(m: SimpleNamespace) -> tuple[float, float, float]:
    """(bar, max |lgprob fp32 - fp64|, max |lgprob restated dp_tanh - fp64|) over the measured samples."""
    e32, eact = ratios(m.fp32, m.ref)["lg_abs"], ratios(m.act, m.ref)["lg_abs"]
    return max(BAR_FACTOR * max(e32, eact), BAR_FLOOR), e32, eact


def layer_sweep(sd: dict, samples, num_executors: int, ref: list, lgprob_bar=None) -> dict:
    """Per nn.Linear weight of `sd`: `ratios` of the fp64 oracle with that weight alone times 1.01 against `ref` (the
    fp64 oracle at `sd` on the same samples)."""
    out = {}
    for name in linear_weights(sd):
        bad = dict(sd)
        bad[name] = sd[name].double() * LAYER_SCALE
        out[name] = ratios(evaluate_all(bad, samples, num_executors, torch.float64), ref, lgprob_bar)
    return out


def strength(sd: dict, samples, num_executors: int, quantities=("stage", "exec", "lgprob"), derive_bar=False,
             sweep_stride: int = 1, m=None) -> SimpleNamespace:
    """Everything the acceptance rule needs. `quantities`: what the case compares (a rollout audit sees only the
    lgprob). derive_bar: take the lgprob bar from the reference (derived_lgprob_bar) instead of the standing one.
    sweep_stride: the layer sweep runs on every sweep_stride-th sample (a subset can only understate a layer's
    movement); the reference's own errors are always taken over all samples."""
    m = m or measure(sd, samples, num_executors)  # (m: this very call's result, when the caller holds it)
    bar, e32, eact = derived_lgprob_bar(m) if derive_bar else (None, *derived_lgprob_bar(m)[1:])
    sub = slice(None, None, sweep_stride)
    sweep = layer_sweep(sd, samples[sub], num_executors, m.ref[sub], bar)
    pick = lambda r: max(r[q] for q in quantities)  # noqa: E731
    return SimpleNamespace(
        lgprob_bar=bar, lg_err_fp32=e32, lg_err_act=eact, spread=m.spread, saturated=m.saturated,
        fp32_share=pick(ratios(m.fp32, m.ref, bar)), act_share=pick(ratios(m.act, m.ref, bar)),
        layers={k: pick(r) for k, r in sweep.items()}, sweep=sweep)


def describe(name: str, s: SimpleNamespace) -> str:
    weakest = min(s.layers, key=s.layers.get)
    bar = "standing" if s.lgprob_bar is None else f"{s.lgprob_bar:.2e}"
    return (f"{name}: lgprob bar {bar} (|fp32 - fp64| {s.lg_err_fp32:.2e}, |dp_tanh - fp64| {s.lg_err_act:.2e}); "
            f"(a) weakest layer {weakest} {s.layers[weakest]:.1f}x, layers under the bar "
            f"{sum(v < 1 for v in s.layers.values())}, under 4x {sum(v < 4 for v in s.layers.values())}; "
            f"(b) fp32 {s.fp32_share:.3f}; (c) dp_tanh {s.act_share:.3f}; (d) saturated {s.saturated:.1%}; "
            f"(e) spread {s.spread:.3f}")


def accept(name: str, s: SimpleNamespace) -> None:
    """The acceptance rule of a spread parameter set on the samples a case audits: (a) every layer's 1% error moves a
    compared quantity by at least 4 x its bar, (b) the fp32 oracle within 1/4 and (c) the restated-dp_tanh oracle
    within 1/2 of the bar of the fp64 oracle, (d) fewer than 20% of Tanh units beyond 0.99, (e) mean spread >= 0.2."""
    assert len(s.layers) == 21, len(s.layers)
    weak = {k: round(v, 2) for k, v in s.layers.items() if v < MIN_LAYER_RATIO}
    assert not weak, f"{name} (a): a 1% error of these layers moves nothing by {MIN_LAYER_RATIO} x its bar: {weak}"
    assert s.fp32_share <= MAX_FP32_SHARE, f"{name} (b): fp32 oracle at {s.fp32_share:.3f} of the bar"
    assert s.act_share <= MAX_ACT_SHARE, f"{name} (c): restated dp_tanh at {s.act_share:.3f} of the bar"
    assert s.saturated < MAX_SATURATED, f"{name} (d): {s.saturated:.1%} of Tanh units saturated"
    assert s.spread >= MIN_SPREAD, f"{name} (e): mean stage-score spread {s.spread:.3f}"
