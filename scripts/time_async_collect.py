#!/usr/bin/env python
"""Times one fixed-duration collect() of the decima_tpch.yaml env with both collectors in one process: the lockstep
AsyncRolloutCollector (per decision: features, fused policy and step launches, two host syncs) and
DeviceAsyncRolloutCollector (persistent launches, csrc/decima_rollout.h timed mode). Both draw the same actions, so
they collect the same decisions. The first call of each (kernel code loads, the first resets) is discarded; the
median of the rest is printed, with the decisions and launches per call.

  python scripts/time_async_collect.py [--rows 16] [--duration 1e6] [--mean-time-limit 2e7] [--calls 6]
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gym-sparksched_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--duration", type=float, default=1e6, help="rollout_duration, ms of simulated time per call")
    ap.add_argument("--mean-time-limit", type=float, default=2e7)
    ap.add_argument("--calls", type=int, default=6, help="collect() calls per collector, the first discarded")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()

    import torch

    from spark_sched_sim.engine import DeviceEngine
    from spark_sched_sim.env import resolve_dataset
    from spark_sched_sim.schedulers.decima import DecimaScheduler
    from spark_sched_sim.trainers import DECIMA_TPCH, AsyncRolloutCollector, DeviceAsyncRolloutCollector

    env = {k: v for k, v in DECIMA_TPCH["env"].items() if k not in ("mean_time_limit", "dataset")}
    dataset = resolve_dataset(DECIMA_TPCH["env"])
    torch.manual_seed(3)
    pol = DecimaScheduler(env["num_executors"]).to(a.device)
    base = [1 + r // 4 for r in range(a.rows)]  # four rows per job sequence, as decima_tpch.yaml's num_rollouts
    out = {"rows": a.rows, "duration_ms": a.duration, "mean_time_limit": a.mean_time_limit}
    for name, cls in (("lockstep", AsyncRolloutCollector), ("device", DeviceAsyncRolloutCollector)):
        eng = DeviceEngine(env, a.rows, dataset, device=a.device)
        col = cls(eng, pol, a.duration, base, a.rows // 4 or 1, mean_time_limit=a.mean_time_limit, seed=77)
        secs, decisions, launches = [], [], []
        for _ in range(a.calls):
            before = getattr(col, "launches", 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            buf = col.collect()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            decisions.append(len(buf))
            launches.append(getattr(col, "launches", 0) - before)
        out[name] = {"median_s": statistics.median(secs[1:]), "calls_s": [round(s, 4) for s in secs],
                     "decisions": decisions, "resets": int(col.reset_count.sum()) - a.rows}
        if name == "device":
            out[name]["launches"] = launches
        eng.close()
    out["same_decisions"] = out["lockstep"]["decisions"] == out["device"]["decisions"]
    out["speedup"] = out["lockstep"]["median_s"] / out["device"]["median_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
