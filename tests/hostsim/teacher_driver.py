"""Python driver for the TEST-ONLY host build of the teacher rollout (teacher.cpp): a HostEngine with a
`teacher_rollout` that runs csrc/teacher_rollout.h TeacherPolicy under rollout.h rollout_loop on the one-lane wave, into
a CPU DecimaSampleArena (torch tensors on the host). Everything else (reset, step, the arenas) is HostEngine's."""

from __future__ import annotations

import ctypes as ct
import os
import subprocess

import numpy as np

from . import driver
from .driver import HERE, REPO, HostEngine

SO_PATH = os.path.join(HERE, "_hostsim_teacher.so")
SOURCES = [os.path.join(HERE, "teacher.cpp"),
           os.path.join(REPO, "gym-sparksched_amd", "csrc", "teacher_rollout.h"),
           os.path.join(REPO, "gym-sparksched_amd", "csrc", "sample_arena.h")] + driver.SOURCES

_lib = None


def build() -> str:
    """Builds _hostsim_teacher.so if stale (one builder at a time, atomic rename: driver.build's scheme)."""
    import fcntl

    def stale():
        newest = max(os.path.getmtime(p) for p in SOURCES)
        return not os.path.exists(SO_PATH) or os.path.getmtime(SO_PATH) < newest

    if not stale():
        return SO_PATH
    with open(SO_PATH + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if stale():
            tmp = f"{SO_PATH}.{os.getpid()}.tmp"
            cmd = ["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall",
                   "-Wno-unused-function", f"-I{os.path.join(REPO, 'include')}",
                   f"-I{os.path.join(REPO, 'gym-sparksched_amd', 'csrc')}", SOURCES[0], "-o", tmp, *driver.ENV_FLAGS]
            subprocess.run(cmd, check=True)
            os.replace(tmp, SO_PATH)
    return SO_PATH


def lib():
    global _lib
    if _lib is None:
        L = ct.CDLL(build())
        vp, i64 = ct.c_void_p, ct.c_int64
        L.hs_teacher_rollout.argtypes = [vp, ct.c_int, ct.c_uint64, ct.c_float, ct.c_float, ct.c_int, vp, i64, i64,
                                         i64, i64, i64, ct.c_int, ct.c_int, vp, vp]
        L.hs_arena_op.argtypes = [ct.c_int, vp, ct.c_int, vp, vp, vp, vp, vp, vp, vp, vp, ct.c_float, ct.c_double]
        _lib = L
    return _lib


class TeacherHostEngine(HostEngine):
    """HostEngine with DeviceEngine.teacher_rollout. `plan_cap` / `plan_dags`: the node and DAG counts up to which a
    decision keeps the features' scratch in the emulated LDS (the device takes its own from the layout; the recorded arena does not
    depend on it). The handle is plain host memory both shared objects lay out alike (teacher.cpp includes
    hostsim.cpp)."""

    def __init__(self, *args, plan_cap: int = 32, plan_dags: int = 16, **kw):
        super().__init__(*args, **kw)
        self.plan_cap, self.plan_dags = int(plan_cap), int(plan_dags)
        self.device = "cpu"
        L = self.layout
        a16 = lambda x: (x + 15) & ~15  # noqa: E731
        self._stride = (a16(10 * L.stage_cap) + 255) & ~255
        o = self._stride * L.num_envs
        self._feats = o
        o = a16(o + L.num_envs * L.stage_cap * 5 * 4)
        self._ccap = o
        o = a16(o + L.num_envs * L.job_cap * 4)
        self._emask = o
        o = a16(o + L.num_envs * L.edge_cap * 4)
        self._depth = o
        self._work = np.zeros(a16(o + L.num_envs * 4), dtype=np.uint8)

    def teacher_rollout(self, kind, seed, steps, samples, num_tasks_scale=200.0, work_scale=1e5, action_log=None):
        st = samples.struct()
        ptr = action_log.ctypes.data if action_log is not None else None
        rc = lib().hs_teacher_rollout(self.handle, int(kind), int(seed) & (2**64 - 1), float(num_tasks_scale),
                                      float(work_scale), int(steps), self._work.ctypes.data, self._stride, self._feats,
                                      self._ccap, self._emask, self._depth, self.plan_cap, self.plan_dags, ct.byref(st), ptr)
        assert rc == 0, f"hostsim teacher rollout rc={rc}"


__all__ = ["TeacherHostEngine", "build", "lib"]
