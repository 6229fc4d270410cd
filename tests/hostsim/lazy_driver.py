"""Python driver for the TEST-ONLY host build of the fused rollouts' decision loop on the lazy engine
(hostsim_lazy.cpp): a HostEngine whose rollouts run rollout.h rollout_loop with deferred arena rows, as the device's
k_rollout / k_rollout_prio do. Everything else (reset, step, the arenas) is HostEngine's."""

from __future__ import annotations

import ctypes as ct
import os
import subprocess

import numpy as np

from . import driver
from .driver import HERE, REPO, HostEngine

SO_PATH = os.path.join(HERE, "_hostsim_lazy.so")
SOURCES = [os.path.join(HERE, "hostsim_lazy.cpp")] + driver.SOURCES

_lib = None


def build() -> str:
    """Builds _hostsim_lazy.so if stale (one builder at a time, atomic rename: driver.build's scheme)."""
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
        vp = ct.c_void_p
        L.hs_rollout_lazy.argtypes = [vp, ct.c_int, ct.c_uint64, vp, ct.c_int, ct.c_int, vp, vp]
        _lib = L
    return _lib


class LazyHostEngine(HostEngine):
    """HostEngine with the rollouts of the lazy engine. The handle is plain host memory both shared objects lay out
    alike (hostsim_lazy.cpp includes hostsim.cpp)."""

    def rollout(self, kind, seed, num_steps, action_log=None, flags=0, time_limits=None):
        self._lazy(kind, seed, None, num_steps, action_log, flags, time_limits)

    def rollout_steps(self, kind, seed, env_steps, max_steps, action_log=None, flags=0, time_limits=None):
        st = np.ascontiguousarray(np.asarray(env_steps, dtype=np.int32).reshape(self.num_envs))
        self._lazy(kind, seed, st, max_steps, action_log, flags, time_limits)

    def _lazy(self, kind, seed, st, num_steps, action_log, flags, time_limits):
        ptr = action_log.ctypes.data if action_log is not None else None
        tl = None if time_limits is None else np.ascontiguousarray(np.asarray(time_limits, dtype=np.float64))
        rc = lib().hs_rollout_lazy(self.handle, kind, seed, None if st is None else st.ctypes.data, num_steps, flags,
                                   None if tl is None else tl.ctypes.data, ptr)
        assert rc == 0, f"hostsim lazy rollout rc={rc}"


__all__ = ["LazyHostEngine", "build", "lib"]
