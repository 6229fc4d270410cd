"""TEST INFRASTRUCTURE ONLY — the host build's ssim_episode_stats: hostsim/episode_stats.cpp (a serial loop over the
host engine's state arena) built into its own library, and `StatsHostEngine`, the host engine (hostsim.driver
HostEngine) with DeviceEngine's `episode_stats()`."""

from __future__ import annotations

import ctypes as ct
import os
import subprocess

import numpy as np

from hostsim import driver
from hostsim.driver import HostEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hostsim", "episode_stats.cpp")
SO_PATH = os.path.join(HERE, "hostsim", "_hostsim_stats.so")

_lib = None


def build(force: bool = False) -> str:
    """Builds _hostsim_stats.so if stale, as hostsim.driver.build does (one builder at a time under an flock, each
    writing its own temporary before the atomic rename)."""
    import fcntl

    deps = [SOURCE] + driver.SOURCES[1:]

    def stale():
        return not os.path.exists(SO_PATH) or os.path.getmtime(SO_PATH) < max(os.path.getmtime(p) for p in deps)

    if not force and not stale():
        return SO_PATH
    with open(SO_PATH + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if force or stale():
            tmp = f"{SO_PATH}.{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall",
                            "-Wno-unused-function", f"-I{os.path.join(driver.REPO, 'include')}",
                            f"-I{os.path.join(driver.REPO, 'gym-sparksched_amd', 'csrc')}", SOURCE, "-o", tmp],
                           check=True)
            os.replace(tmp, SO_PATH)
    return SO_PATH


def lib():
    global _lib
    if _lib is None:
        L = ct.CDLL(build())
        L.hs_episode_stats.argtypes = [ct.c_void_p, ct.c_void_p]
        L.hs_episode_stats.restype = None
        _lib = L
    return _lib


class StatsHostEngine(HostEngine):
    def episode_stats(self) -> np.ndarray:
        """float64 [B][4] as DeviceEngine.episode_stats (ssim_episode_stats)."""
        out = np.zeros((self.num_envs, 4))
        lib().hs_episode_stats(self.state.ctypes.data, out.ctypes.data)
        return out
