"""Loader for the in-tree gfx950 library (libsparksched.so). Fails loudly: there is no CPU fallback."""

from __future__ import annotations

import ctypes as ct
import os

from ._abi import SsimConfig, SsimDataset, SsimLayout

_HERE = os.path.dirname(os.path.abspath(__file__))
# SSIM_LIB overrides the path (development A/B runs of alternative builds of the same sources)
LIB_PATH = os.environ.get("SSIM_LIB") or os.path.join(os.path.dirname(_HERE), "build", "libsparksched.so")

_lib = None


class NativeError(RuntimeError):
    pass


_vp, _i32, _i64, _u64, _f32 = ct.c_void_p, ct.c_int32, ct.c_int64, ct.c_uint64, ct.c_float
_DECIMA_ROLLOUT = [_vp, _vp, _i32, _f32, _f32, _u64, _u64, _i32, _i64, _i32, _vp, _vp, _i64, _vp]
# The C ABI (include/sparksched.h): (symbol, restype, argtypes). lib() sets every prototype from this one table.
_PROTOTYPES = [
    ("ssim_layout_for", ct.c_int, [ct.POINTER(SsimConfig), ct.POINTER(SsimLayout)]),
    ("ssim_create", ct.c_int, [ct.POINTER(SsimConfig), ct.POINTER(SsimDataset), _vp, _vp, _vp, ct.POINTER(_vp)]),
    ("ssim_destroy", ct.c_int, [_vp]),
    ("ssim_reset", ct.c_int, [_vp, _vp]),
    ("ssim_step", ct.c_int, [_vp, _vp, _vp, _vp]),
    ("ssim_policy", ct.c_int, [_vp, _i32, _u64, _u64, _vp, _vp, _vp]),
    ("ssim_rollout", ct.c_int, [_vp, _i32, _u64, _i32, _vp, _vp]),
    ("ssim_rollout_ex", ct.c_int, [_vp, _i32, _u64, _i32, _i32, _vp, _vp, _vp]),
    ("ssim_rollout_budget", ct.c_int, [_vp, _i32, _u64, _i32, _i64, _i32, _vp, _vp, _vp]),
    ("ssim_rollout_steps", ct.c_int, [_vp, _i32, _u64, _vp, _i32, _i32, _vp, _vp, _vp]),
    ("ssim_reset_sampled", ct.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("ssim_job_times", ct.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("ssim_episode_stats", ct.c_int, [_vp, _vp, _vp]),
    ("ssim_decima_features", ct.c_int, [_vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp]),
    ("ssim_decima_policy", ct.c_int, [_vp] * 6 + [_i32, _i32, _u64, _u64] + [_vp] * 10),
    ("ssim_decima_workspace_bytes", _i64, [_vp]),
    ("ssim_decima_rollout", ct.c_int, _DECIMA_ROLLOUT + [_vp, _vp]),
    ("ssim_decima_rollout_timed", ct.c_int, _DECIMA_ROLLOUT + [_vp, _vp, _vp]),
    ("ssim_decima_rollout_lds_bytes", _i64, [_vp]),
    ("ssim_debug_decima_plan", ct.c_int, [_vp, ct.POINTER(_i32), ct.POINTER(_i32)]),
    ("ssim_teacher_rollout", ct.c_int, [_vp, _i32, _u64, _f32, _f32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    ("ssim_debug_teacher_plan", ct.c_int, [_vp, ct.POINTER(_i32), ct.POINTER(_i32)]),
    ("ssim_last_error", ct.c_char_p, []),
    ("ssim_build_id", ct.c_char_p, []),
    ("ssim_debug_set_trace", ct.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    ("ssim_debug_set_trace_ex", ct.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    ("ssim_debug_kernel_name", ct.c_char_p, [_vp, _i32]),
    ("ssim_debug_wfair", ct.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    ("ssim_linear_fwd", ct.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    ("ssim_linear_wgrad_parts", _i32, [_i64]),
    ("ssim_linear_wgrad", ct.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp]),
    ("ssim_mlp3_supported", _i32, [_i32] * 5),
    ("ssim_mlp3_fwd", ct.c_int, [_vp, _vp, _i32] + [_vp] * 9 + [_i64] + [_i32] * 5 + [_f32, _vp]),
    ("ssim_mlp3_parts", _i32, [_i64]),
    ("ssim_mlp3_partial_floats", _i64, [_i64, _i32, _i32, _i32, _i32]),
    ("ssim_mlp3_bwd", ct.c_int, [_vp, _vp, _vp, _i32] + [_vp] * 14 + [_i64] + [_i32] * 5 + [_f32, _vp, _i32, _vp]),
    ("ssim_discounted_returns", ct.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _vp]),
]
EXPORTED_SYMBOLS = [name for name, _, _ in _PROTOTYPES]


def lib() -> ct.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its HIP runtime must be the process's (the library's libamdhip64 dependency then resolves to the copy
    # torch loaded). Loaded the other way round, torch's device init later fails ("no ROCm-capable device").
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"libsparksched.so not found at {LIB_PATH}; build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). The simulator has no CPU fallback.")
    L = ct.CDLL(LIB_PATH)
    for name, restype, argtypes in _PROTOTYPES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise NativeError(f"{what} failed ({rc}): {lib().ssim_last_error().decode(errors='replace')}")


def build_id() -> str:
    """The loaded library's build identity (source + definition hash, __graft_entry__.source_hash)."""
    return lib().ssim_build_id().decode()
