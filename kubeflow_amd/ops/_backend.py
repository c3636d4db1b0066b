"""ctypes loader for the in-tree CDNA4 kernel library.

Policy (per the project's "no silent eager fallback" rule):
  * On a machine WITH a GPU, the HIP library is required — a missing or
    unloadable libkfops.so raises at first use, unless the user explicitly
    sets KF_NATIVE_KERNELS=0 (bisection escape hatch).
  * On CPU-only machines (CI container), ops fall back to the pure-torch
    reference implementations so unit tests run without a GPU.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

_LIB_PATH = Path(__file__).resolve().parent / "libkfops.so"
_lib = None
_load_error: str | None = None


def native_enabled() -> bool:
    return os.environ.get("KF_NATIVE_KERNELS", "1") != "0"


def try_load():
    """Load libkfops.so if present; returns the CDLL or None."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if not native_enabled():
        _load_error = "disabled via KF_NATIVE_KERNELS=0"
        return None
    from . import build_ext
    if build_ext.needs_build():
        # stale or missing .so — rebuild (sources are authoritative; a stale
        # library with a changed C ABI segfaults at call time)
        try:
            build_ext.build(verbose=True)
        except Exception as e:
            _load_error = f"build failed: {e}"
            return None
    try:
        _lib = ctypes.CDLL(str(_LIB_PATH))
    except OSError as e:  # pragma: no cover
        _load_error = str(e)
        return None
    _configure(_lib)
    return _lib


def require():
    """Return the library, raising loudly if it should be there but is not."""
    lib = try_load()
    if lib is None:
        raise RuntimeError(
            "kubeflow_amd native kernels unavailable on a GPU machine: "
            f"{_load_error}. Build with `python -m kubeflow_amd.ops.build_ext` "
            "or set KF_NATIVE_KERNELS=0 to explicitly allow the (slow) "
            "reference path.")
    return lib


def _configure(lib: ctypes.CDLL) -> None:
    c = ctypes
    P, F, I64, I32, FP = c.c_void_p, c.c_float, c.c_int64, c.c_int, c.POINTER(c.c_float)
    PI64 = c.POINTER(c.c_int64)
    PI32 = c.POINTER(c.c_int32)
    lib.kf_rmsnorm_fwd.restype = I32
    lib.kf_rmsnorm_fwd.argtypes = [P, FP, P, P, I64, I64, F, P]
    lib.kf_rmsnorm_bwd.restype = I32
    lib.kf_rmsnorm_bwd.argtypes = [P, P, FP, P, P, P, FP, I64, I64, P]
    lib.kf_rmsnorm_bwd_nparts.restype = I64
    lib.kf_rmsnorm_bwd_nparts.argtypes = [I64]
    lib.kf_rope.restype = I32
    lib.kf_rope.argtypes = [P, P, FP, FP, PI64, I64, I64, I64, I64, I64, I64, I64, I64, I32, P]
    lib.kf_adamw.restype = I32
    lib.kf_adamw.argtypes = [P, FP, P, FP, FP, FP, I64, F, F, F, F, F, I64, P]
    lib.kf_ce_fwd.restype = I32
    lib.kf_ce_fwd.argtypes = [FP, FP, P, PI64, I64, I64, I64, P]
    lib.kf_ce_bwd.restype = I32
    lib.kf_ce_bwd.argtypes = [P, P, FP, PI64, FP, I64, I64, I64, P]
    lib.kf_attn_fwd.restype = I32
    lib.kf_attn_fwd.argtypes = [P, FP, P, P, P, I64, I64, I64, I64, I64, I64, I64, F, I32, P]
    if hasattr(lib, "kf_skinny_gemm"):
        lib.kf_skinny_gemm.restype = I32
        lib.kf_skinny_gemm.argtypes = [P, P, P, P, FP, F, I64, I64, I64,
                                       I64, I64, I64, I64, P]
    if hasattr(lib, "kf_skinny_gemm_q8"):
        lib.kf_skinny_gemm_q8.restype = I32
        lib.kf_skinny_gemm_q8.argtypes = [P, P, P, FP, P, FP, F, I64,
                                          I64, I64, I64, I64, I64, I64,
                                          P]
    if hasattr(lib, "kf_kv_store"):
        lib.kf_kv_store.restype = I32
        lib.kf_kv_store.argtypes = [P, P, P, P, P, P, I64, I64, I64, P]
    if hasattr(lib, "kf_attn_fwd4_rect"):
        lib.kf_attn_fwd4_rect.restype = I32
        lib.kf_attn_fwd4_rect.argtypes = [P, FP, P, P, P, I64, I64, I64,
                                          I64, I64, I64, I64, I64, F, I64, P]
    if hasattr(lib, "kf_attn_bwd"):
        lib.kf_attn_bwd.restype = I32
        lib.kf_attn_bwd.argtypes = [P, P, P, P, P, P, P, P, FP, FP, I64, I64,
                                    I64, I64, I64, I64, I64, I64, I64, F, I32,
                                    P]
    if hasattr(lib, "kf_attn_bwd_rope"):
        # kf_attn_bwd's arguments + cos, sin, pos_offset before the stream
        lib.kf_attn_bwd_rope.restype = I32
        lib.kf_attn_bwd_rope.argtypes = [P, P, P, P, P, P, P, P, FP, FP, I64,
                                         I64, I64, I64, I64, I64, I64, I64,
                                         I64, F, I32, FP, FP, I64, P]
    # per-pass entry points of the 8-wave backward (tests / bisection);
    # the *_rope forms add cos, sin, pos_offset before the stream
    dq8 = [P, P, P, P, P, FP, FP, I64, I64, I64, I64, I64, I64, I64, F, I32]
    dkv8 = [P] + dq8
    for name, args in (("kf_attn_bwd8_dq", dq8), ("kf_attn_bwd8_dkv", dkv8),
                       ("kf_attn_bwd8_dkv_fused", dkv8)):
        if hasattr(lib, name):
            getattr(lib, name).restype = I32
            getattr(lib, name).argtypes = args + [P]
        if hasattr(lib, name + "_rope"):
            getattr(lib, name + "_rope").restype = I32
            getattr(lib, name + "_rope").argtypes = args + [FP, FP, I64, P]
    # head-dim-64 family (attention_d64.hip): ..., qts, kts, scale, causal,
    # kv_len, stream
    if hasattr(lib, "kf_attn64_fwd"):
        lib.kf_attn64_fwd.restype = I32
        lib.kf_attn64_fwd.argtypes = [P, FP, P, P, P, I64, I64, I64, I64,
                                      I64, I64, F, I32, I64, P]
    if hasattr(lib, "kf_attn64_bwd"):
        lib.kf_attn64_bwd.restype = I32
        lib.kf_attn64_bwd.argtypes = [P, P, P, P, P, P, P, P, FP, FP, I64,
                                      I64, I64, I64, I64, I64, F, I32, I64, P]
    lib.kf_layernorm_fwd.restype = I32
    lib.kf_layernorm_fwd.argtypes = [P, FP, FP, P, P, P, I64, I64, F, P]
    lib.kf_layernorm_bwd.restype = I32
    lib.kf_layernorm_bwd.argtypes = [P, P, P, FP, P, P, P, FP, FP, I64, I64, P]
    lib.kf_layernorm_bwd_nparts.restype = I64
    lib.kf_layernorm_bwd_nparts.argtypes = [I64]
    lib.kf_swiglu_fwd.restype = I32
    lib.kf_swiglu_fwd.argtypes = [P, P, I64, I64, P]
    lib.kf_swiglu_bwd.restype = I32
    lib.kf_swiglu_bwd.argtypes = [P, P, P, I64, I64, P]
    lib.kf_attn_decode.restype = I32
    lib.kf_attn_decode.argtypes = [P, P, P, P, P, P, PI32, PI32, I64, I64,
                                   I64, I64, I64, I64, F, P]
    if hasattr(lib, "kf_decode_rope_store"):
        lib.kf_decode_rope_store.restype = I32
        lib.kf_decode_rope_store.argtypes = [P, P, P, P, FP, FP, PI32, P,
                                             I64, I64, I64, I64, I64, P]


def check(err: int, name: str) -> None:
    if err != 0:
        raise RuntimeError(f"HIP kernel {name} failed with hipError_t={err}")
