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
        lib = ctypes.CDLL(str(_LIB_PATH))
    except OSError as e:  # pragma: no cover
        _load_error = str(e)
        return None
    _configure(lib)  # raises, naming the symbol, if one is missing
    _lib = lib
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


# The C ABI of libkfops.so as data: entry point -> argtypes, one entry per
# prototype in csrc/kf_ops.h (tests/test_ops_abi.py checks the two against
# each other). Every entry point returns hipError_t as int, except the
# *_nparts helpers, which return a count as int64.
_P, _F = ctypes.c_void_p, ctypes.c_float
_I64, _I32 = ctypes.c_int64, ctypes.c_int
_FP = ctypes.POINTER(ctypes.c_float)
_PI64 = ctypes.POINTER(ctypes.c_int64)
_PI32 = ctypes.POINTER(ctypes.c_int32)

# dq, q, k, v, dout, lse, delta, B, S, Hq, Hkv, qts, kts, dqts, scale, causal
_DQ8 = [_P] * 5 + [_FP, _FP] + [_I64] * 7 + [_F, _I32]
_DKV8 = [_P] + _DQ8                 # dk, dv lead instead of dq; dkts for dqts
_ROPE_TAIL = [_FP, _FP, _I64]       # cos, sin, pos_offset before the stream
# dq, dk, dv, dout, q, k, v, o, lse, delta, B, S, Hq, Hkv
_BWD_HEAD = [_P] * 8 + [_FP, _FP] + [_I64] * 4
# D, qts, kts, dqts, dkts, scale, causal
_ATTN_BWD = _BWD_HEAD + [_I64] * 5 + [_F, _I32]
# o, lse, q, k, v, B, S, Hq, Hkv, D, qts, kts, scale, causal, stream
_ATTN_FWD = [_P, _FP, _P, _P, _P] + [_I64] * 7 + [_F, _I32, _P]

SIGNATURES: dict[str, list] = {
    "kf_rmsnorm_fwd": [_P, _FP, _P, _P, _I64, _I64, _F, _P],
    "kf_rmsnorm_bwd_nparts": [_I64],
    "kf_rmsnorm_bwd": [_P, _P, _FP, _P, _P, _P, _FP, _I64, _I64, _P],
    "kf_rmsnorm_bwd_res": [_P, _P, _FP, _P, _P, _P, _FP, _P, _I64, _I64, _P],
    "kf_layernorm_fwd": [_P, _FP, _FP, _P, _P, _P, _I64, _I64, _F, _P],
    "kf_layernorm_bwd_nparts": [_I64],
    "kf_layernorm_bwd": [_P, _P, _P, _FP, _P, _P, _P, _FP, _FP, _I64, _I64,
                         _P],
    "kf_rope": [_P, _P, _FP, _FP, _PI64] + [_I64] * 8 + [_I32, _P],
    "kf_swiglu_fwd": [_P, _P, _I64, _I64, _P],
    "kf_swiglu_bwd": [_P, _P, _P, _I64, _I64, _P],
    "kf_adamw": [_P, _FP, _P, _FP, _FP, _FP, _I64, _F, _F, _F, _F, _F, _I64,
                 _P],
    # p16, p32, g, m, v, wd_mask, wd_groups, gscale, n, lr..wd, step, stream
    "kf_adamw_clip": [_P, _FP, _P, _FP, _FP, _FP, _P, _FP, _I64, _F, _F, _F,
                      _F, _F, _I64, _P],
    "kf_grad_sumsq_nparts": [_I64],
    "kf_grad_sumsq": [_FP, _FP, _P, _I64, _P],
    "kf_ce_fwd": [_FP, _FP, _P, _PI64, _I64, _I64, _I64, _P],
    "kf_ce_bwd": [_P, _P, _FP, _PI64, _FP, _I64, _I64, _I64, _P],
    "kf_skinny_gemm": [_P, _P, _P, _P] + [_I64] * 6 + [_P],
    "kf_skinny_gemm_q8": [_P, _P, _P, _FP, _P] + [_I64] * 6 + [_P],
    # c, a, w_bank | w8, wscale, offsets, a_rows, n_groups, max_rows,
    # total_rows, a_nrows, N, K, stream
    "kf_skinny_gemm_grouped": [_P, _P, _P, _PI32, _PI32] + [_I64] * 6 + [_P],
    "kf_skinny_gemm_grouped_q8": [_P, _P, _P, _FP, _PI32, _PI32] +
                                 [_I64] * 6 + [_P],
    "kf_kv_store": [_P] * 6 + [_I64, _I64, _I64, _P],
    "kf_decode_rope_store": [_P, _P, _P, _P, _FP, _FP, _PI32, _P] +
                            [_I64] * 5 + [_P],
    "kf_attn_fwd": _ATTN_FWD,
    "kf_attn_fwd4": _ATTN_FWD,
    # ..., B, Sq, Skv, Hq, Hkv, D, qts, kts, scale, qoff, stream
    "kf_attn_fwd4_rect": [_P, _FP, _P, _P, _P] + [_I64] * 8 + [_F, _I64, _P],
    # scripts/attn_ablate.py, scripts/probe_tr16.py
    "kf_attn_fwd4_abl": [_I32] + _ATTN_FWD,
    "kf_tr16_probe": [_P, _P, _I32, _P],
    "kf_attn_bwd": _ATTN_BWD + [_P],
    "kf_attn_bwd_rope": _ATTN_BWD + _ROPE_TAIL + [_P],
    # per-pass entry points of the 8-wave backward (tests / bisection)
    "kf_attn_bwd8_dq": _DQ8 + [_P],
    "kf_attn_bwd8_dq_rope": _DQ8 + _ROPE_TAIL + [_P],
    "kf_attn_bwd8_dkv": _DKV8 + [_P],
    "kf_attn_bwd8_dkv_rope": _DKV8 + _ROPE_TAIL + [_P],
    "kf_attn_bwd8_dkv_fused": _DKV8 + [_P],
    "kf_attn_bwd8_dkv_fused_rope": _DKV8 + _ROPE_TAIL + [_P],
    # head-dim-64 family: ..., qts, kts, scale, causal, kv_len, stream
    "kf_attn64_fwd": [_P, _FP, _P, _P, _P] + [_I64] * 6 + [_F, _I32, _I64,
                                                           _P],
    "kf_attn64_bwd": _BWD_HEAD + [_I64, _I64, _F, _I32, _I64, _P],
    # ..., seq_lens, B, S, Hq, Hkv, qts, kts, scale, stream
    "kf_attn64_fwd_varlen": [_P, _FP, _P, _P, _P, _PI32] + [_I64] * 6 +
                            [_F, _P],
    "kf_attn64_bwd_varlen": _BWD_HEAD[:10] + [_PI32] + [_I64] * 6 + [_F, _P],
    "kf_attn_decode": [_P] * 6 + [_PI32, _PI32] + [_I64] * 6 + [_F, _P],
    # mixture of experts (moe.hip): ..., T, E | k | h ..., stream
    "kf_moe_route": [_P, _FP, _P, _P, _I64, _I64, _I64, _P],
    "kf_moe_route_bwd": [_P, _P, _FP, _P, _I64, _I64, _I64, _P],
    "kf_moe_sort_nwork": [_I64, _I64, _I64],
    # pos, src, offsets, work, topi, T, k, e_lo, n_local, stream
    "kf_moe_sort": [_P] * 5 + [_I64] * 4 + [_P],
    "kf_moe_gather": [_P, _P, _P, _I64, _I64, _I64, _P],       # M, T, h
    "kf_moe_gather_bwd": [_P, _P, _P] + [_I64] * 4 + [_P],     # T, k, h, M
    "kf_moe_combine": [_P] * 4 + [_I64] * 4 + [_P],
    "kf_moe_combine_bwd": [_P] * 6 + [_I64] * 4 + [_P],
}
_RETURNS_INT64 = ("kf_rmsnorm_bwd_nparts", "kf_layernorm_bwd_nparts",
                  "kf_grad_sumsq_nparts", "kf_moe_sort_nwork")


def _configure(lib: ctypes.CDLL) -> None:
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RuntimeError(
                f"{_LIB_PATH.name} does not export {name}: the library and "
                "kubeflow_amd/ops/_backend.py disagree") from None
        fn.restype = _I64 if name in _RETURNS_INT64 else _I32
        fn.argtypes = argtypes


def check(err: int, name: str) -> None:
    if err != 0:
        raise RuntimeError(f"HIP kernel {name} failed with hipError_t={err}")
