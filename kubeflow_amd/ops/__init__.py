"""kubeflow_amd.ops — the hot-op library (CDNA4 HIP kernels + CPU reference).

Dispatch policy:
  * CUDA (= ROCm/HIP) tensors -> hand-written gfx950 kernels in libkfops.so,
    loaded via ctypes (`_backend`). Missing library on a GPU box raises —
    no silent eager fallback (KF_NATIVE_KERNELS=0 is the explicit escape
    hatch for bisection).
  * CPU tensors -> the pure-torch reference implementations (differentiable),
    so the full stack runs in CPU-only CI.

All ops are exposed as autograd-capable functions:
  rms_norm, rope, flash_attention, cross_entropy, fused_adamw (no autograd),
  moe_route / moe_gather / grouped_linear / moe_combine (the MoE block);
  grouped_skinny_linear / moe_experts_decode (its decode form: inference
  only, no host sync).
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import Optional

import torch

from . import reference
from . import _backend

__all__ = [
    "rms_norm", "layer_norm", "rope", "flash_attention", "attention_decode",
    "flash_attention_rect", "skinny_linear", "kv_store",
    "decode_rope_store", "skinny_linear_q8", "quantize_fp8_rows",
    "dequantize_fp8_rows",
    "cross_entropy", "fused_adamw", "rope_cos_sin", "native_available",
    "masked_attention",
    "swiglu", "fused_qkv_attention",
    "rms_norm_residual", "grad_norm", "step_tail_enabled",
    "MoeRouting", "moe_route", "moe_gather", "moe_combine", "grouped_linear",
    "moe_experts", "moe_native_ok",
    "grouped_skinny_ok", "grouped_skinny_linear", "grouped_skinny_linear_q8",
    "moe_experts_decode",
]

rope_cos_sin = reference.rope_cos_sin


def native_available() -> bool:
    return _backend.try_load() is not None


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _fp(t: Optional[torch.Tensor]):
    return ctypes.cast(0 if t is None else t.data_ptr(),
                       ctypes.POINTER(ctypes.c_float))


def _ip(t: torch.Tensor):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int64))


def _ip_or_null(t):
    if t is None:
        return ctypes.cast(0, ctypes.POINTER(ctypes.c_int64))
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int64))


def _i32p(t):
    if t is None:
        return ctypes.cast(0, ctypes.POINTER(ctypes.c_int32))
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32))


def _index_arg(op: str, name: str, t, dtype: torch.dtype, n: int,
               like: torch.Tensor) -> None:
    """The kernels read index tensors through a bare pointer at a fixed
    width: `t` must be a contiguous `dtype` tensor of shape [n] on `like`'s
    device, or the launch would scatter to (or read from) the wrong rows.
    Metadata only: no host sync and no value check, so it is safe under
    graph capture."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(
            f"{op}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(
            f"{op}: {name} must be {dtype} (the kernel reads it at that "
            f"width), got {t.dtype}")
    if t.device != like.device:
        raise ValueError(
            f"{op}: {name} must be on {like.device}, got {t.device}")
    if tuple(t.shape) != (n,):
        raise ValueError(
            f"{op}: {name} must have shape [{n}], got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{op}: {name} must be contiguous")


def _use_native(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    if _backend.native_enabled():
        _backend.require()
        return True
    return False


# --------------------------------------------------------------- RMSNorm --

class _RMSNormHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        lib = _backend.require()
        shape = x.shape
        x2 = x.contiguous().view(-1, shape[-1])
        rows, cols = x2.shape
        y = torch.empty_like(x2)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _backend.check(
            lib.kf_rmsnorm_fwd(_p(y), _fp(rstd), _p(x2), _p(weight), rows,
                               cols, float(eps), _stream()), "rmsnorm_fwd")
        ctx.save_for_backward(x2, weight, rstd)
        ctx.shape = shape
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        lib = _backend.require()
        x2, weight, rstd = ctx.saved_tensors
        rows, cols = x2.shape
        dy2 = dy.contiguous().view(rows, cols)
        dx = torch.empty_like(x2)
        dw = torch.empty_like(weight)
        dw_part = torch.zeros(cols, dtype=torch.float32, device=x2.device)
        _backend.check(
            lib.kf_rmsnorm_bwd(_p(dx), _p(dw), _fp(dw_part), _p(dy2), _p(x2),
                               _p(weight), _fp(rstd), rows, cols, _stream()),
            "rmsnorm_bwd")
        return dx.view(ctx.shape), dw, None


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5):
    if _use_native(x):
        return _RMSNormHip.apply(x, weight, eps)
    return reference.rms_norm(x, weight, eps)


def _norm_res_enabled() -> bool:
    """KF_NORM_RES=0: bisection switch — rms_norm_residual composes rms_norm
    with a pass-through x, and autograd sums the two gradients of x with its
    own add kernel."""
    return os.environ.get("KF_NORM_RES", "1") != "0"


class _RMSNormResHip(torch.autograd.Function):
    """RMSNorm that also hands its input back: (y, x). A block's x feeds the
    norm and the residual add; routing the residual branch through this
    node brings both gradients of x to one backward, which adds the
    residual's in the store of kf_rmsnorm_bwd_res instead of leaving the sum
    to a separate bf16 add pass over [rows, cols]."""

    @staticmethod
    def forward(ctx, x, weight, eps):
        lib = _backend.require()
        shape = x.shape
        x2 = x.contiguous().view(-1, shape[-1])
        rows, cols = x2.shape
        y = torch.empty_like(x2)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _backend.check(
            lib.kf_rmsnorm_fwd(_p(y), _fp(rstd), _p(x2), _p(weight), rows,
                               cols, float(eps), _stream()), "rmsnorm_fwd")
        ctx.save_for_backward(x2, weight, rstd)
        ctx.shape = shape
        ctx.set_materialize_grads(False)
        return y.view(shape), x

    @staticmethod
    def backward(ctx, dy, dxr):
        if dy is None:  # only the pass-through was used
            return dxr, None, None
        lib = _backend.require()
        x2, weight, rstd = ctx.saved_tensors
        rows, cols = x2.shape
        dy2 = dy.contiguous().view(rows, cols)
        dx = torch.empty_like(x2)
        dw = torch.empty_like(weight)
        dw_part = torch.zeros(cols, dtype=torch.float32, device=x2.device)
        if (dxr is not None and dxr.is_contiguous()
                and dxr.dtype == dx.dtype and dxr.data_ptr() % 16 == 0):
            _backend.check(
                lib.kf_rmsnorm_bwd_res(_p(dx), _p(dw), _fp(dw_part), _p(dy2),
                                       _p(x2), _p(weight), _fp(rstd),
                                       _p(dxr), rows, cols, _stream()),
                "rmsnorm_bwd_res")
            return dx.view(ctx.shape), dw, None
        _backend.check(
            lib.kf_rmsnorm_bwd(_p(dx), _p(dw), _fp(dw_part), _p(dy2), _p(x2),
                               _p(weight), _fp(rstd), rows, cols, _stream()),
            "rmsnorm_bwd")
        dx = dx.view(ctx.shape)
        return (dx if dxr is None else dx + dxr), dw, None


def rms_norm_residual(x: torch.Tensor, weight: torch.Tensor,
                      eps: float = 1e-5):
    """(rms_norm(x), x) for a pre-norm residual block: use the returned x,
    not the argument, as the residual input. Values are rms_norm's; on the
    GPU the backward makes one kernel call for both gradients of x."""
    if _use_native(x):
        if _norm_res_enabled():
            return _RMSNormResHip.apply(x, weight, eps)
        return _RMSNormHip.apply(x, weight, eps), x
    return reference.rms_norm(x, weight, eps), x


# ------------------------------------------------------------------ RoPE --

class _RopeHip(torch.autograd.Function):
    """Joint rotary embedding on (q, k); in-place rotation on fresh clones."""

    @staticmethod
    def forward(ctx, q, k, cos, sin, pos_offset, positions):
        lib = _backend.require()
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        # clone(contiguous_format) compacts strided inputs in ONE copy
        # (the QKV-split views are always strided; .contiguous().clone()
        # would copy twice)
        q = q.clone(memory_format=torch.contiguous_format)
        k = k.clone(memory_format=torch.contiguous_format)
        _backend.check(
            lib.kf_rope(_p(q), _p(k), _fp(cos), _fp(sin),
                        _ip_or_null(positions), B, S, Hq, Hkv, D,
                        Hq * D, Hkv * D, pos_offset, 0, _stream()),
            "rope_fwd")
        ctx.save_for_backward(cos, sin, *(
            [positions] if positions is not None else []))
        ctx.dims = (B, S, Hq, Hkv, D, pos_offset)
        return q, k

    @staticmethod
    def backward(ctx, dq, dk):
        lib = _backend.require()
        cos, sin = ctx.saved_tensors[0], ctx.saved_tensors[1]
        positions = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        B, S, Hq, Hkv, D, pos_offset = ctx.dims
        dq = dq.clone(memory_format=torch.contiguous_format)
        dk = dk.clone(memory_format=torch.contiguous_format)
        _backend.check(
            lib.kf_rope(_p(dq), _p(dk), _fp(cos), _fp(sin),
                        _ip_or_null(positions), B, S, Hq, Hkv, D,
                        Hq * D, Hkv * D, pos_offset, 1, _stream()),
            "rope_bwd")
        return dq, dk, None, None, None, None


def rope(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor,
         sin: torch.Tensor, pos_offset: int = 0,
         positions: Optional[torch.Tensor] = None):
    """q [B,S,Hq,D], k [B,S,Hkv,D]; cos/sin fp32 [>=S+off, D/2].
    positions: optional int64 [B] per-row base position (serving decode)."""
    if _use_native(q):
        if positions is not None:
            _index_arg("rope", "positions", positions, torch.int64,
                       q.shape[0], q)
        return _RopeHip.apply(q, k, cos, sin, pos_offset, positions)
    if positions is not None:
        qs = [reference.rope_apply(q[i:i+1], cos, sin, int(positions[i]))
              for i in range(q.shape[0])]
        ks = [reference.rope_apply(k[i:i+1], cos, sin, int(positions[i]))
              for i in range(k.shape[0])]
        return torch.cat(qs), torch.cat(ks)
    return (reference.rope_apply(q, cos, sin, pos_offset),
            reference.rope_apply(k, cos, sin, pos_offset))


def kv_store(cache_k: torch.Tensor, cache_v: torch.Tensor,
             k: torch.Tensor, v: torch.Tensor, slots: torch.Tensor,
             positions: torch.Tensor) -> None:
    """Scatter this decode step's k/v token rows into cache row
    [slot[i], position[i]] for each sequence i — one launch instead of two
    advanced-indexing kernels per layer (kv_store.hip). cache_k/v
    [SLOTS,SMAX,Hkv,D]; k/v [N,1,Hkv,D] (or [N,Hkv,D]); slots int32 [N];
    positions int64 [N] (the kernel reads them at that width: on the native
    path another dtype, device, length or a strided tensor raises).
    Capture-safe; no autograd (serving only)."""
    n = k.shape[0]
    row = cache_k.shape[2] * cache_k.shape[3]
    if _use_native(k) and k.dtype == torch.bfloat16 and row % 8 == 0:
        lib = _backend.require()
        _index_arg("kv_store", "slots", slots, torch.int32, n, k)
        _index_arg("kv_store", "positions", positions, torch.int64, n, k)
        kk, vv = k.reshape(n, row), v.reshape(n, row)
        if not kk.is_contiguous():
            kk = kk.contiguous()
        if not vv.is_contiguous():
            vv = vv.contiguous()
        _backend.check(
            lib.kf_kv_store(_p(cache_k), _p(cache_v), _p(kk), _p(vv),
                            _i32p(slots), _p(positions), cache_k.shape[1],
                            row, n, _stream()), "kv_store")
        return
    cache_k[slots.long(), positions] = k.reshape(n, *cache_k.shape[2:])
    cache_v[slots.long(), positions] = v.reshape(n, *cache_v.shape[2:])


def _skinny_shape_ok(rows: int, N: int, K: int, q8: bool) -> bool:
    """The shape rule of skinny_gemm.hip for `rows` batch rows against
    [N, K] weights: the LDS kernel takes K % 512 == 0 (q8: K % 1024 == 0)
    up to 32 rows, the direct bf16 kernel K % 32 == 0 up to 16 rows."""
    if not 1 <= rows <= 32 or N % 16:
        return False
    if q8:
        return K % 1024 == 0
    return K % 512 == 0 or (K % 32 == 0 and rows <= 16)


def _skinny(x, w, scale, residual):
    """Shared body of the two skinny linears; scale None = bf16 weight."""
    shape = x.shape
    M = 1
    for d in shape[:-1]:
        M *= int(d)
    K = shape[-1]
    N = w.shape[0]
    if (not _use_native(x) or x.dtype != torch.bfloat16
            or not _skinny_shape_ok(M, N, K, scale is not None)):
        wb = w if scale is None else dequantize_fp8_rows(w, scale, x.dtype)
        y = torch.nn.functional.linear(x, wb)
        return y + residual if residual is not None else y
    lib = _backend.require()
    x2 = x.reshape(M, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    r2 = None
    if residual is not None:
        r2 = residual.reshape(M, N)
        if not r2.is_contiguous():
            r2 = r2.contiguous()
    y = torch.empty(M, N, dtype=x.dtype, device=x.device)
    if scale is None:
        _backend.check(
            lib.kf_skinny_gemm(_p(y), _p(x2), _p(w), _p(r2), M, N, K,
                               K, 0, 0, _stream()),
            "skinny_gemm")
    else:
        _backend.check(
            lib.kf_skinny_gemm_q8(_p(y), _p(x2), _p(w), _fp(scale), _p(r2),
                                  M, N, K, K, 0, 0, _stream()),
            "skinny_gemm_q8")
    return y.view(*shape[:-1], N)


def skinny_linear(x: torch.Tensor, weight: torch.Tensor,
                  residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode-batch linear y = x @ W^T (+ residual) for small leading dims
    (M <= 32): the LDS-staged weight-streaming kernel (skinny_gemm.hip)
    replaces hipBLASLt's ~30-50%-of-BW GEMV path in the serving decode
    step; `residual` fuses the following elementwise add into the
    epilogue. Falls back to F.linear off-GPU or for larger M /
    unsupported shapes. Inference-only (no autograd)."""
    return _skinny(x, weight, None, residual)


def quantize_fp8_rows(w: torch.Tensor):
    """Per-output-row OCP e4m3 weight quantization for the W8A16 decode
    path: scale = absmax/448 per row, w8 = round(w/scale) in e4m3fn.
    Returns (w8 uint8 [N,K], scale fp32 [N])."""
    with torch.no_grad():  # w is usually a requires-grad Parameter — the
        # fp32 temps would otherwise be RETAINED by autograd (141 GB of
        # them for llama3-70b)
        wf = w.detach().float()
        scale = wf.abs().amax(dim=1).clamp_min(1e-12) / 448.0
        q = (wf / scale.unsqueeze(1)).to(torch.float8_e4m3fn)
        return q.view(torch.uint8).contiguous(), scale.contiguous()


def dequantize_fp8_rows(w8: torch.Tensor, scale: torch.Tensor,
                        dtype=torch.bfloat16) -> torch.Tensor:
    return (w8.view(torch.float8_e4m3fn).float()
            * scale.unsqueeze(1)).to(dtype)


def skinny_linear_q8(x: torch.Tensor, w8: torch.Tensor,
                     scale: torch.Tensor,
                     residual: Optional[torch.Tensor] = None
                     ) -> torch.Tensor:
    """Quantized decode linear y = x @ dequant(W8)^T (+ residual): fp8
    weights halve the HBM traffic of the weight-BW-bound decode GEMMs
    (skinny_gemm.hip kf_skinny_q8_kernel); activations stay bf16 and the
    MFMA runs bf16 (W8A16). Serving-only, behind KF_SERVE_QUANT=fp8."""
    return _skinny(x, w8, scale, residual)


def decode_rope_store(qkv: torch.Tensor, cache_k: torch.Tensor,
                      cache_v: torch.Tensor, cos: torch.Tensor,
                      sin: torch.Tensor, slots: torch.Tensor,
                      positions: torch.Tensor, n_heads: int,
                      n_kv_heads: int) -> torch.Tensor:
    """Fused decode-step RoPE + cache scatter (decode_fused.hip): consume
    the fused QKV projection [N, 1, (Hq+2*Hkv)*D] directly — rotate q and
    k, write q to a fresh [N, Hq, D] tensor, scatter rotated k and copied
    v into cache row [slot[i], position[i]]. Replaces split + rope clones
    + kv_store (~4 launches and two D2D copies per layer). Serving only
    (no autograd); capture-safe."""
    D = cache_k.shape[3]
    n = qkv.shape[0]
    q = torch.empty(n, n_heads, D, dtype=qkv.dtype, device=qkv.device)
    if (_use_native(qkv) and qkv.dtype == torch.bfloat16 and D == 128):
        lib = _backend.require()
        _index_arg("decode_rope_store", "slots", slots, torch.int32, n, qkv)
        _index_arg("decode_rope_store", "positions", positions, torch.int64,
                   n, qkv)
        q3 = qkv.reshape(n, -1)
        if not q3.is_contiguous():
            q3 = q3.contiguous()
        _backend.check(
            lib.kf_decode_rope_store(_p(q), _p(cache_k), _p(cache_v),
                                     _p(q3), _fp(cos), _fp(sin),
                                     _i32p(slots), _p(positions), n,
                                     n_heads, n_kv_heads, D,
                                     cache_k.shape[1], _stream()),
            "decode_rope_store")
        return q
    # reference path: split + rope + indexed store
    qq, kk, vv = qkv.reshape(n, 1, -1).split(
        [n_heads * D, n_kv_heads * D, n_kv_heads * D], dim=-1)
    qq = qq.view(n, 1, n_heads, D)
    kk = kk.view(n, 1, n_kv_heads, D)
    vv = vv.view(n, 1, n_kv_heads, D)
    qq, kk = rope(qq, kk, cos, sin, positions=positions)
    kv_store(cache_k, cache_v, kk, vv, slots, positions)
    return qq.reshape(n, n_heads, D)


# ------------------------------------------------------- Flash attention --

class _FlashAttnHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale):
        lib = _backend.require()
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o = torch.empty_like(q)
        lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        _backend.check(
            lib.kf_attn_fwd(_p(o), _fp(lse), _p(q), _p(k), _p(v), B, S, Hq,
                            Hkv, D, 0, 0, float(scale), int(causal),
                            _stream()), "attn_fwd")
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.meta = (causal, scale)
        return o

    @staticmethod
    def backward(ctx, dout):
        lib = _backend.require()
        q, k, v, o, lse = ctx.saved_tensors
        causal, scale = ctx.meta
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        dout = dout.contiguous()
        dq = torch.empty_like(q)
        dk = torch.empty_like(k)
        dv = torch.empty_like(v)
        delta = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        _backend.check(
            lib.kf_attn_bwd(_p(dq), _p(dk), _p(dv), _p(dout), _p(q), _p(k),
                            _p(v), _p(o), _fp(lse), _fp(delta), B, S, Hq, Hkv,
                            D, 0, 0, 0, 0, float(scale), int(causal),
                            _stream()), "attn_bwd")
        return dq, dk, dv, None, None


_ATTN_DIMS = (64, 128)  # head dims with a native attention family


def _attn64_enabled() -> bool:
    """KF_ATTN_D64=0: bisection switch — D == 64 attention on the GPU runs
    the torch reference math instead of attention_d64.hip."""
    return os.environ.get("KF_ATTN_D64", "1") != "0"


def _check_head_dim(D: int) -> None:
    if D not in _ATTN_DIMS:
        raise ValueError(
            f"native attention supports head_dim in {_ATTN_DIMS}, got {D}")


def _row_stride(t: torch.Tensor) -> Optional[int]:
    """Token-row stride (elements) if the kernels can read t [B,S,H,D] in
    place — heads packed, uniform row stride across the batch, 16-byte
    aligned (the split views of a fused QKV projection) — else None."""
    B, S, H, D = t.shape
    rs = t.stride(1)
    if (t.stride(3) == 1 and t.stride(2) == D and rs >= H * D and rs % 8 == 0
            and (B == 1 or t.stride(0) == S * rs)
            and t.data_ptr() % 16 == 0):
        return rs
    return None


def _attn64_fwd(q, k, v, causal, scale, kv_len):
    """kf_attn64_fwd on [B,S,H,64] bf16 tensors, S % 128 == 0. Returns
    (o, lse, q, k, v, qts, kts) with q/k/v as actually passed."""
    lib = _backend.require()
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    qts = _row_stride(q)
    if qts is None:
        q = q.contiguous()
        qts = Hq * D
    kts = _row_stride(k)
    if kts is None or _row_stride(v) != kts:
        k, v = k.contiguous(), v.contiguous()
        kts = Hkv * D
    o = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
    _backend.check(
        lib.kf_attn64_fwd(_p(o), _fp(lse), _p(q), _p(k), _p(v), B, S, Hq,
                          Hkv, qts, kts, float(scale), int(causal),
                          int(kv_len), _stream()), "attn64_fwd")
    return o, lse, q, k, v, qts, kts


class _FlashAttn64Hip(torch.autograd.Function):
    """Head-dim-64 family (attention_d64.hip): forward + deterministic
    two-pass backward, kv rows >= kv_len never attended."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, kv_len):
        o, lse, q, k, v, qts, kts = _attn64_fwd(q, k, v, causal, scale,
                                                kv_len)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.meta = (causal, scale, kv_len, qts, kts)
        return o

    @staticmethod
    def backward(ctx, dout):
        lib = _backend.require()
        q, k, v, o, lse = ctx.saved_tensors
        causal, scale, kv_len, qts, kts = ctx.meta
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        dout = dout.contiguous()
        dq = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
        dk = torch.empty(B, S, Hkv, D, dtype=k.dtype, device=k.device)
        dv = torch.empty_like(dk)
        delta = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        _backend.check(
            lib.kf_attn64_bwd(_p(dq), _p(dk), _p(dv), _p(dout), _p(q), _p(k),
                              _p(v), _p(o), _fp(lse), _fp(delta), B, S, Hq,
                              Hkv, qts, kts, float(scale), int(causal),
                              int(kv_len), _stream()), "attn64_bwd")
        return dq, dk, dv, None, None, None


def _pad_rows(t: torch.Tensor, pad: int) -> torch.Tensor:
    return torch.cat(
        [t, t.new_zeros(t.shape[0], pad, t.shape[2], t.shape[3])], dim=1)


def _flash_attention64(q, k, v, causal, scale, kv_len):
    """D == 64 native route: any S (zero-padded to a 128 multiple; for
    non-causal input the pad rows are masked through kv_len, padded q rows
    are sliced off and so receive zero dout)."""
    if q.dtype != torch.bfloat16:
        raise ValueError(f"native attention needs bf16 inputs, got {q.dtype}")
    S = q.shape[1]
    if kv_len is None:
        kv_len = S
    pad = (128 - S % 128) % 128
    if pad:
        q, k, v = _pad_rows(q, pad), _pad_rows(k, pad), _pad_rows(v, pad)
        if causal:
            kv_len = S + pad  # pad keys are causally masked for real queries
    o = _FlashAttn64Hip.apply(q, k, v, causal, scale, kv_len)
    return o[:, :S] if pad else o


class _FlashAttn64VarlenHip(torch.autograd.Function):
    """Head-dim-64 family with per-sequence lengths (kf_attn64_*_varlen):
    rows >= seq_lens[b] are padding on both axes; o and all three gradients
    are exact zeros there. Non-causal."""

    @staticmethod
    def forward(ctx, q, k, v, scale, seq_lens):
        lib = _backend.require()
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        qts = _row_stride(q)
        if qts is None:
            q = q.contiguous()
            qts = Hq * D
        kts = _row_stride(k)
        if kts is None or _row_stride(v) != kts:
            k, v = k.contiguous(), v.contiguous()
            kts = Hkv * D
        o = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
        lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        _backend.check(
            lib.kf_attn64_fwd_varlen(_p(o), _fp(lse), _p(q), _p(k), _p(v),
                                     _i32p(seq_lens), B, S, Hq, Hkv, qts,
                                     kts, float(scale), _stream()),
            "attn64_fwd_varlen")
        ctx.save_for_backward(q, k, v, o, lse, seq_lens)
        ctx.meta = (scale, qts, kts)
        return o

    @staticmethod
    def backward(ctx, dout):
        lib = _backend.require()
        q, k, v, o, lse, seq_lens = ctx.saved_tensors
        scale, qts, kts = ctx.meta
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        dout = dout.contiguous()
        dq = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
        dk = torch.empty(B, S, Hkv, D, dtype=k.dtype, device=k.device)
        dv = torch.empty_like(dk)
        delta = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        _backend.check(
            lib.kf_attn64_bwd_varlen(_p(dq), _p(dk), _p(dv), _p(dout), _p(q),
                                     _p(k), _p(v), _p(o), _fp(lse),
                                     _fp(delta), _i32p(seq_lens), B, S, Hq,
                                     Hkv, qts, kts, float(scale), _stream()),
            "attn64_bwd_varlen")
        return dq, dk, dv, None, None


def _flash_attention64_varlen(q, k, v, scale, seq_lens):
    """D == 64 native route with per-sequence lengths: any S (zero-padded to
    a 128 multiple; the pad rows are past every length, so the lengths need
    no adjustment and the padded rows come back as zeros and are sliced
    off)."""
    if q.dtype != torch.bfloat16:
        raise ValueError(f"native attention needs bf16 inputs, got {q.dtype}")
    S = q.shape[1]
    pad = (128 - S % 128) % 128
    if pad:
        q, k, v = _pad_rows(q, pad), _pad_rows(k, pad), _pad_rows(v, pad)
    o = _FlashAttn64VarlenHip.apply(q, k, v, scale, seq_lens)
    return o[:, :S] if pad else o


def _seq_lens_arg(seq_lens, q):
    """seq_lens as flash_attention takes it -> int32 [B] on q's device. An
    int32 tensor already there is used as is (no host sync, no validation:
    the kernels clamp); anything else is checked on the host and moved."""
    B, S = q.shape[0], q.shape[1]
    if (isinstance(seq_lens, torch.Tensor) and seq_lens.device == q.device
            and seq_lens.dtype == torch.int32 and q.is_cuda):
        if seq_lens.shape != (B,):
            raise ValueError(
                f"seq_lens must have shape [{B}], got {tuple(seq_lens.shape)}")
        return seq_lens.contiguous()
    host = torch.as_tensor(seq_lens).detach().cpu()
    if host.shape != (B,) or host.is_floating_point():
        raise ValueError(
            f"seq_lens must be {B} integers, got shape {tuple(host.shape)} "
            f"dtype {host.dtype}")
    if int(host.min()) < 1 or int(host.max()) > S:
        raise ValueError(
            f"seq_lens must be in [1, {S}], got {host.tolist()}")
    return host.to(device=q.device, dtype=torch.int32)


def _sdpa_ref_varlen(q, k, v, scale, seq_lens):
    """Reference math per sequence (differentiable): reference.sdpa on the
    [:L] slices, scattered into zeros — the kernels' zero-row semantics, so
    o and every gradient are exactly zero past each length."""
    lens = seq_lens.tolist()
    S = q.shape[1]
    rows = []
    for b, L in enumerate(lens):
        L = min(max(int(L), 1), S)
        ob = reference.sdpa(q[b:b + 1, :L].transpose(1, 2),
                            k[b:b + 1, :L].transpose(1, 2),
                            v[b:b + 1, :L].transpose(1, 2),
                            causal=False, scale=scale).transpose(1, 2)
        rows.append(torch.cat(
            [ob, ob.new_zeros(1, S - L, ob.shape[2], ob.shape[3])], dim=1))
    return torch.cat(rows, dim=0)


def _sdpa_ref(q, k, v, causal, scale, kv_len):
    """Reference math in bshd (differentiable): k/v sliced to kv_len, so
    autograd yields zero gradient rows past it."""
    if kv_len is not None:
        k, v = k[:, :kv_len], v[:, :kv_len]
    o = reference.sdpa(q.transpose(1, 2), k.transpose(1, 2),
                       v.transpose(1, 2), causal=causal, scale=scale)
    return o.transpose(1, 2)


def flash_attention_rect(q: torch.Tensor, k: torch.Tensor,
                         v: torch.Tensor, q_offset: int,
                         scale: Optional[float] = None) -> torch.Tensor:
    """Rectangular-causal attention for chunked prefill (inference only,
    no autograd): q [B, C, Hq, D] holds C query rows at global offset
    q_offset; k/v [B, Skv, Hkv, D] hold the KV prefix INCLUDING the chunk
    (Skv >= q_offset + C). Row i attends kv <= q_offset + i.

    Native path: kf_attn_fwd4_rect (attention_fwd4.hip) — q is padded to a
    256-row multiple and the kv buffers must have row capacity up to the
    next 64 multiple of Skv (the serving KV-cache slabs do; this wrapper
    re-pads otherwise)."""
    B, C, Hq, D = q.shape
    Skv = k.shape[1]
    Hkv = k.shape[2]
    if scale is None:
        scale = D ** -0.5
    assert Skv >= q_offset + C, (Skv, q_offset, C)
    if _use_native(q):
        lib = _backend.require()
        pad = (256 - C % 256) % 256
        if pad:
            q = torch.cat([q, q.new_zeros(B, pad, Hq, D)], dim=1)
        o = torch.empty_like(q)
        lse = torch.empty(B, Hq, q.shape[1], dtype=torch.float32,
                          device=q.device)
        q = q.contiguous()
        # rows must be contiguous [.., Hkv, D] and the buffer must extend
        # to the next KV-TILE multiple of Skv (A4_KT=64 in
        # attention_fwd4.hip; 128 kept for headroom if the tile grows)
        need = (Skv + 127) // 128 * 128
        # the kernel's kv batch stride is b * Sq_padded rows, so the
        # zero-copy fast path is B == 1 only (the serving slabs)
        def _rows_ok(t):
            return (B == 1 and t.stride(1) == Hkv * D and t.stride(2) == D
                    and t.stride(3) == 1
                    and t.stride(0) // (Hkv * D) >= need)
        if not (_rows_ok(k) and _rows_ok(v)):
            rows = max(need, q.shape[1])
            if B > 1 and rows != q.shape[1]:
                raise ValueError(
                    "batched rectangular attention requires Skv <= padded "
                    f"Sq (kernel batch stride); got Skv={Skv} B={B}")
            kp = torch.zeros(B, rows, Hkv, D, dtype=k.dtype, device=k.device)
            vp = torch.zeros_like(kp)
            kp[:, :Skv] = k[:, :Skv]
            vp[:, :Skv] = v[:, :Skv]
            k, v = kp, vp
        _backend.check(
            lib.kf_attn_fwd4_rect(_p(o), _fp(lse), _p(q), _p(k), _p(v),
                                  B, q.shape[1], Skv, Hq, Hkv, D,
                                  0, Hkv * D,
                                  ctypes.c_float(float(scale)), q_offset,
                                  _stream()), "attn_fwd4_rect")
        return o[:, :C]
    # reference: sdpa's tril(Sk - Sq) IS the rectangular-causal mask when
    # the chunk sits at the END of the kv prefix
    kv_end = q_offset + C
    o = reference.sdpa(q.float().transpose(1, 2),
                       k[:, :kv_end].float().transpose(1, 2),
                       v[:, :kv_end].float().transpose(1, 2),
                       causal=True, scale=scale).transpose(1, 2)
    return o.to(q.dtype)


def masked_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     kv_len: int, scale: Optional[float] = None
                     ) -> torch.Tensor:
    """Bidirectional (non-causal) attention over only the first `kv_len`
    kv rows — the padded-batch classifier case (BERT serving): rows
    beyond kv_len are padding and must not be attended. Uses the
    rectangular-causal kernel with q_offset = kv_len, which makes every
    query's limit min(row + kv_len, kv_len-1) = kv_len-1 (inference
    only, no autograd) at D == 128; at D == 64 the mask is built into
    kf_attn64_fwd (no K/V repack copies)."""
    B, S, Hq, D = q.shape
    if scale is None:
        scale = D ** -0.5
    if _use_native(q):
        _check_head_dim(D)
    if _use_native(q) and D == 64 and _attn64_enabled():
        with torch.no_grad():
            return _flash_attention64(q, k, v, False, scale, kv_len)
    if _use_native(q) and D == 128:
        lib = _backend.require()
        Hkv = k.shape[2]
        pad = (256 - S % 256) % 256
        if pad:
            q = torch.cat([q, q.new_zeros(B, pad, Hq, D)], dim=1)
        o = torch.empty_like(q)
        lse = torch.empty(B, Hq, q.shape[1], dtype=torch.float32,
                          device=q.device)
        q = q.contiguous()
        # the kernel's kv batch stride is b * Sq_padded rows (training
        # layout) — repack kv into that shape, zeroed past kv_len
        Sp = q.shape[1]
        kp = torch.zeros(B, Sp, Hkv, D, dtype=k.dtype, device=k.device)
        vp = torch.zeros_like(kp)
        kp[:, :kv_len] = k[:, :kv_len]
        vp[:, :kv_len] = v[:, :kv_len]
        _backend.check(
            lib.kf_attn_fwd4_rect(_p(o), _fp(lse), _p(q), _p(kp), _p(vp),
                                  B, Sp, kv_len, Hq, Hkv, D,
                                  0, Hkv * D,
                                  ctypes.c_float(float(scale)), kv_len,
                                  _stream()), "attn_fwd4_rect")
        return o[:, :S]
    o = reference.sdpa(q.float().transpose(1, 2),
                       k[:, :kv_len].float().transpose(1, 2),
                       v[:, :kv_len].float().transpose(1, 2),
                       causal=False, scale=scale).transpose(1, 2)
    return o.to(q.dtype)


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    causal: bool = True, scale: Optional[float] = None,
                    kv_len: Optional[int] = None, seq_lens=None):
    """bshd layout: q [B,S,Hq,D], k/v [B,S,Hkv,D] -> o [B,S,Hq,D].

    kv_len (non-causal only): key/value rows >= kv_len are padding and are
    never attended; their gradients are zero. Works under autograd.

    seq_lens (non-causal only, not together with kv_len): one length per
    batch row, shape [B] — the right-padded batch. Rows >= seq_lens[b] of
    sequence b are padding on both axes: its queries attend keys
    [0, seq_lens[b]), and o and dq/dk/dv rows past the length are exact
    zeros whatever dout holds there. An int32 tensor on q's device is used as
    is, with no host sync and no validation (the kernels clamp each length
    into [1, S]); a CPU tensor or a list is checked (1 <= len <= S) and
    moved. Native at D == 64 (kf_attn64_*_varlen: the work is
    sum_b len_b^2, padded blocks and tiles are skipped, not masked); D == 128
    on the GPU raises. Off the GPU and under KF_ATTN_D64=0 the reference
    math runs per sequence with the same zero-row semantics.

    The CDNA4 kernels tile q in 128-row blocks. D == 128: causal sequences
    are zero-padded to a 128 multiple here (padded key rows are causally
    masked for every real query, so results are exact) and the output is
    sliced back; non-causal input must already satisfy seq_len % 128 == 0
    and kv_len is not supported (see masked_attention). D == 64
    (attention_d64.hip): any seq_len, causal or not — non-causal input is
    zero-padded too and the pad rows are masked through kv_len.
    KF_ATTN_D64=0 sends D == 64 to the torch reference math (bisection).
    """
    D = q.shape[-1]
    if scale is None:
        scale = D ** -0.5
    if kv_len is not None:
        if causal:
            raise ValueError("flash_attention: kv_len is non-causal only")
        kv_len = int(kv_len)
        if not 1 <= kv_len <= k.shape[1]:
            raise ValueError(
                f"kv_len must be in [1, {k.shape[1]}], got {kv_len}")
    if seq_lens is not None:
        if causal:
            raise ValueError("flash_attention: seq_lens is non-causal only")
        if kv_len is not None:
            raise ValueError(
                "flash_attention: pass kv_len or seq_lens, not both")
        seq_lens = _seq_lens_arg(seq_lens, q)
    if _use_native(q):
        _check_head_dim(D)
        if seq_lens is not None:
            if D != 64:
                raise ValueError(
                    "flash_attention: seq_lens needs head_dim 64 on the "
                    "native path; the head_dim 128 kernels have no "
                    "per-sequence mask")
            if _attn64_enabled():
                return _flash_attention64_varlen(q, k, v, scale, seq_lens)
            return _sdpa_ref_varlen(q, k, v, scale, seq_lens)
        if D == 64:
            if _attn64_enabled():
                return _flash_attention64(q, k, v, causal, scale, kv_len)
            return _sdpa_ref(q, k, v, causal, scale, kv_len)
        if kv_len is not None:
            raise ValueError(
                "flash_attention: kv_len needs head_dim 64 on the native "
                "path; for head_dim 128 use masked_attention (inference)")
        S = q.shape[1]
        pad = (128 - S % 128) % 128
        if pad:
            if not causal:
                raise ValueError(
                    "non-causal flash_attention requires seq_len % 128 == 0 "
                    f"(got {S}); pad inputs with an attention mask upstream")
            zq = q.new_zeros(q.shape[0], pad, q.shape[2], q.shape[3])
            zk = k.new_zeros(k.shape[0], pad, k.shape[2], k.shape[3])
            q = torch.cat([q, zq], dim=1)
            k = torch.cat([k, zk], dim=1)
            v = torch.cat([v, zk], dim=1)
            return _FlashAttnHip.apply(q, k, v, causal, scale)[:, :S]
        return _FlashAttnHip.apply(q, k, v, causal, scale)
    if seq_lens is not None:
        return _sdpa_ref_varlen(q, k, v, scale, seq_lens)
    return _sdpa_ref(q, k, v, causal, scale, kv_len)


def _p_off(t: torch.Tensor, elem_off: int) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() + elem_off * t.element_size())


# ------------------------------------------------------------------ SwiGLU --

class _SwigluHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        lib = _backend.require()
        shape = h.shape
        F2 = shape[-1]
        h2 = h.contiguous().view(-1, F2)
        T = h2.shape[0]
        y = torch.empty(T, F2 // 2, dtype=h.dtype, device=h.device)
        _backend.check(lib.kf_swiglu_fwd(_p(y), _p(h2), T, F2 // 2,
                                         _stream()), "swiglu_fwd")
        ctx.save_for_backward(h2)
        ctx.shape = shape
        return y.view(*shape[:-1], F2 // 2)

    @staticmethod
    def backward(ctx, dy):
        lib = _backend.require()
        (h2,) = ctx.saved_tensors
        T, F2 = h2.shape
        dy2 = dy.contiguous().view(T, F2 // 2)
        dh = torch.empty_like(h2)
        _backend.check(lib.kf_swiglu_bwd(_p(dh), _p(dy2), _p(h2), T, F2 // 2,
                                         _stream()), "swiglu_bwd")
        return dh.view(ctx.shape)


def swiglu(h: torch.Tensor) -> torch.Tensor:
    """h = [gate ++ up] on the last dim -> silu(gate) * up."""
    if _use_native(h):
        return _SwigluHip.apply(h)
    g, u = h.chunk(2, dim=-1)
    return torch.nn.functional.silu(g) * u


# -------------------------------------------- Fused QKV -> RoPE -> attention

class _FusedQkvAttentionHip(torch.autograd.Function):
    """RoPE applied IN PLACE on the q/k regions of the fused qkv projection,
    then flash attention reading q/k/v as strided views — zero copies, and
    backward writes dq/dk/dv directly into one dqkv buffer (no torch.cat).

    In-place note: qkv is the wqkv GEMM output; torch.linear's backward
    needs its input and weight, never its output, so rotating the buffer in
    place is safe. No other consumer may read qkv afterwards.
    """

    @staticmethod
    def forward(ctx, qkv, cos, sin, Hq, Hkv, D, causal, scale):
        lib = _backend.require()
        B, S, _ = qkv.shape
        ts = (Hq + 2 * Hkv) * D  # token stride in elements
        qkv = qkv.contiguous()
        _backend.check(
            lib.kf_rope(_p(qkv), _p_off(qkv, Hq * D), _fp(cos), _fp(sin),
                        _ip_or_null(None), B, S, Hq, Hkv, D, ts, ts, 0, 0,
                        _stream()), "rope_fwd")
        o = torch.empty(B, S, Hq * D, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(B, Hq, S, dtype=torch.float32, device=qkv.device)
        _backend.check(
            lib.kf_attn_fwd(_p(o), _fp(lse), _p(qkv), _p_off(qkv, Hq * D),
                            _p_off(qkv, (Hq + Hkv) * D), B, S, Hq, Hkv, D,
                            ts, ts, float(scale), int(causal), _stream()),
            "attn_fwd")
        ctx.save_for_backward(qkv, cos, sin, o, lse)
        ctx.meta = (Hq, Hkv, D, causal, scale)
        return o

    @staticmethod
    def backward(ctx, dout):
        lib = _backend.require()
        qkv, cos, sin, o, lse = ctx.saved_tensors
        Hq, Hkv, D, causal, scale = ctx.meta
        B, S, _ = qkv.shape
        ts = (Hq + 2 * Hkv) * D
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        delta = torch.empty(B, Hq, S, dtype=torch.float32, device=qkv.device)
        # the adjoint of the in-place rotation on the dq/dk regions runs in
        # the backward kernels' store epilogues
        _backend.check(
            lib.kf_attn_bwd_rope(_p(dqkv), _p_off(dqkv, Hq * D),
                                 _p_off(dqkv, (Hq + Hkv) * D), _p(dout),
                                 _p(qkv), _p_off(qkv, Hq * D),
                                 _p_off(qkv, (Hq + Hkv) * D), _p(o),
                                 _fp(lse), _fp(delta), B, S, Hq, Hkv, D,
                                 ts, ts, ts, ts, float(scale), int(causal),
                                 _fp(cos), _fp(sin), 0, _stream()),
            "attn_bwd_rope")
        return dqkv, None, None, None, None, None, None, None


def fused_qkv_attention(qkv: torch.Tensor, cos: torch.Tensor,
                        sin: torch.Tensor, Hq: int, Hkv: int, D: int,
                        causal: bool = True,
                        scale: Optional[float] = None) -> torch.Tensor:
    """qkv [B,S,(Hq+2Hkv)*D] -> attention output [B,S,Hq*D].

    Native path requires S % 128 == 0 (training shapes); otherwise (and on
    CPU) falls back to the composed split->rope->attention ops.
    """
    if scale is None:
        scale = D ** -0.5
    B, S, _ = qkv.shape
    if _use_native(qkv) and S % 128 == 0:
        return _FusedQkvAttentionHip.apply(qkv, cos, sin, Hq, Hkv, D, causal,
                                           scale)
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q = q.reshape(B, S, Hq, D)
    k = k.reshape(B, S, Hkv, D)
    v = v.reshape(B, S, Hkv, D)
    q, k = rope(q, k, cos, sin)
    o = flash_attention(q, k, v, causal=causal, scale=scale)
    return o.reshape(B, S, Hq * D)


# --------------------------------------------------------------- LayerNorm --

class _LayerNormHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = _backend.require()
        shape = x.shape
        x2 = x.contiguous().view(-1, shape[-1])
        rows, cols = x2.shape
        y = torch.empty_like(x2)
        mu = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _backend.check(
            lib.kf_layernorm_fwd(_p(y), _fp(mu), _fp(rstd), _p(x2), _p(weight),
                                 _p(bias), rows, cols, float(eps), _stream()),
            "layernorm_fwd")
        ctx.save_for_backward(x2, weight, mu, rstd)
        ctx.shape = shape
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        lib = _backend.require()
        x2, weight, mu, rstd = ctx.saved_tensors
        rows, cols = x2.shape
        dy2 = dy.contiguous().view(rows, cols)
        dx = torch.empty_like(x2)
        dw = torch.empty_like(weight)
        db = torch.empty_like(weight)
        part = torch.zeros(2 * cols, dtype=torch.float32, device=x2.device)
        _backend.check(
            lib.kf_layernorm_bwd(_p(dx), _p(dw), _p(db), _fp(part), _p(dy2),
                                 _p(x2), _p(weight), _fp(mu), _fp(rstd), rows,
                                 cols, _stream()), "layernorm_bwd")
        return dx.view(ctx.shape), dw, db, None


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float = 1e-5):
    if _use_native(x):
        return _LayerNormHip.apply(x, weight, bias, eps)
    return reference.layer_norm(x, weight, bias, eps)


# --------------------------------------------------------- Decode attention --

def attention_decode(q: torch.Tensor, kcache: torch.Tensor,
                     vcache: torch.Tensor, slots: torch.Tensor,
                     lens: torch.Tensor, scale: Optional[float] = None):
    """Single-token GQA attention over the KV cache (no autograd — serving).

    q [N,Hq,D] bf16; kcache/vcache [SLOTS,SMAX,Hkv,D] bf16;
    slots/lens int32 [N] (checked on the native path: the kernel reads them
    at that width). Returns o [N,Hq,D].
    """
    N, Hq, D = q.shape
    Hkv = kcache.shape[2]
    if scale is None:
        scale = D ** -0.5
    if _use_native(q):
        lib = _backend.require()
        _index_arg("attention_decode", "slots", slots, torch.int32, N, q)
        _index_arg("attention_decode", "lens", lens, torch.int32, N, q)
        q = q.contiguous()
        out = torch.empty_like(q)
        # flash-decoding split: N*Hkv blocks alone underfill the 256-CU
        # chip at serving batch sizes; split the sequence over grid.z and
        # merge partials (one extra tiny kernel). Static per (N, Hkv) so
        # hipGraph capture sees fixed shapes.
        splits = int(os.environ.get("KF_DECODE_SPLITS", "0")) or \
            min(8, max(1, 512 // max(1, N * Hkv)))
        po = pm = None
        if splits > 1:
            po = torch.empty(N, Hq, splits, D, dtype=torch.float32,
                             device=q.device)
            pm = torch.empty(N, Hq, splits, 2, dtype=torch.float32,
                             device=q.device)
        _backend.check(
            lib.kf_attn_decode(_p(out), _p(po), _p(pm), _p(q), _p(kcache),
                               _p(vcache), _i32p(slots), _i32p(lens), N,
                               kcache.shape[1], Hq, Hkv, D, splits,
                               float(scale), _stream()),
            "attn_decode")
        return out
    # reference path: per-sequence sdpa over the cached prefix
    outs = []
    for i in range(N):
        L = int(lens[i])
        s = int(slots[i])
        kk = kcache[s, :L].unsqueeze(0).transpose(1, 2)   # [1,Hkv,L,D]
        vv = vcache[s, :L].unsqueeze(0).transpose(1, 2)
        qq = q[i].view(1, 1, Hq, D).transpose(1, 2)       # [1,Hq,1,D]
        o = reference.sdpa(qq, kk, vv, causal=False, scale=scale)
        outs.append(o.transpose(1, 2).reshape(1, Hq, D))
    return torch.cat(outs)


# --------------------------------------------------------- Cross entropy --

class _CrossEntropyHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index, inplace_ok=False):
        lib = _backend.require()
        T, V = logits.shape
        logits = logits.contiguous()
        loss_sum = torch.zeros(1, dtype=torch.float32, device=logits.device)
        lse = torch.empty(T, dtype=torch.float32, device=logits.device)
        _backend.check(
            lib.kf_ce_fwd(_fp(loss_sum), _fp(lse), _p(logits), _ip(targets),
                          T, V, ignore_index, _stream()), "ce_fwd")
        valid = (targets != ignore_index).sum()
        inv_valid = torch.where(valid > 0, 1.0 / valid.float(),
                                torch.zeros((), device=logits.device))
        ctx.save_for_backward(logits, lse, targets, inv_valid)
        ctx.ignore_index = ignore_index
        ctx.inplace_ok = inplace_ok
        return (loss_sum * inv_valid).squeeze(0)

    @staticmethod
    def backward(ctx, grad_out):
        lib = _backend.require()
        logits, lse, targets, inv_valid = ctx.saved_tensors
        T, V = logits.shape
        scale = (grad_out.float() * inv_valid).contiguous()
        # dlogits is written INTO the saved logits buffer when the caller
        # passed a NON-LEAF (the model path: logits = lm_head(x), whose
        # backward uses x and W, never this output): the kernel is
        # elementwise per position (read lv -> write ov at the same
        # address), and at mb6-7 x seq 4096 x 128256-vocab this buffer is
        # ~7 GB — materializing a second one was the OOM that blocked
        # micro-batch 7. Leaf inputs (user holds the tensor / wants
        # .grad) always get a fresh buffer. KF_CE_INPLACE=0 disables.
        if ctx.inplace_ok and os.environ.get("KF_CE_INPLACE", "1") == "1":
            dlogits = logits
        else:
            dlogits = torch.empty_like(logits)
        _backend.check(
            lib.kf_ce_bwd(_p(dlogits), _p(logits), _fp(lse), _ip(targets),
                          _fp(scale), T, V, ctx.ignore_index, _stream()),
            "ce_bwd")
        return dlogits, None, None, None


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor,
                  ignore_index: int = -100):
    """Mean CE over non-ignored rows. logits [T,V] bf16, targets [T] int64."""
    if _use_native(logits):
        _index_arg("cross_entropy", "targets", targets, torch.int64,
                   logits.shape[0], logits)
        inplace_ok = not logits.is_leaf and logits.is_contiguous()
        return _CrossEntropyHip.apply(logits, targets, ignore_index,
                                      inplace_ok)
    return reference.softmax_cross_entropy(logits, targets, ignore_index)


# ----------------------------------------------------------- Fused AdamW --

WD_GROUP = 64  # elements per wd_groups byte (KF_WD_GROUP in adamw.hip)


def step_tail_enabled() -> bool:
    """KF_STEP_TAIL=0: bisection switch — the trainer's step tail runs as
    torch vector_norm, grad.mul_(scale) and kf_adamw with the fp32 mask
    instead of kf_grad_sumsq and one kf_adamw_clip."""
    return os.environ.get("KF_STEP_TAIL", "1") != "0"


def grad_norm(grad: torch.Tensor) -> torch.Tensor:
    """L2 norm of a flat gradient buffer as a 0-dim fp32 tensor on its
    device, without a host sync. bf16 GPU buffers take kf_grad_sumsq: one
    streaming read, fp32 partial per block, fp64 final sum, no atomics (the
    same buffer gives the same bits)."""
    if (grad.is_cuda and _backend.native_enabled()
            and grad.dtype == torch.bfloat16 and grad.is_contiguous()
            and grad.data_ptr() % 16 == 0):
        lib = _backend.require()
        n = grad.numel()
        out = torch.empty(1, dtype=torch.float32, device=grad.device)
        parts = torch.empty(int(lib.kf_grad_sumsq_nparts(n)),
                            dtype=torch.float32, device=grad.device)
        _backend.check(
            lib.kf_grad_sumsq(_fp(out), _fp(parts), _p(grad), n, _stream()),
            "grad_sumsq")
        return out.view(())
    return torch.linalg.vector_norm(grad, dtype=torch.float32)


def fused_adamw(p16: torch.Tensor, p32: torch.Tensor, grad: torch.Tensor,
                m: torch.Tensor, v: torch.Tensor,
                wd_mask: Optional[torch.Tensor], lr: float, beta1: float,
                beta2: float, eps: float, weight_decay: float, step: int,
                wd_groups: Optional[torch.Tensor] = None,
                gscale: Optional[torch.Tensor] = None):
    """One fused update over a flat bf16 parameter shard + fp32 state.

    p16/grad bf16 [N]; p32/m/v fp32 [N]; wd_mask fp32 {0,1} [N] or None.

    wd_groups: uint8 {0,1} [ceil(N / 64)], one byte per 64 elements, in place
    of wd_mask (FlatParamSpace.build_wd_groups). gscale: 1-element fp32
    tensor holding float(bf16(clip scale)); the gradient is scaled as
    grad.mul_(scale.to(bf16)) would, inside the update, and `grad` holds the
    scaled values afterwards. Either one selects kf_adamw_clip on the GPU.
    """
    if wd_mask is not None and wd_groups is not None:
        raise ValueError("fused_adamw: pass wd_mask or wd_groups, not both")
    if p16.is_cuda and _backend.native_enabled():
        lib = _backend.require()
        if wd_groups is None and gscale is None:
            _backend.check(
                lib.kf_adamw(_p(p16), _fp(p32), _p(grad), _fp(m), _fp(v),
                             _fp(wd_mask), p16.numel(), lr, beta1, beta2, eps,
                             weight_decay, step, _stream()), "adamw")
            return
        n = p16.numel()
        if wd_groups is not None and (
                wd_groups.dtype != torch.uint8
                or wd_groups.numel() * WD_GROUP < n):
            raise ValueError("fused_adamw: wd_groups must be uint8 with one "
                             f"entry per {WD_GROUP} elements")
        if gscale is not None and (gscale.dtype != torch.float32
                                   or gscale.numel() != 1):
            raise ValueError("fused_adamw: gscale must be one fp32 element")
        _backend.check(
            lib.kf_adamw_clip(_p(p16), _fp(p32), _p(grad), _fp(m), _fp(v),
                              _fp(wd_mask), _p(wd_groups), _fp(gscale), n,
                              lr, beta1, beta2, eps, weight_decay, step,
                              _stream()), "adamw_clip")
        return
    # reference path (CPU tests)
    if gscale is not None:
        grad.mul_(gscale.reshape(()).to(grad.dtype))
    if wd_groups is not None:
        wd_mask = wd_groups.float().repeat_interleave(WD_GROUP)[:p16.numel()]
    g32 = grad.float()
    m.mul_(beta1).add_(g32, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g32, g32, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v / bc2).sqrt().add_(eps)
    decay = weight_decay if wd_mask is None else wd_mask * weight_decay
    p32.mul_(1 - lr * decay)
    p32.addcdiv_(m / bc1, denom, value=-lr)
    p16.copy_(p32.to(torch.bfloat16))


# ------------------------------------------------------ Mixture of experts --

MOE_MAX_EXPERTS = 64
MOE_MAX_TOP_K = 8


def _moe_native_enabled() -> bool:
    """KF_MOE_NATIVE=0: bisection switch — MoEMLP runs its per-expert Python
    loop (topk, nonzero, index_add_) instead of the moe.hip path."""
    return os.environ.get("KF_MOE_NATIVE", "1") != "0"


def moe_native_ok(x: torch.Tensor, n_experts: int, top_k: int) -> bool:
    """True if MoEMLP takes the moe.hip path for token rows x [T, h]: a bf16
    GPU tensor, the library loaded, KF_MOE_NATIVE != 0 and the shape within
    the kernels' limits."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and _moe_native_enabled()
            and 2 <= n_experts <= MOE_MAX_EXPERTS
            and 1 <= top_k <= min(n_experts, MOE_MAX_TOP_K)
            and x.shape[-1] % 8 == 0 and _use_native(x))


def _moe_check(t: torch.Tensor, n_experts: int, top_k: int) -> None:
    if not (2 <= n_experts <= MOE_MAX_EXPERTS
            and 1 <= top_k <= min(n_experts, MOE_MAX_TOP_K)):
        raise ValueError(
            f"moe ops support 2 <= n_experts <= {MOE_MAX_EXPERTS} and "
            f"1 <= top_k <= min(n_experts, {MOE_MAX_TOP_K}); got "
            f"n_experts={n_experts}, top_k={top_k}")
    if t.is_cuda and _backend.native_enabled() and t.dtype != torch.bfloat16:
        raise ValueError(f"native moe ops need bf16 inputs, got {t.dtype}")


@dataclasses.dataclass(frozen=True)
class MoeRouting:
    """The routing of one MoE layer, as ops.moe_route returns it.

    topi int32 [T, k] expert of each slot (descending logit, lower index
    first among equals); topw [T, k] gate weights (differentiable w.r.t. the
    logits); probs fp32 [T, k], topw before rounding; pos int32 [T, k] row of
    each (token, slot) pair in the permuted buffer, -1 if its expert is not
    local; src int32 [T * k], src[pos[t, s]] = t (first `rows` entries);
    offsets int32 [n_local + 1] first row of each local expert; splits: host
    list, rows per local expert, or None from moe_route(sync=False), where
    every expert is local and the permuted buffer has all T * k rows."""
    topi: torch.Tensor
    topw: torch.Tensor
    probs: torch.Tensor
    pos: torch.Tensor
    src: torch.Tensor
    offsets: torch.Tensor
    splits: tuple
    e_lo: int
    n_local: int

    @property
    def rows(self) -> int:
        """M: rows of the permuted buffer (pairs routed to a local expert)."""
        if self.splits is None:
            return self.pos.numel()
        return sum(self.splits)


class _MoeRoute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, top_k):
        T, E = logits.shape
        if _use_native(logits):
            lib = _backend.require()
            lg = logits.contiguous()
            topi = torch.empty(T, top_k, dtype=torch.int32,
                               device=logits.device)
            probs = torch.empty(T, top_k, dtype=torch.float32,
                                device=logits.device)
            topw = torch.empty(T, top_k, dtype=logits.dtype,
                               device=logits.device)
            _backend.check(
                lib.kf_moe_route(_p(topi), _fp(probs), _p(topw), _p(lg), T, E,
                                 top_k, _stream()), "moe_route")
        else:
            topi, probs, topw = reference.moe_route(logits, top_k)
            if topw is probs:  # fp32 logits: .to() returned the same tensor
                topw = probs.clone()
        ctx.save_for_backward(probs, topi)
        ctx.n_experts = E
        ctx.mark_non_differentiable(topi, probs)
        return topw, topi, probs

    @staticmethod
    def backward(ctx, dw, _dtopi, _dprobs):
        probs, topi = ctx.saved_tensors
        T, k = topi.shape
        E = ctx.n_experts
        if _use_native(dw):
            lib = _backend.require()
            dw = dw.contiguous()
            dlogits = torch.empty(T, E, dtype=dw.dtype, device=dw.device)
            _backend.check(
                lib.kf_moe_route_bwd(_p(dlogits), _p(dw), _fp(probs),
                                     _p(topi), T, E, k, _stream()),
                "moe_route_bwd")
            return dlogits, None
        return reference.moe_route_bwd(dw, probs, topi, E), None


def _moe_sort(topi: torch.Tensor, e_lo: int, n_local: int):
    T, k = topi.shape
    if not _use_native(topi):
        return reference.moe_sort(topi, e_lo, n_local)
    lib = _backend.require()
    dev = topi.device
    pos = torch.empty(T, k, dtype=torch.int32, device=dev)
    src = torch.empty(T * k, dtype=torch.int32, device=dev)
    offsets = torch.empty(n_local + 1, dtype=torch.int32, device=dev)
    work = torch.empty(int(lib.kf_moe_sort_nwork(T, k, n_local)),
                       dtype=torch.int32, device=dev)
    _backend.check(
        lib.kf_moe_sort(_p(pos), _p(src), _p(offsets), _p(work), _p(topi), T,
                        k, e_lo, n_local, _stream()), "moe_sort")
    return pos, src, offsets


def moe_route(logits: torch.Tensor, top_k: int, e_lo: int = 0,
              n_local: Optional[int] = None, sync: bool = True) -> MoeRouting:
    """Route T tokens: logits [T, E] -> MoeRouting for the local experts
    [e_lo, e_lo + n_local) (default: all E).

    The expert choice is that of a stable descending sort: among equal logits
    the lower expert index wins, whatever the values (NaN, inf, all equal) the
    k experts of a token are distinct and in range. routing.topw is the
    softmax over the k selected logits (fp32 math) and carries the gradient
    back to `logits`. The pairs are sorted by expert with a stable counting
    sort, so the routing is a pure function of the logits.

    `splits` is read from the device with one copy: the only host sync of an
    MoE layer, and what sizes the [M, .] buffers exactly.

    sync=False skips that copy (splits is None), so the call can be captured
    in a graph. It is legal only when the local range is all E experts: then
    M = T * k whatever the logits, and `offsets` stays on the device for
    grouped_skinny_linear."""
    if logits.dim() != 2:
        raise ValueError(f"moe_route: logits must be [T, E], got "
                         f"{tuple(logits.shape)}")
    E = logits.shape[1]
    top_k = int(top_k)
    _moe_check(logits, E, top_k)
    n_local = E - e_lo if n_local is None else int(n_local)
    if not (0 <= e_lo and 1 <= n_local and e_lo + n_local <= E):
        raise ValueError(f"moe_route: local expert range [{e_lo}, "
                         f"{e_lo + n_local}) is not within [0, {E})")
    if not sync and (e_lo != 0 or n_local != E):
        raise ValueError(
            f"moe_route: sync=False needs all {E} experts local (the row "
            f"count is then T * k), got [{e_lo}, {e_lo + n_local})")
    topw, topi, probs = _MoeRoute.apply(logits, top_k)
    pos, src, offsets = _moe_sort(topi, e_lo, n_local)
    if not sync:
        return MoeRouting(topi, topw, probs, pos, src, offsets, None, e_lo,
                          n_local)
    off = offsets.tolist()  # the one device-to-host copy
    splits = tuple(off[i + 1] - off[i] for i in range(n_local))
    return MoeRouting(topi, topw, probs, pos, src, offsets, splits, e_lo,
                      n_local)


class _MoeGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, src, pos, M):
        T, h = x.shape
        ctx.save_for_backward(pos)
        ctx.dims = (T, h, M)
        if _use_native(x):
            lib = _backend.require()
            x = x.contiguous()
            xp = torch.empty(M, h, dtype=x.dtype, device=x.device)
            _backend.check(
                lib.kf_moe_gather(_p(xp), _p(x), _p(src), M, T, h, _stream()),
                "moe_gather")
            return xp
        return reference.moe_gather(x, src, M)

    @staticmethod
    def backward(ctx, dxp):
        (pos,) = ctx.saved_tensors
        T, h, M = ctx.dims
        if _use_native(dxp):
            lib = _backend.require()
            dxp = dxp.contiguous()
            dx = torch.empty(T, h, dtype=dxp.dtype, device=dxp.device)
            _backend.check(
                lib.kf_moe_gather_bwd(_p(dx), _p(dxp), _p(pos), T,
                                      pos.shape[1], h, M, _stream()),
                "moe_gather_bwd")
            return dx, None, None, None
        return reference.moe_gather_bwd(dxp, pos), None, None, None


def _moe_rows_check(t: torch.Tensor, routing: MoeRouting, rows: int,
                    name: str) -> None:
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError(f"{name}: expected [{rows}, h], got "
                         f"{tuple(t.shape)}")
    if _use_native(t) and (t.shape[1] % 8 or t.dtype != torch.bfloat16):
        raise ValueError(f"{name}: the native path needs bf16 rows with "
                         f"h % 8 == 0, got {t.dtype}, h={t.shape[1]}")


def moe_gather(x: torch.Tensor, routing: MoeRouting) -> torch.Tensor:
    """Dispatch: x [T, h] -> xp [M, h], xp[r] = x[routing.src[r]], the rows of
    each local expert contiguous (routing.splits). A bit-exact row copy; its
    backward sums each token's rows in fp32, in slot order, without
    atomics."""
    _moe_rows_check(x, routing, routing.pos.shape[0], "moe_gather")
    return _MoeGather.apply(x, routing.src, routing.pos, routing.rows)


class _MoeCombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, topw, pos):
        M, h = y.shape
        T, k = pos.shape
        if _use_native(y):
            lib = _backend.require()
            y, topw = y.contiguous(), topw.contiguous()
            out = torch.empty(T, h, dtype=y.dtype, device=y.device)
            _backend.check(
                lib.kf_moe_combine(_p(out), _p(y), _p(topw), _p(pos), T, k, h,
                                   M, _stream()), "moe_combine")
        else:
            out = reference.moe_combine(y, topw, pos)
        ctx.save_for_backward(y, topw, pos)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, topw, pos = ctx.saved_tensors
        M, h = y.shape
        T, k = pos.shape
        if _use_native(dout):
            lib = _backend.require()
            dout = dout.contiguous()
            dy = torch.empty_like(y)  # every row < M is written exactly once
            dw = torch.empty_like(topw)
            _backend.check(
                lib.kf_moe_combine_bwd(_p(dy), _p(dw), _p(dout), _p(y),
                                       _p(topw), _p(pos), T, k, h, M,
                                       _stream()), "moe_combine_bwd")
            return dy, dw, None
        dy, dw = reference.moe_combine_bwd(dout, y, topw, pos)
        return dy, dw, None


def moe_combine(y: torch.Tensor, routing: MoeRouting) -> torch.Tensor:
    """Combine: y [M, h] (expert outputs in permuted order) -> out [T, h],
    out[t] = sum_s topw[t, s] * y[pos[t, s]] in fp32, ascending slot order,
    rounded once. A token with no local expert gets zeros. Gradients flow to
    y and to routing.topw; the same inputs give the same bits."""
    _moe_rows_check(y, routing, routing.rows, "moe_combine")
    topw = routing.topw
    if topw.dtype != y.dtype:
        topw = topw.to(y.dtype)
    return _MoeCombine.apply(y, topw, routing.pos)


class _GroupedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xp, w_bank, splits):
        out = torch.empty(xp.shape[0], w_bank.shape[1], dtype=xp.dtype,
                          device=xp.device)
        o = 0
        for e, n in enumerate(splits):
            if n:
                torch.mm(xp[o:o + n], w_bank[e].t(), out=out[o:o + n])
            o += n
        ctx.save_for_backward(xp, w_bank)
        ctx.splits = splits
        return out

    @staticmethod
    def backward(ctx, dout):
        xp, w_bank = ctx.saved_tensors
        dout = dout.contiguous()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dxp = torch.empty_like(xp) if need_x else None
        dw = torch.empty_like(w_bank) if need_w else None
        o = 0
        for e, n in enumerate(ctx.splits):
            if n == 0:
                if need_w:
                    dw[e].zero_()
                continue
            if need_x:
                torch.mm(dout[o:o + n], w_bank[e], out=dxp[o:o + n])
            if need_w:
                torch.mm(dout[o:o + n].t(), xp[o:o + n], out=dw[e])
            o += n
        return dxp, dw, None


def grouped_linear(xp: torch.Tensor, w_bank: torch.Tensor,
                   splits) -> torch.Tensor:
    """Per-expert linear over one permuted buffer: xp [M, in], w_bank
    [n, out, in], splits n row counts summing to M ->
    out[off_e : off_e + n_e] = xp[off_e : off_e + n_e] @ w_bank[e].T, written
    into one preallocated [M, out]. Library GEMMs over contiguous slices; the
    backward loops the same slices (dW[e] is zeros for an empty expert)."""
    splits = tuple(int(n) for n in splits)
    if (xp.dim() != 2 or w_bank.dim() != 3 or len(splits) != w_bank.shape[0]
            or sum(splits) != xp.shape[0] or xp.shape[1] != w_bank.shape[2]):
        raise ValueError(
            f"grouped_linear: xp {tuple(xp.shape)}, w_bank "
            f"{tuple(w_bank.shape)} and splits {splits} do not agree")
    return _GroupedLinear.apply(xp, w_bank, splits)


def moe_experts(x: torch.Tensor, logits: torch.Tensor, w13: torch.Tensor,
                w2: torch.Tensor, top_k: int, e_lo: int = 0) -> torch.Tensor:
    """The routed expert block on token rows: x [T, h], router logits [T, E],
    local expert banks w13 [n, 2f, h] and w2 [n, h, f] for experts
    [e_lo, e_lo + n) -> [T, h]. route, sort, gather, grouped w13 GEMMs, one
    swiglu over the whole [M, 2f] buffer, grouped w2 GEMMs, combine."""
    routing = moe_route(logits, top_k, e_lo, w13.shape[0])
    xp = moe_gather(x, routing)
    a = swiglu(grouped_linear(xp, w13, routing.splits))
    return moe_combine(grouped_linear(a, w2, routing.splits), routing)


# ----------------------------------------------------- Routed MoE decode --

GROUPED_SKINNY_MAX_ROWS = 32


def grouped_skinny_ok(T: int, N: int, K: int, dtype,
                      q8: bool = False) -> bool:
    """True if kf_skinny_gemm_grouped (q8: kf_skinny_gemm_grouped_q8) takes
    T token rows against [., N, K] banks: what a caller asks before it
    captures a graph, since the fallback of grouped_skinny_linear syncs. The
    LDS kernel needs K % 512 == 0 (q8: K % 1024 == 0) and T <= 32, the direct
    bf16 kernel K % 32 == 0 and T <= 16."""
    return (dtype == torch.bfloat16 and N >= 16 and K >= 32
            and _skinny_shape_ok(T, N, K, q8))


def _grouped_skinny(x, w, scale, offsets, max_rows, rows, out, n, N, K):
    """Shared body of the two grouped linears; scale None = bf16 bank."""
    name = "grouped_skinny_linear" + ("" if scale is None else "_q8")
    if (x.dim() != 2 or x.shape[1] != K or offsets.dim() != 1
            or offsets.numel() != n + 1
            or (rows is not None and rows.dim() != 1)):
        raise ValueError(
            f"{name}: x {tuple(x.shape)}, bank [{n}, {N}, {K}], offsets "
            f"{tuple(offsets.shape)} and rows "
            f"{None if rows is None else tuple(rows.shape)} do not agree")
    total = x.shape[0] if rows is None else rows.numel()
    if out is not None and (out.dim() != 2 or out.shape[0] < total
                            or out.shape[1] != N or out.dtype != x.dtype
                            or not out.is_contiguous()):
        raise ValueError(f"{name}: out must be a contiguous [>= {total}, "
                         f"{N}] {x.dtype} tensor, got {tuple(out.shape)}")
    max_rows = int(max_rows)
    native = (_use_native(x) and offsets.dtype == torch.int32
              and (rows is None or rows.dtype == torch.int32)
              and grouped_skinny_ok(max_rows, N, K, x.dtype,
                                    q8=scale is not None))
    if not native:
        wb = w if scale is None else dequantize_fp8_rows(w, scale, x.dtype)
        y = reference.grouped_linear_offsets(x, wb.reshape(n, N, K), offsets,
                                             rows)
        if out is None:
            return y
        out[:total].copy_(y)
        return out
    lib = _backend.require()
    x = x.contiguous()
    offsets = offsets.contiguous()
    if rows is not None:
        rows = rows.contiguous()
    if out is None:
        out = torch.empty(total, N, dtype=x.dtype, device=x.device)
    if scale is None:
        _backend.check(
            lib.kf_skinny_gemm_grouped(
                _p(out), _p(x), _p(w), _i32p(offsets), _i32p(rows), n,
                max_rows, total, x.shape[0], N, K, _stream()),
            "skinny_gemm_grouped")
    else:
        _backend.check(
            lib.kf_skinny_gemm_grouped_q8(
                _p(out), _p(x), _p(w), _fp(scale), _i32p(offsets),
                _i32p(rows), n, max_rows, total, x.shape[0], N, K,
                _stream()),
            "skinny_gemm_grouped_q8")
    return out


def grouped_skinny_linear(x: torch.Tensor, w_bank: torch.Tensor,
                          offsets: torch.Tensor, max_rows: int,
                          rows: Optional[torch.Tensor] = None, *,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-expert decode linear over device offsets: w_bank [n, N, K],
    offsets int32 [n + 1] (MoeRouting.offsets, left on the device) ->
    y [R, N], y[lo_e + i] = x[rows[lo_e + i] if rows is given else lo_e + i]
    @ w_bank[e].T for i < offsets[e + 1] - lo_e. R is rows.numel(), else
    x.shape[0]; rows at or past offsets[n] are not written.

    One launch of kf_skinny_gemm_grouped (skinny_gemm.hip), no host sync, so
    it captures into a graph and the replay follows the offsets of the day.
    An expert without rows reads none of its weights. max_rows bounds the
    rows of one expert (the decode token count T: a token's experts are
    distinct); the kernel clamps to it. `rows` (int32, e.g. MoeRouting.src)
    reads token rows of x in place of a gathered copy. `out`: a contiguous
    [>= R, N] buffer to write rows [0, R) of. Each expert's rows are, bit for
    bit, skinny_linear's for the same rows and w_bank[e].

    Inference only (no autograd). Off the GPU and for shapes
    grouped_skinny_ok rejects, reference.grouped_linear_offsets runs
    instead; that path reads offsets on the host and is not for capture."""
    if w_bank.dim() != 3:
        raise ValueError("grouped_skinny_linear: w_bank must be [n, N, K], "
                         f"got {tuple(w_bank.shape)}")
    n, N, K = w_bank.shape
    if _use_native(x) and (w_bank.dtype != x.dtype
                           or not w_bank.is_contiguous()):
        raise ValueError("grouped_skinny_linear: w_bank must be contiguous "
                         f"and of x's dtype, got {w_bank.dtype}")
    return _grouped_skinny(x, w_bank, None, offsets, max_rows, rows, out, n,
                           N, K)


def grouped_skinny_linear_q8(x: torch.Tensor, w8: torch.Tensor,
                             scale: torch.Tensor, offsets: torch.Tensor,
                             max_rows: int,
                             rows: Optional[torch.Tensor] = None, *,
                             out: Optional[torch.Tensor] = None
                             ) -> torch.Tensor:
    """grouped_skinny_linear on a quantized bank: w8 uint8 [n * N, K] and
    scale fp32 [n * N], quantize_fp8_rows of the bank flattened to rows
    (expert e, column j is row e * N + j); n = offsets.numel() - 1. Each
    expert's rows are skinny_linear_q8's on the bank slice, bit for bit."""
    n = offsets.numel() - 1
    if (w8.dim() != 2 or n < 1 or w8.shape[0] % n or w8.dtype != torch.uint8
            or scale.shape != (w8.shape[0],) or scale.dtype != torch.float32
            or not w8.is_contiguous() or not scale.is_contiguous()):
        raise ValueError(
            f"grouped_skinny_linear_q8: w8 {tuple(w8.shape)} {w8.dtype}, "
            f"scale {tuple(scale.shape)} {scale.dtype} and {n} experts do "
            "not agree")
    return _grouped_skinny(x, w8, scale, offsets, max_rows, rows, out, n,
                           w8.shape[0] // n, w8.shape[1])


@torch.no_grad()
def moe_experts_decode(x: torch.Tensor, logits: torch.Tensor,
                       w13: torch.Tensor, w2: torch.Tensor, top_k: int,
                       q8=None) -> torch.Tensor:
    """moe_experts for the decode step, without a host sync: x [T, h],
    logits [T, E], full banks w13 [E, 2f, h] and w2 [E, h, f] -> [T, h].

    moe_route(sync=False); the grouped w13 GEMM reading x through routing.src
    (no gather launch, no permuted copy of x); one swiglu over [T * k, 2f];
    the grouped w2 GEMM; moe_combine. Every buffer is sized from T, k and the
    weight shapes, so a graph captured on one routing replays any other.
    q8 = ((w13_8, w13_scale), (w2_8, w2_scale)), the banks through
    quantize_fp8_rows on their [E * out, in] views, selects the fp8 kernels.
    Inference only. For capture the caller checks grouped_skinny_ok for both
    banks first."""
    T = x.shape[0]
    routing = moe_route(logits, top_k, 0, w13.shape[0], sync=False)
    if q8 is None:
        h13 = grouped_skinny_linear(x, w13, routing.offsets, T, routing.src)
        y = grouped_skinny_linear(swiglu(h13), w2, routing.offsets, T)
    else:
        (w13_8, s13), (w2_8, s2) = q8
        h13 = grouped_skinny_linear_q8(x, w13_8, s13, routing.offsets, T,
                                       routing.src)
        y = grouped_skinny_linear_q8(swiglu(h13), w2_8, s2, routing.offsets,
                                     T)
    return moe_combine(y, routing)
