"""Parity-test helpers: per-row error metrics, fp32 oracles that return every
output of an op, and a bf16-emulated attention that sets the per-row bound.

Plain torch, CPU only, importable without a GPU. The oracles are thin
autograd wrappers over `ops/reference.py` (the single source of the math);
only `emulated()` spells the attention math out, because it has to round
every intermediate to bf16.

Why a per-row metric: a whole-tensor Frobenius ratio averages a wrong row or
a wrong 32-row sub-tile over the whole tensor, so a dropped store or an
off-by-one mask in one tile passes a 2e-2 bound (see
tests/test_parity_metric_cpu.py). `row_err` is the worst row instead.

Per-row bounds
  * attention (o, dq, dk, dv): 3 x row_err(emulated, oracle) on the case's own
    seeded inputs. `emulated()` holds scores, P, dP, dS and all outputs in
    bf16, which rounds strictly more than the kernels (fp32 accumulators, fp32
    softmax statistics), so a correct kernel sits below 1 x; the factor 3
    covers a different summation order. It is derived from the reference
    alone, never from a kernel's output.
  * mask probe (mask_probe_inputs): the project's fixed 2e-2 (o) / 4e-2 (dv)
    per row against attention_oracle on the probe inputs; a mask off by one
    key moves a row by more than 1.
  * elementwise / row kernels (rope, norms, swiglu, CE grads, adamw p16): the
    op's whole-tensor bound from tests/test_ops_gpu.py, applied per row. A
    correctly bf16-rounded row sits at 2^-9 ~ 0.002, a wrong row near 1.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import reference as R

__all__ = [
    "row_err", "col_err", "rel_err", "attention_inputs", "attention_oracle",
    "emulated", "attention_case", "attention_case_varlen", "AttnCase",
    "attention_case_rect", "mask_probe_inputs", "rope_oracle",
    "rope_store_oracle",
    "rms_norm_oracle", "layer_norm_oracle", "swiglu_oracle",
    "cross_entropy_oracle", "adamw_oracle", "decode_oracle",
    "linear_residual_oracle", "moe_mlp_oracle", "moe_mlp_emulated",
]


# ------------------------------------------------------------------ metrics

def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().cpu()


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """Whole-tensor Frobenius ratio (the metric of tests/test_ops_gpu.py)."""
    got, ref = _f32(got), _f32(ref)
    return ((got - ref).norm() / (ref.norm() + 1e-12)).item()


def row_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max_r ||got_r - ref_r|| / max(||ref_r||, rms), the last dim being the
    row and rms = sqrt(mean_r ||ref_r||^2).

    The rms floor keeps rows that are (near) zero in the oracle from
    dominating: causal dq row 0 is exactly 0 in fp32 and a few bf16 ulps in
    any kernel. NaN anywhere in `got` gives nan (which fails every `<`)."""
    got, ref = _f32(got), _f32(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    got = got.reshape(-1, got.shape[-1])
    ref = ref.reshape(-1, ref.shape[-1])
    rn = ref.norm(dim=1)
    rms = rn.pow(2).mean().sqrt()
    den = torch.maximum(rn, rms).clamp_min(1e-30)
    e = (got - ref).norm(dim=1) / den
    if torch.isnan(e).any():
        return float("nan")
    return e.max().item()


def col_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """row_err over the other axis: every column of the [-1, last] view is one
    "row". For a dW/dB vector [cols] each element is its own row."""
    got, ref = _f32(got), _f32(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return row_err(got.reshape(-1, got.shape[-1]).t(),
                   ref.reshape(-1, ref.shape[-1]).t())


# ---------------------------------------------------------------- attention

def attention_inputs(B: int, S: int, Hq: int, Hkv: int, D: int = 128,
                     seed: int = 1234):
    """Seeded bf16 randn (q, k, v, dout) in bshd, built on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, S, Hq, D, generator=g).bfloat16()
    k = torch.randn(B, S, Hkv, D, generator=g).bfloat16()
    v = torch.randn(B, S, Hkv, D, generator=g).bfloat16()
    dout = torch.randn(B, S, Hq, D, generator=g).bfloat16()
    return q, k, v, dout


def _rope_rows(x, cos, sin, pos_offset, positions):
    """reference.rope_apply with one base position for the batch, or one per
    batch row (`positions`, int64 [B])."""
    if positions is None:
        return R.rope_apply(x, cos, sin, pos_offset)
    return torch.cat([R.rope_apply(x[i:i + 1], cos, sin, int(positions[i]))
                      for i in range(x.shape[0])])


def _lse(q, k, scale, causal):
    """logsumexp of the fp32 scores, [B, Hq, S]; q/k bshd (k already sliced
    and rotated)."""
    g = q.shape[2] // k.shape[2]
    kk = k.float().repeat_interleave(g, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), kk) * scale
    if causal:
        Sq, Sk = s.shape[-2:]
        mask = torch.ones(Sq, Sk, dtype=torch.bool).tril(Sk - Sq)
        s = s.masked_fill(~mask, float("-inf"))
    return torch.logsumexp(s, dim=-1)


def attention_oracle(q, k, v, dout, causal: bool, scale: Optional[float] = None,
                     kv_len: Optional[int] = None, cos=None, sin=None,
                     pos_offset: int = 0, positions=None):
    """fp32 oracle, bshd: (o, lse, dq, dk, dv) by autograd through
    reference.rope_apply (if cos/sin given) and reference.sdpa. k/v are sliced
    to kv_len, so dk/dv rows past it are zero. Gradients are with respect to
    the un-rotated q and k."""
    D = q.shape[-1]
    if scale is None:
        scale = D ** -0.5
    qr, kr, vr = (_f32(t).clone().requires_grad_(True) for t in (q, k, v))
    q2, k2 = qr, kr
    if cos is not None:
        q2 = _rope_rows(qr, cos, sin, pos_offset, positions)
        k2 = _rope_rows(kr, cos, sin, pos_offset, positions)
    v2 = vr
    if kv_len is not None:
        k2, v2 = k2[:, :kv_len], v2[:, :kv_len]
    o = R.sdpa(q2.transpose(1, 2), k2.transpose(1, 2), v2.transpose(1, 2),
               causal=causal, scale=scale).transpose(1, 2)
    o.backward(_f32(dout))
    with torch.no_grad():
        lse = _lse(q2, k2, scale, causal)
    return o.detach(), lse, qr.grad, kr.grad, vr.grad


def _bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 and back: 'held in bf16'."""
    return t.bfloat16().float()


def emulated(q, k, v, dout, causal: bool, scale: Optional[float] = None,
             kv_len: Optional[int] = None, cos=None, sin=None,
             pos_offset: int = 0, positions=None):
    """The same attention, forward and backward, with every intermediate
    rounded to bf16: rotated q/k, scores, P, o, dP, delta, dS, per-head dk/dv
    and all outputs. Returns (o, lse, dq, dk, dv) as fp32 tensors holding
    bf16 values (lse from the bf16 scores, fp32). A correct kernel rounds
    only P, dS and the outputs and accumulates in fp32, so this is an upper
    envelope of honest bf16 error, not a model of any one kernel."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    g = Hq // Hkv
    if scale is None:
        scale = D ** -0.5
    q2, k2 = q.bfloat16(), k.bfloat16()
    if cos is not None:  # rope_apply computes in fp32 and rounds to x.dtype
        q2 = _rope_rows(q2, cos, sin, pos_offset, positions)
        k2 = _rope_rows(k2, cos, sin, pos_offset, positions)
    L = S if kv_len is None else kv_len
    qf = q2.float().transpose(1, 2)                       # [B,Hq,S,D]
    kf = k2.float()[:, :L].transpose(1, 2).repeat_interleave(g, dim=1)
    vf = v.bfloat16().float()[:, :L].transpose(1, 2).repeat_interleave(
        g, dim=1)
    dof = dout.bfloat16().float().transpose(1, 2)
    s = _bf(torch.einsum("bhqd,bhkd->bhqk", qf, kf) * scale)
    if causal:
        mask = torch.ones(S, L, dtype=torch.bool).tril(L - S)
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = _bf(torch.softmax(s, dim=-1))
    o = _bf(torch.einsum("bhqk,bhkd->bhqd", p, vf))
    dp = _bf(torch.einsum("bhqd,bhkd->bhqk", dof, vf))
    delta = _bf((dof * o).sum(dim=-1, keepdim=True))
    ds = _bf(p * (dp - delta))
    dq = _bf(torch.einsum("bhqk,bhkd->bhqd", ds, kf) * scale)
    dk = _bf(torch.einsum("bhqk,bhqd->bhkd", ds, qf) * scale)
    dv = _bf(torch.einsum("bhqk,bhqd->bhkd", p, dof))
    # GQA: the group's per-head bf16 partials are summed, then rounded again
    dk = _bf(dk.view(B, Hkv, g, L, D).sum(dim=2))
    dv = _bf(dv.view(B, Hkv, g, L, D).sum(dim=2))
    dq = dq.transpose(1, 2)
    dk_full = torch.zeros(B, S, Hkv, D)
    dv_full = torch.zeros(B, S, Hkv, D)
    dk_full[:, :L] = dk.transpose(1, 2)
    dv_full[:, :L] = dv.transpose(1, 2)
    if cos is not None:
        # adjoint of the rotation = rotation by -angle, on the bf16 grads
        dq = _rope_rows(dq.bfloat16(), cos, -sin, pos_offset,
                        positions).float()
        dk_full = _rope_rows(dk_full.bfloat16(), cos, -sin, pos_offset,
                             positions).float()
    return o.transpose(1, 2).contiguous(), lse, dq.contiguous(), dk_full, \
        dv_full


class AttnCase(NamedTuple):
    inputs: Tuple[torch.Tensor, ...]   # q, k, v, dout (bf16, CPU, un-rotated)
    oracle: Dict[str, torch.Tensor]    # o, lse, dq, dk, dv (fp32)
    emu_err: Dict[str, float]          # row_err(emulated, oracle) per output
    bound: Dict[str, float]            # 3 x emu_err


_ATTN_CACHE: Dict[tuple, AttnCase] = {}
ROW_BOUND_FACTOR = 3.0
_OUTS = ("o", "lse", "dq", "dk", "dv")


def attention_case(B: int, S: int, Hq: int, Hkv: int, causal: bool,
                   D: int = 128, seed: int = 1234,
                   kv_len: Optional[int] = None, rope_len: Optional[int] = None,
                   pos_offset: int = 0,
                   positions: Optional[Tuple[int, ...]] = None) -> AttnCase:
    """Inputs, fp32 oracle and per-row bounds of one attention case, computed
    once per argument tuple. rope_len: length of the cos/sin table (None = no
    RoPE); `positions` a tuple of per-batch base positions."""
    key = (B, S, Hq, Hkv, causal, D, seed, kv_len, rope_len, pos_offset,
           positions)
    if key in _ATTN_CACHE:
        return _ATTN_CACHE[key]
    inputs = attention_inputs(B, S, Hq, Hkv, D, seed)
    kw = dict(kv_len=kv_len)
    if rope_len is not None:
        cos, sin = R.rope_cos_sin(rope_len, D)
        kw.update(cos=cos, sin=sin, pos_offset=pos_offset,
                  positions=None if positions is None
                  else torch.tensor(positions))
    oracle = dict(zip(_OUTS, attention_oracle(*inputs, causal, **kw)))
    emu = dict(zip(_OUTS, emulated(*inputs, causal, **kw)))
    emu_err = {n: row_err(emu[n], oracle[n]) for n in ("o", "dq", "dk", "dv")}
    bound = {n: ROW_BOUND_FACTOR * e for n, e in emu_err.items()}
    _ATTN_CACHE[key] = AttnCase(inputs, oracle, emu_err, bound)
    return _ATTN_CACHE[key]


def _embed_varlen(fn, inputs, seq_lens):
    """Run fn (attention_oracle / emulated, non-causal) on each sequence's
    [b:b+1, :L] slices and embed (o, lse, dq, dk, dv) into zero tensors of
    the full shape: rows past a length are zero in every output."""
    q, k, v, dout = inputs
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    out = {"o": torch.zeros(B, S, Hq, D), "lse": torch.zeros(B, Hq, S),
           "dq": torch.zeros(B, S, Hq, D), "dk": torch.zeros(B, S, Hkv, D),
           "dv": torch.zeros(B, S, Hkv, D)}
    for b, L in enumerate(seq_lens):
        o, lse, dq, dk, dv = fn(q[b:b + 1, :L], k[b:b + 1, :L],
                                v[b:b + 1, :L], dout[b:b + 1, :L], False)
        out["o"][b, :L], out["lse"][b, :, :L] = o[0], lse[0]
        out["dq"][b, :L], out["dk"][b, :L], out["dv"][b, :L] = \
            dq[0], dk[0], dv[0]
    return out


def attention_case_varlen(B: int, S: int, Hq: int, Hkv: int,
                          seq_lens: Tuple[int, ...], D: int = 64,
                          seed: int = 1234) -> AttnCase:
    """attention_case for a right-padded batch with one length per sequence
    (non-causal): sequence b attends within its first seq_lens[b] rows, and
    o, dq, dk, dv are zero past them (lse is left 0 there). Inputs are the
    plain seeded ones; a test may overwrite k/v rows past a length, which the
    oracle never reads. emu_err / bound come from row_err over the whole
    embedded tensors, not per sequence: a length-1 sequence has no emulation
    error at all and would give a zero bound."""
    seq_lens = tuple(int(L) for L in seq_lens)
    assert len(seq_lens) == B and all(1 <= L <= S for L in seq_lens), seq_lens
    key = ("varlen", B, S, Hq, Hkv, seq_lens, D, seed)
    if key in _ATTN_CACHE:
        return _ATTN_CACHE[key]
    inputs = attention_inputs(B, S, Hq, Hkv, D, seed)
    oracle = _embed_varlen(attention_oracle, inputs, seq_lens)
    emu = _embed_varlen(emulated, inputs, seq_lens)
    emu_err = {n: row_err(emu[n], oracle[n]) for n in ("o", "dq", "dk", "dv")}
    bound = {n: ROW_BOUND_FACTOR * e for n, e in emu_err.items()}
    _ATTN_CACHE[key] = AttnCase(inputs, oracle, emu_err, bound)
    return _ATTN_CACHE[key]


def attention_case_rect(B: int, C: int, Skv: int, q_offset: int, Hq: int,
                        Hkv: int, seed: int = 1234, D: int = 128) -> AttnCase:
    """attention_case for rectangular-causal attention (chunked prefill): C
    query rows at global offset q_offset over Skv >= q_offset + C kv rows,
    row i attending keys <= q_offset + i. inputs = (q [B,C,Hq,D],
    k, v [B,Skv,Hkv,D]); oracle, emu_err and bound hold "o" (and the oracle
    "lse" [B,Hq,C]) only: there is no backward.

    The oracle is rows [q_offset, q_offset + C) of the square causal
    attention over n = q_offset + C rows: q is embedded into a zero tensor of
    n rows, k/v are sliced to n (keys past n are visible to no row), dout is
    zero. The bound is ROW_BOUND_FACTOR x row_err(emulated, oracle) over the
    C rows, from the reference alone, and must exceed 2^-9 (one bf16 ulp of
    relative error): a case with a single visible key has no emulation error
    and is checked by equality instead."""
    assert Skv >= q_offset + C and C >= 1 and q_offset >= 0, \
        (C, Skv, q_offset)
    key = ("rect", B, C, Skv, q_offset, Hq, Hkv, D, seed)
    if key in _ATTN_CACHE:
        return _ATTN_CACHE[key]
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, C, Hq, D, generator=g).bfloat16()
    k = torch.randn(B, Skv, Hkv, D, generator=g).bfloat16()
    v = torch.randn(B, Skv, Hkv, D, generator=g).bfloat16()
    n = q_offset + C
    qn = torch.zeros(B, n, Hq, D, dtype=q.dtype)
    qn[:, q_offset:] = q
    dout = torch.zeros(B, n, Hq, D)
    o, lse = attention_oracle(qn, k[:, :n], v[:, :n], dout, True)[:2]
    eo = emulated(qn, k[:, :n], v[:, :n], dout, True)[0]
    oracle = {"o": o[:, q_offset:].contiguous(),
              "lse": lse[:, :, q_offset:].contiguous()}
    emu_err = {"o": row_err(eo[:, q_offset:], oracle["o"])}
    bound = {"o": ROW_BOUND_FACTOR * emu_err["o"]}
    assert bound["o"] > 2.0 ** -9, (key, bound)
    _ATTN_CACHE[key] = AttnCase((q, k, v), oracle, emu_err, bound)
    return _ATTN_CACHE[key]


def mask_probe_inputs(B: int, Sq: int, Skv: int, Hq: int, Hkv: int,
                      D: int = 128, seed: int = 1234):
    """(q [B,Sq,Hq,D], k, v [B,Skv,Hkv,D], scale): bf16 inputs that pin the
    mask boundary of every single row. The score of key j is 8 * j for every
    query, so each query puts all its weight but e^-8 on its LAST visible
    key: its output row is that key's v row, and dv[j] is the sum over the
    GQA group of the dout rows whose last visible key is j. A mask that is
    off by one key for one row moves that row to another v row.

    Construction: q and k are seeded randn x 0.1; then q[..., 0] = q[..., 1]
    = 8, k[:, j, :, 0] = 256 * (j // 32), k[:, j, :, 1] = 8 * (j % 32) and
    scale = 0.125, all exact in bf16 (j < 2^13), so dims 0 and 1 contribute
    exactly 0.125 * (2048 * (j // 32) + 64 * (j % 32)) = 8 * j. The other
    D - 2 dims add 0.125 * sum of D - 2 products of two N(0, 0.01) values:
    std 0.014 at D = 128, under 0.25 in every case used (18 sigma), against
    a gap of 8 between neighbouring keys. v is seeded randn.

    Margins, measured from the reference alone (seed 7, Hq, Hkv = 2, 1) at
    D = 128 rect (C, Skv, off) = (300, 1115, 815), (256, 256, 0),
    (100, 133, 33) and at D = 64 square S = 200, with row_err against
    attention_oracle on the probe inputs; the fixed per-row bounds are 2e-2
    (o) and 4e-2 (dv):
      row_err(oracle o, v[limit])             <= 5.9e-4
      mask shifted by one key either way      >= 1.54
      one wrong row among 100 .. 300          >= 1.23
      dv vs group-summed dout                 <= 6.6e-4; shifted a row >= 1.58
    (tests/test_attn_probe_cpu.py prints them and asserts a factor 10 below
    the bounds and 1.0 above).

    Not for emulated(): it rounds the scores to bf16, which destroys their
    order at this magnitude (row_err 0.98). dq and dk are pure cancellation
    here (rms ~3e-3 against k entries in the thousands) and lse sits near
    8 * Skv, where an absolute 1e-2 means nothing: check o and dv only."""
    assert Skv <= 8192, Skv   # 256 * (j // 32) stays exact in bf16
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, generator=g) * 0.1
    k = torch.randn(B, Skv, Hkv, D, generator=g) * 0.1
    v = torch.randn(B, Skv, Hkv, D, generator=g).bfloat16()
    j = torch.arange(Skv)
    q[..., 0] = 8.0
    q[..., 1] = 8.0
    k[..., 0] = (256 * (j // 32)).float().view(1, Skv, 1)
    k[..., 1] = (8 * (j % 32)).float().view(1, Skv, 1)
    return q.bfloat16(), k.bfloat16(), v, 0.125


# ------------------------------------------------- row / elementwise oracles

def rope_oracle(q, k, cos, sin, pos_offset: int = 0, positions=None,
                dq2=None, dk2=None):
    """(q2, k2[, dq, dk]): reference.rope_apply in fp32, per batch row when
    `positions` is given; with upstream grads dq2/dk2 also the input grads."""
    qr, kr = (_f32(t).clone().requires_grad_(True) for t in (q, k))
    q2 = _rope_rows(qr, cos, sin, pos_offset, positions)
    k2 = _rope_rows(kr, cos, sin, pos_offset, positions)
    if dq2 is None:
        return q2.detach(), k2.detach()
    gq, gk = torch.autograd.grad(
        (q2 * _f32(dq2)).sum() + (k2 * _f32(dk2)).sum(), [qr, kr])
    return q2.detach(), k2.detach(), gq, gk


def rope_store_oracle(qkv, cos, sin, positions, Hq: int, Hkv: int,
                      D: int = 128):
    """fp32 (q_rot [N,Hq,D], k_rot [N,Hkv,D], v [N,Hkv,D]) of one decode
    step's fused projection qkv [N, ..., (Hq + 2 Hkv) * D]: q and k rotated
    at positions[i] (reference.rope_apply), v as is. What decode_rope_store
    returns (q) and writes to cache rows [slot[i], positions[i]] (k, v)."""
    n = qkv.shape[0]
    qq, kk, vv = _f32(qkv).reshape(n, -1).split(
        [Hq * D, Hkv * D, Hkv * D], dim=-1)
    pos = torch.as_tensor(positions).detach().cpu().long()
    q2 = _rope_rows(qq.reshape(n, 1, Hq, D), cos, sin, 0, pos)
    k2 = _rope_rows(kk.reshape(n, 1, Hkv, D), cos, sin, 0, pos)
    return (q2.reshape(n, Hq, D), k2.reshape(n, Hkv, D),
            vv.reshape(n, Hkv, D).clone())


def rms_norm_oracle(x, w, dy, eps: float = 1e-5):
    """(y, dx, dw) of reference.rms_norm in fp32."""
    xr, wr = (_f32(t).clone().requires_grad_(True) for t in (x, w))
    y = R.rms_norm(xr, wr, eps)
    y.backward(_f32(dy))
    return y.detach(), xr.grad, wr.grad


def layer_norm_oracle(x, w, b, dy, eps: float = 1e-5):
    """(y, dx, dw, db) of reference.layer_norm in fp32."""
    xr, wr, br = (_f32(t).clone().requires_grad_(True) for t in (x, w, b))
    y = R.layer_norm(xr, wr, br, eps)
    y.backward(_f32(dy))
    return y.detach(), xr.grad, wr.grad, br.grad


def swiglu_oracle(h, dy):
    """(y, dh) of silu(gate) * up, h = [gate ++ up], in fp32."""
    hr = _f32(h).clone().requires_grad_(True)
    g, u = hr.chunk(2, dim=-1)
    y = torch.nn.functional.silu(g) * u
    y.backward(_f32(dy))
    return y.detach(), hr.grad


def cross_entropy_oracle(logits, targets, ignore_index: int = -100,
                         grad_out: float = 1.0):
    """(loss, dlogits) of reference.softmax_cross_entropy in fp32, with the
    ops wrapper's all-ignored semantics: loss 0 and zero grad (inv_valid = 0),
    not F.cross_entropy's NaN."""
    lr = _f32(logits).clone().requires_grad_(True)
    tg = targets.detach().cpu()
    if not bool((tg != ignore_index).any()):
        return torch.zeros(()), torch.zeros_like(lr)
    loss = R.softmax_cross_entropy(lr, tg, ignore_index)
    loss.backward(torch.tensor(float(grad_out)))
    return loss.detach(), lr.grad


def adamw_oracle(p32, grads, wd_mask, lr, beta1, beta2, eps, weight_decay):
    """(p32, m, v) after len(grads) steps of reference.adamw_step from zero
    moments. A {0,1} wd_mask selects, per element, between a run with the
    decay and a run without it (the update is elementwise and m, v do not
    depend on the decay)."""
    def run(wd):
        p = _f32(p32).clone()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step, g in enumerate(grads, 1):
            R.adamw_step(p, _f32(g), m, v, lr, beta1, beta2, eps, wd, step)
        return p, m, v
    p, m, v = run(weight_decay)
    if wd_mask is not None:
        p0, _, _ = run(0.0)
        p = torch.where(_f32(wd_mask) != 0, p, p0)
    return p, m, v


def decode_oracle(q, kcache, vcache, slots, lens, scale=None):
    """[N, Hq, D] fp32: per-sequence reference.sdpa over the cached prefix;
    a sequence with len == 0 attends nothing and gives a zero row."""
    N, Hq, D = q.shape
    if scale is None:
        scale = D ** -0.5
    out = torch.zeros(N, Hq, D)
    for i in range(N):
        L, s = int(lens[i]), int(slots[i])
        if L == 0:
            continue
        o = R.sdpa(_f32(q[i]).view(1, 1, Hq, D).transpose(1, 2),
                   _f32(kcache[s, :L]).unsqueeze(0).transpose(1, 2),
                   _f32(vcache[s, :L]).unsqueeze(0).transpose(1, 2),
                   causal=False, scale=scale)
        out[i] = o.transpose(1, 2).reshape(Hq, D)
    return out


def linear_residual_oracle(x, w, residual=None):
    """fp32 x @ w^T (+ residual)."""
    y = torch.nn.functional.linear(_f32(x), _f32(w))
    return y if residual is None else y + _f32(residual)


# ------------------------------------------------------- mixture of experts

class _RoundBf16(torch.autograd.Function):
    """'Held in bf16' in both directions: the value and its gradient."""

    @staticmethod
    def forward(ctx, t):
        return _bf(t)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def _moe_block(x, gate_w, w13, w2, topi, dout, e_lo, rnd):
    """One MoE block with the routing given: topi [T, k] picks the experts,
    everything else (the logits, the gate weights as the softmax over the
    selected logits, the experts, the weighted sum in slot order) is computed
    here. `rnd` is applied where the bf16 model path holds a tensor in bf16.
    Returns out, dx, dgate, dw13, dw2 (fp32)."""
    xr, gr, w13r, w2r = (_f32(t).clone().requires_grad_(True)
                         for t in (x, gate_w, w13, w2))
    topi = topi.detach().cpu().long()
    T, k = topi.shape
    # x feeds the router and the experts; the two gradients are held in bf16
    # before autograd adds them
    logits = rnd(rnd(xr) @ gr.t())
    topw = rnd(torch.softmax(logits.gather(1, topi), dim=-1))
    xe = rnd(xr)
    out = torch.zeros(T, xr.shape[1])
    for s in range(k):
        ys = torch.zeros(T, xr.shape[1])
        for el in range(w13r.shape[0]):
            sel = (topi[:, s] == e_lo + el).nonzero(as_tuple=True)[0]
            if sel.numel() == 0:
                continue
            h13 = rnd(xe[sel] @ w13r[el].t())
            g, u = h13.chunk(2, dim=-1)
            a = rnd(torch.nn.functional.silu(g) * u)
            ys = ys.index_copy(0, sel, rnd(a @ w2r[el].t()))
        out = out + topw[:, s:s + 1] * ys
    out = rnd(out)
    out.backward(_f32(dout))
    return (out.detach(), rnd(xr.grad), rnd(gr.grad), rnd(w13r.grad),
            rnd(w2r.grad))


def moe_mlp_oracle(x, gate_w, w13, w2, topi, dout, e_lo: int = 0):
    """(out, dx, dgate, dw13, dw2) of one MoE block in fp32, routing given:
    x [T, h], gate_w [E, h], w13 [n, 2f, h], w2 [n, h, f] the banks of
    experts [e_lo, e_lo + n), topi [T, k]. The gate weights are the softmax
    over the k selected logits, so dx and dgate include the router path."""
    return _moe_block(x, gate_w, w13, w2, topi, dout, e_lo, lambda t: t)


def moe_mlp_emulated(x, gate_w, w13, w2, topi, dout, e_lo: int = 0):
    """moe_mlp_oracle's math with a bf16 round (of the value and of its
    gradient) after every GEMM, after the softmax, after swiglu and after the
    weighted sum, and of every returned gradient. The kernels round at the
    same places but accumulate in fp32 between them and compute swiglu and
    the softmax from unrounded fp32 intermediates, so this rounds strictly
    more: the envelope that sets the per-row bound."""
    return _moe_block(x, gate_w, w13, w2, topi, dout, e_lo,
                      _RoundBf16.apply)
