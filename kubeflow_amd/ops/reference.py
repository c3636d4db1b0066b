"""Pure-PyTorch reference implementations of the hot ops.

These are the numerics oracle for the HIP kernels (tests compare the CDNA4
kernels against these run in fp32) and the CPU fallback used when no GPU is
present (unit tests in CI run on CPU). On a GPU box the HIP kernels are the
only path — `kubeflow_amd.ops` refuses to fall back silently there.

Reference behavior anchor: the worker hot loop of a Kubeflow PyTorchJob /
InferenceService (BASELINE.json north_star; the reference repo itself contains
no kernels — SURVEY.md §2.13).
"""
from __future__ import annotations

import torch


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """y = x * rsqrt(mean(x^2, dim=-1) + eps) * weight, computed in fp32."""
    dt = x.dtype
    x32 = x.float()
    var = x32.pow(2).mean(dim=-1, keepdim=True)
    y = x32 * torch.rsqrt(var + eps)
    return (y * weight.float()).to(dt)


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    dt = x.dtype
    x32 = x.float()
    mu = x32.mean(dim=-1, keepdim=True)
    var = x32.var(dim=-1, unbiased=False, keepdim=True)
    y = (x32 - mu) * torch.rsqrt(var + eps)
    return (y * weight.float() + bias.float()).to(dt)


def rope_cos_sin(seq_len: int, head_dim: int, theta: float = 500000.0,
                 device=None, dtype=torch.float32):
    """Precomputed rotary tables (host-side per CDNA guide: no device trig).

    Returns cos, sin of shape [seq_len, head_dim//2] in fp32.
    """
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, device=device,
                                             dtype=torch.float32) / head_dim))
    t = torch.arange(seq_len, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)  # [S, D/2]
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def rope_apply(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
               pos_offset: int = 0) -> torch.Tensor:
    """Apply rotary embedding. x: [B, S, H, D]; cos/sin: [>=S, D/2] fp32.

    Pairing is (x[..., :D/2], x[..., D/2:]) — the "rotate_half" convention
    used by Llama-family models.
    """
    B, S, H, D = x.shape
    c = cos[pos_offset:pos_offset + S].view(1, S, 1, D // 2).float()
    s = sin[pos_offset:pos_offset + S].view(1, S, 1, D // 2).float()
    x32 = x.float()
    x1, x2 = x32[..., : D // 2], x32[..., D // 2:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    return out.to(x.dtype)


def sdpa(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
         causal: bool = True, scale: float | None = None) -> torch.Tensor:
    """Reference attention (materializes S×S — oracle only, fp32 math).

    q: [B, Hq, S, D]; k, v: [B, Hkv, S, D] (GQA: Hq % Hkv == 0).
    """
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    if scale is None:
        scale = D ** -0.5
    g = Hq // Hkv
    k = k.repeat_interleave(g, dim=1)
    v = v.repeat_interleave(g, dim=1)
    scores = torch.einsum("bhqd,bhkd->bhqk", q.float(), k.float()) * scale
    if causal:
        Sk = k.shape[2]
        mask = torch.ones(S, Sk, dtype=torch.bool, device=q.device).tril(Sk - S)
        scores = scores.masked_fill(~mask, float("-inf"))
    p = torch.softmax(scores, dim=-1)
    out = torch.einsum("bhqk,bhkd->bhqd", p, v.float())
    return out.to(q.dtype)


def softmax_cross_entropy(logits: torch.Tensor, targets: torch.Tensor,
                          ignore_index: int = -100):
    """Mean CE over non-ignored targets, fp32 math. logits [T, V], targets [T]."""
    return torch.nn.functional.cross_entropy(
        logits.float(), targets, ignore_index=ignore_index)


def adamw_step(p32: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
               v: torch.Tensor, lr: float, beta1: float, beta2: float,
               eps: float, weight_decay: float, step: int):
    """Decoupled AdamW on fp32 master weights (in-place); returns nothing.

    Matches torch.optim.AdamW semantics with bias correction.
    """
    g32 = g.float()
    m.mul_(beta1).add_(g32, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g32, g32, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v / bc2).sqrt_().add_(eps)
    p32.mul_(1 - lr * weight_decay)
    p32.addcdiv_(m / bc1, denom, value=-lr)


# ---------------------------------------------------- mixture of experts --
#
# The semantics of csrc/moe.hip in plain torch: the CPU path of the public
# ops and the oracle of the GPU tests. T tokens, E experts, k = top_k; the
# local expert range is [e_lo, e_lo + n_local) and M pairs (token, slot) are
# routed into it. Every sum over a token's slots is an fp32 loop in ascending
# slot order starting from 0, skipping slots whose expert is not local, so
# that the kernels can be compared bit for bit.

def moe_route(logits: torch.Tensor, top_k: int):
    """logits [T, E] -> (topi int32 [T, k], probs fp32 [T, k], topw [T, k] in
    logits.dtype). Slots by descending logit; among equal logits the lower
    expert index first (a stable descending sort, NaN sorting first as in
    torch.sort). probs is the fp32 softmax over the k selected logits."""
    vals, idx = torch.sort(logits, dim=-1, descending=True, stable=True)
    probs = torch.softmax(vals[:, :top_k].float(), dim=-1)
    return idx[:, :top_k].to(torch.int32), probs, probs.to(logits.dtype)


def moe_route_bwd(dw: torch.Tensor, probs: torch.Tensor, topi: torch.Tensor,
                  n_experts: int) -> torch.Tensor:
    """dlogits [T, E] in dw.dtype: p_i * (dw_i - sum_j p_j dw_j) at column
    topi[t, i], exact zeros elsewhere."""
    d = dw.float()
    g = probs * (d - (probs * d).sum(dim=-1, keepdim=True))
    out = torch.zeros(dw.shape[0], n_experts, dtype=torch.float32,
                      device=dw.device)
    out.scatter_(1, topi.long(), g)
    return out.to(dw.dtype)


def moe_sort(topi: torch.Tensor, e_lo: int, n_local: int):
    """Stable counting sort of the (token, slot) pairs by expert ->
    (pos int32 [T, k], src int32 [T * k], offsets int32 [n_local + 1]).
    pos[t, s] is the pair's row in the permuted buffer (-1: expert not
    local), src[pos[t, s]] = t, offsets[el] the first row of local expert el
    and offsets[n_local] = M. Only src[:M] is defined."""
    T, k = topi.shape
    flat = topi.reshape(-1).long() - e_lo
    local = (flat >= 0) & (flat < n_local)
    key = torch.where(local, flat, torch.full_like(flat, n_local))
    order = torch.argsort(key, stable=True)
    pos = torch.empty(T * k, dtype=torch.int64, device=topi.device)
    pos[order] = torch.arange(T * k, device=topi.device)
    pos[~local] = -1
    src = torch.zeros(T * k, dtype=torch.int32, device=topi.device)
    m = int(local.sum())
    src[:m] = (order[:m] // k).to(torch.int32)
    counts = torch.bincount(key[local], minlength=n_local)[:n_local]
    offsets = torch.zeros(n_local + 1, dtype=torch.int64, device=topi.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return (pos.view(T, k).to(torch.int32), src, offsets.to(torch.int32))


def moe_gather(x: torch.Tensor, src: torch.Tensor, m: int) -> torch.Tensor:
    """xp[r] = x[src[r]], r < m."""
    return x[src[:m].long()]


def _moe_slot_sum(rows: torch.Tensor, pos: torch.Tensor, w, dtype):
    T, k = pos.shape
    acc = torch.zeros(T, rows.shape[1], dtype=torch.float32,
                      device=rows.device)
    if rows.shape[0] == 0:
        return acc.to(dtype)
    for s in range(k):
        p = pos[:, s].long()
        term = rows[p.clamp_min(0)].float()
        if w is not None:
            term = w[:, s:s + 1].float() * term
        acc = torch.where((p >= 0).unsqueeze(1), acc + term, acc)
    return acc.to(dtype)


def moe_gather_bwd(dxp: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """dx[t] = sum_s dxp[pos[t, s]] (fp32, slot order), in dxp.dtype."""
    return _moe_slot_sum(dxp, pos, None, dxp.dtype)


def moe_combine(y: torch.Tensor, topw: torch.Tensor,
                pos: torch.Tensor) -> torch.Tensor:
    """out[t] = sum_s topw[t, s] * y[pos[t, s]] (fp32, slot order), in
    y.dtype."""
    return _moe_slot_sum(y, pos, topw, y.dtype)


def moe_combine_bwd(dout: torch.Tensor, y: torch.Tensor, topw: torch.Tensor,
                    pos: torch.Tensor):
    """(dy [M, h], dw [T, k]): dy[pos[t, s]] = topw[t, s] * dout[t] and
    dw[t, s] = <dout[t], y[pos[t, s]]> in fp32, 0 for a slot that is not
    local; both rounded to y.dtype."""
    T, k = pos.shape
    dy = torch.zeros_like(y)
    dw = torch.zeros(T, k, dtype=torch.float32, device=y.device)
    d32 = dout.float()
    for s in range(k):
        p = pos[:, s].long()
        sel = (p >= 0).nonzero(as_tuple=True)[0]
        if sel.numel() == 0:
            continue
        dy[p[sel]] = (topw[sel, s:s + 1].float() * d32[sel]).to(y.dtype)
        dw[sel, s] = (d32[sel] * y[p[sel]].float()).sum(dim=-1)
    return dy, dw.to(topw.dtype)


def grouped_linear_offsets(x: torch.Tensor, w_bank: torch.Tensor,
                           offsets: torch.Tensor, rows=None) -> torch.Tensor:
    """The reference of ops.grouped_skinny_linear: w_bank [n, N, K], offsets
    [n + 1] as a tensor (read on the host here: not a capture path) ->
    y [R, N], y[lo_e + i] = x[rows[lo_e + i] if rows is given else lo_e + i]
    @ w_bank[e].T, R = rows.numel() or x.shape[0]. Rows no expert owns are
    zeros. One torch.mm per expert that has rows, over the same slices as
    ops.grouped_linear, so the two agree bit for bit on the CPU."""
    n, N, _ = w_bank.shape
    total = x.shape[0] if rows is None else rows.numel()
    y = torch.zeros(total, N, dtype=x.dtype, device=x.device)
    off = offsets.tolist()
    for e in range(n):
        lo, hi = off[e], off[e + 1]
        if hi <= lo:
            continue
        xs = x[lo:hi] if rows is None else x[rows[lo:hi].long()]
        torch.mm(xs, w_bank[e].t(), out=y[lo:hi])
    return y
