"""MoE routing, dispatch and combine without a GPU: the plain-torch semantics
in ops/reference.py (the CPU path of ops.moe_* and the oracle of
tests/test_moe_gpu.py) and the functional block against MoEMLP's per-expert
loop."""
import dataclasses

import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.models import llama
from kubeflow_amd.ops import reference as R

INF = float("inf")
NAN = float("nan")

# [4, 8] router logits, top_k = 2:
#   row 0  all equal                      -> the two lowest indices
#   row 1  rank 2 ties with rank 3        -> the lower index takes the slot
#   row 2  one finite value, the rest -inf -> slot 1 is the first -inf
#   row 3  one NaN                        -> only distinct and in range
ROUTE_TABLE = torch.tensor([
    [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
    [0.0, 3.0, 1.0, 2.0, 2.0, 0.0, 0.0, 0.0],
    [-INF, -INF, -INF, -INF, -INF, 2.0, -INF, -INF],
    [0.1, NAN, 0.3, -0.2, 0.0, 0.5, 0.4, -1.0],
])
ROUTE_EXPECT = torch.tensor([[0, 1], [1, 3], [5, 0]], dtype=torch.int32)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _distinct_in_range(row, E):
    vals = row.tolist()
    return len(set(vals)) == len(vals) and all(0 <= v < E for v in vals)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_route_reference_table(dtype):
    logits = ROUTE_TABLE.to(dtype)
    topi, probs, topw = R.moe_route(logits, 2)
    assert topi.dtype == torch.int32 and probs.dtype == torch.float32
    assert topw.dtype == dtype
    assert torch.equal(topi[:3], ROUTE_EXPECT)
    assert _distinct_in_range(topi[3], 8)
    assert torch.equal(probs[0], torch.tensor([0.5, 0.5]))
    assert torch.equal(probs[2], torch.tensor([1.0, 0.0]))
    want = torch.softmax(torch.tensor([3.0, 2.0], dtype=torch.float64), 0)
    assert torch.allclose(probs[1].double(), want, rtol=1e-6, atol=0)
    # the public op on the CPU is the same routing
    r = ops.moe_route(logits, 2)
    assert torch.equal(r.topi, topi) and torch.equal(r.topw[:3], topw[:3])


def test_route_matches_topk_without_ties():
    logits = torch.randn(333, 8, generator=_gen(1))
    top3 = logits.topk(3, dim=-1).values
    assert bool((top3[:, :-1] > top3[:, 1:]).all())  # no tie in the top-(k+1)
    topi, probs, _ = R.moe_route(logits, 2)
    tv, ti = logits.topk(2, dim=-1)
    assert torch.equal(topi.long(), ti)
    assert torch.allclose(probs, torch.softmax(tv, dim=-1), rtol=1e-6, atol=0)


def _check_sort(topi, pos, src, offsets, e_lo, n_local):
    T, k = topi.shape
    flat = topi.reshape(-1).long()
    local = (flat >= e_lo) & (flat < e_lo + n_local)
    M = int(local.sum())
    counts = torch.bincount(flat[local] - e_lo, minlength=n_local)
    want_off = torch.cat([torch.zeros(1, dtype=torch.long),
                          torch.cumsum(counts, 0)])
    assert torch.equal(offsets.long(), want_off) and int(offsets[-1]) == M
    p = pos.reshape(-1).long()
    assert torch.equal(p < 0, ~local) and bool((p[~local] == -1).all())
    assert sorted(p[local].tolist()) == list(range(M))      # a permutation
    tok = torch.arange(T).repeat_interleave(k)
    assert torch.equal(src[:M].long()[p[local]], tok[local])  # src[pos] == t
    for el in range(n_local):
        lo, hi = int(offsets[el]), int(offsets[el + 1])
        seg = src[lo:hi].long()
        assert bool((seg[1:] >= seg[:-1]).all())              # stable
        assert bool((flat[local][torch.argsort(p[local])][lo:hi]
                     == e_lo + el).all())
    return M


def test_sort_reference():
    T, E, k = 333, 8, 2
    logits = torch.randn(T, E, generator=_gen(2))
    topi, _, _ = R.moe_route(logits, k)
    pos, src, offsets = R.moe_sort(topi, 0, E)
    assert pos.dtype == src.dtype == offsets.dtype == torch.int32
    assert _check_sort(topi, pos, src, offsets, 0, E) == T * k
    assert sorted(pos.reshape(-1).tolist()) == list(range(T * k))


def test_sort_reference_empty_expert():
    T, E, k = 333, 8, 2
    logits = torch.randn(T, E, generator=_gen(3))
    logits[:, 5] = -INF
    topi, _, _ = R.moe_route(logits, k)
    pos, src, offsets = R.moe_sort(topi, 0, E)
    _check_sort(topi, pos, src, offsets, 0, E)
    assert int(offsets[5]) == int(offsets[6])                 # empty slice
    r = ops.moe_route(logits, k)
    assert r.splits[5] == 0 and sum(r.splits) == T * k == r.rows


def test_expert_parallel_subsets():
    T, E, k, h = 97, 4, 2, 16
    g = _gen(4)
    logits = torch.randn(T, E, generator=g)
    full = ops.moe_route(logits, k)
    y = torch.randn(T * k, h, generator=g)
    want = R.moe_combine(y, full.topw, full.pos)
    parts, covered = [], torch.zeros(T, k, dtype=torch.int32)
    for e_lo in (0, 2):
        r = ops.moe_route(logits, k, e_lo=e_lo, n_local=2)
        assert torch.equal(r.topi, full.topi)
        _check_sort(r.topi, r.pos, r.src, r.offsets, e_lo, 2)
        covered += (r.pos >= 0).int()
        lo = int(full.offsets[e_lo])
        # the local permuted buffer is a contiguous slice of the full one
        assert torch.equal(torch.where(r.pos >= 0, r.pos + lo, r.pos),
                           torch.where(r.pos >= 0, full.pos,
                                       torch.full_like(full.pos, -1)))
        parts.append(ops.moe_combine(y[lo:lo + r.rows], r))
    assert bool((covered == 1).all())        # disjoint, and cover every pair
    assert torch.allclose(parts[0] + parts[1], want, rtol=0, atol=1e-6)


def test_slot_sums_and_adjoints_match_autograd():
    T, E, k, h = 61, 4, 2, 24
    g = _gen(5)
    logits = torch.randn(T, E, generator=g, dtype=torch.float64)
    r = ops.moe_route(logits.float(), k, e_lo=1, n_local=2)
    M = r.rows
    x = torch.randn(T, h, generator=g).requires_grad_(True)
    xp = ops.moe_gather(x, r)
    assert torch.equal(xp, x[r.src[:M].long()])
    dxp = torch.randn(M, h, generator=g)
    xp.backward(dxp)
    want = torch.zeros(T, h).index_add_(0, r.src[:M].long(), dxp)
    assert torch.allclose(x.grad, want, rtol=1e-6, atol=1e-6)
    no_local = (r.pos < 0).all(dim=1)
    assert bool(no_local.any()) and bool((x.grad[no_local] == 0).all())

    y = torch.randn(M, h, generator=g).requires_grad_(True)
    lg = logits.float().requires_grad_(True)
    r2 = ops.moe_route(lg, k, e_lo=1, n_local=2)
    out = ops.moe_combine(y, r2)
    dout = torch.randn(T, h, generator=g)
    out.backward(dout)
    # the same block written with dense torch ops
    y2 = y.detach().clone().requires_grad_(True)
    lg2 = logits.float().requires_grad_(True)
    tv, ti = lg2.topk(k, dim=-1)
    w = torch.softmax(tv, dim=-1)
    ref = torch.zeros(T, h)
    for s in range(k):
        p = r.pos[:, s].long()
        ref = ref + torch.where((p >= 0).unsqueeze(1),
                                w[:, s:s + 1] * y2[p.clamp_min(0)],
                                torch.zeros(()))
    ref.backward(dout)
    assert torch.allclose(out, ref, rtol=1e-6, atol=1e-6)
    assert torch.allclose(y.grad, y2.grad, rtol=1e-6, atol=1e-6)
    assert torch.allclose(lg.grad, lg2.grad, rtol=1e-5, atol=1e-6)


def test_grouped_linear_matches_loop_and_zeroes_empty_expert():
    g = _gen(6)
    splits = (5, 0, 9)
    xp = torch.randn(14, 12, generator=g).requires_grad_(True)
    w = torch.randn(3, 7, 12, generator=g).requires_grad_(True)
    out = ops.grouped_linear(xp, w, splits)
    dout = torch.randn(14, 7, generator=g)
    out.backward(dout)
    xp2 = xp.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    ref = torch.cat([xp2[:5] @ w2[0].t(), xp2[5:] @ w2[2].t()])
    ref.backward(dout)
    assert torch.allclose(out, ref, rtol=1e-6, atol=1e-6)
    assert torch.allclose(xp.grad, xp2.grad, rtol=1e-6, atol=1e-6)
    assert torch.allclose(w.grad, w2.grad, rtol=1e-6, atol=1e-6)
    assert bool((w.grad[1] == 0).all())
    with pytest.raises(ValueError):
        ops.grouped_linear(xp, w, (5, 9))


def test_whole_block_matches_the_expert_loop():
    cfg = llama.llama_moe_tiny()
    g = _gen(7)
    moe = llama.MoEMLP(cfg)
    with torch.no_grad():
        for p in moe.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    x = torch.randn(2, 83, cfg.hidden_size, generator=g)
    dout = torch.randn(2, 83, cfg.hidden_size, generator=g)

    logits = torch.nn.functional.linear(x.reshape(-1, cfg.hidden_size),
                                        moe.gate.weight).detach()
    top = logits.topk(cfg.top_k + 1, dim=-1).values
    assert bool((top[:, :-1] > top[:, 1:]).all()), "tie in the top-(k+1)"

    xa = x.clone().requires_grad_(True)
    out_loop = moe(xa)                       # CPU: the per-expert loop
    out_loop.backward(dout)
    want = {"out": out_loop.detach(), "dx": xa.grad,
            "gate": moe.gate.weight.grad.clone(),
            "w13": moe.experts_w13.grad.clone(),
            "w2": moe.experts_w2.grad.clone()}
    moe.zero_grad(set_to_none=True)

    xb = x.clone().requires_grad_(True)
    xf = xb.reshape(-1, cfg.hidden_size)
    out_fn = ops.moe_experts(
        xf, torch.nn.functional.linear(xf, moe.gate.weight),
        moe.experts_w13, moe.experts_w2, cfg.top_k).view_as(x)
    out_fn.backward(dout)
    got = {"out": out_fn.detach(), "dx": xb.grad,
           "gate": moe.gate.weight.grad, "w13": moe.experts_w13.grad,
           "w2": moe.experts_w2.grad}
    for name in want:
        assert torch.allclose(got[name], want[name], rtol=1e-5, atol=1e-6), (
            name, (got[name] - want[name]).abs().max().item())


def test_block_oracle_matches_the_expert_loop_and_emulation_is_near():
    """ops/testing.py's fp32 oracle (routing given) is the loop's math, and
    the bf16 emulation that sets the GPU test's per-row bound differs from it
    by bf16 rounding, not by a different formula."""
    from kubeflow_amd.ops import testing as T
    cfg = llama.llama_moe_tiny()
    g = _gen(9)
    moe = llama.MoEMLP(cfg)
    with torch.no_grad():
        for p in moe.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.05).bfloat16())
    h = cfg.hidden_size
    x = torch.randn(61, h, generator=g).bfloat16().float()
    dout = torch.randn(61, h, generator=g).bfloat16().float()
    xa = x.clone().requires_grad_(True)
    moe(xa.view(1, 61, h)).backward(dout.view(1, 61, h))
    topi = moe.gate(x).topk(cfg.top_k, dim=-1).indices
    args = (x, moe.gate.weight, moe.experts_w13, moe.experts_w2, topi, dout)
    want = (moe(x.view(1, 61, h)).detach().view(61, h), xa.grad,
            moe.gate.weight.grad, moe.experts_w13.grad, moe.experts_w2.grad)
    oracle = T.moe_mlp_oracle(*args)
    emu = T.moe_mlp_emulated(*args)
    for name, o, w, e in zip(("out", "dx", "gate", "w13", "w2"), oracle, want,
                             emu):
        metric = T.row_err if name in ("out", "dx") else T.col_err
        # two fp32 evaluations of one formula in different summation orders:
        # 2^-24 ~ 6e-8 per rounding; 1e-5 per row is far above that and far
        # below what a different formula or bf16 rounding (4e-3) would give
        assert metric(o, w) < 1e-5, (name, metric(o, w))
        assert 0 < metric(e, o) < 2e-2, (name, metric(e, o))
        assert torch.equal(e, e.bfloat16().float()), name   # holds bf16 values


def test_native_switch_is_off_the_gpu_path_on_cpu():
    x = torch.zeros(4, 16, dtype=torch.bfloat16)
    assert not ops.moe_native_ok(x, 4, 2)
    r = ops.moe_route(torch.randn(4, 4, generator=_gen(8)), 2)
    assert dataclasses.is_dataclass(r) and sum(r.splits) == r.rows == 8
    with pytest.raises(ValueError):
        ops.moe_route(torch.zeros(4, 4), 5)
    with pytest.raises(ValueError):
        ops.moe_route(torch.zeros(4, 4), 2, e_lo=3, n_local=2)
