"""Head-dim-64 attention family (attention_d64.hip) through the public ops.

Inputs are seeded bf16 randn built on the CPU; the oracle is the fp32
reference.sdpa on CPU copies with k/v sliced to kv_len. Bounds are the
project's own: forward rel. error < 2e-2 (test_attention_fwd), each of
dq/dk/dv < 4e-2 (test_attention_bwd). Shapes are the smallest that reach
every branch: one and several q blocks, diagonal / off-diagonal tiles, GQA
head loop, odd head count, the wrapper pad path, kv_len inside a tile, one
past a 128 boundary and exactly on a tile edge.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.ops import reference as R

D = 64
FWD_BOUND = 2e-2  # test_attention_fwd's bound
BWD_BOUND = 4e-2  # test_attention_bwd's bound
GARBAGE = 1e4     # fills k/v rows >= kv_len: finite, never to be read

# name -> (B, S, Hq, Hkv, causal, kv_len)
CASES = {
    "one_block": (2, 128, 4, 4, False, None),
    "causal_gqa": (1, 256, 4, 2, True, None),
    "odd_heads_three_blocks": (2, 384, 3, 3, False, None),
    "pad_causal": (1, 100, 2, 2, True, None),
    "pad_non_causal": (1, 100, 2, 2, False, None),
    "kv_inside_tile": (2, 128, 4, 4, False, 37),
    "kv_past_boundary": (1, 256, 2, 2, False, 129),
    "kv_on_tile_edge": (1, 256, 4, 1, False, 64),
}
KV_CASES = [n for n, c in CASES.items() if c[5] is not None]

_cache = {}


def _relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _inputs(B, S, Hq, Hkv, kv_len, seed=1234):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, S, Hq, D, generator=g).bfloat16()
    k = torch.randn(B, S, Hkv, D, generator=g).bfloat16()
    v = torch.randn(B, S, Hkv, D, generator=g).bfloat16()
    dout = torch.randn(B, S, Hq, D, generator=g).bfloat16()
    if kv_len is not None:
        k[:, kv_len:] = GARBAGE
        v[:, kv_len:] = GARBAGE
    return q, k, v, dout


def _oracle(q, k, v, dout, causal, kv_len):
    """fp32 CPU reference: (o, dq, dk, dv); dk/dv are zero past kv_len."""
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    kk, vv = (kr, vr) if kv_len is None else (kr[:, :kv_len], vr[:, :kv_len])
    o = R.sdpa(qr.transpose(1, 2), kk.transpose(1, 2), vv.transpose(1, 2),
               causal=causal).transpose(1, 2)
    o.backward(dout.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


def _gpu_run(q, k, v, dout, causal, kv_len):
    dev = torch.device("cuda", 0)
    qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    o = ops.flash_attention(qg, kg, vg, causal=causal, kv_len=kv_len)
    o.backward(dout.to(dev))
    torch.cuda.synchronize()
    return o.detach(), qg.grad, kg.grad, vg.grad


def _case(name):
    if name not in _cache:
        B, S, Hq, Hkv, causal, kv_len = CASES[name]
        q, k, v, dout = _inputs(B, S, Hq, Hkv, kv_len)
        _cache[name] = (_gpu_run(q, k, v, dout, causal, kv_len),
                        _oracle(q, k, v, dout, causal, kv_len))
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_fwd_bwd_matches_oracle(name):
    got, want = _case(name)
    errs = {n: _relerr(g, w)
            for n, g, w in zip(("o", "dq", "dk", "dv"), got, want)}
    print(name, errs)
    assert got[0].shape == want[0].shape
    assert errs["o"] < FWD_BOUND, errs
    for n in ("dq", "dk", "dv"):
        assert errs[n] < BWD_BOUND, errs


@pytest.mark.parametrize("name", KV_CASES)
def test_kv_len_grads_exact_zero_past_kv_len(name):
    (_, _, dk, dv), _ = _case(name)
    kv_len = CASES[name][5]
    assert torch.equal(dk[:, kv_len:], torch.zeros_like(dk[:, kv_len:]))
    assert torch.equal(dv[:, kv_len:], torch.zeros_like(dv[:, kv_len:]))


def test_kv_len_one_returns_first_value_row():
    B, S, Hq, Hkv = 1, 128, 2, 1
    q, k, v, _ = _inputs(B, S, Hq, Hkv, 1)
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        o = ops.flash_attention(q.to(dev), k.to(dev), v.to(dev),
                                causal=False, kv_len=1)
    want = v[:, 0].view(B, 1, Hkv, D).expand(B, S, Hq, D)
    assert torch.equal(o.cpu(), want)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _fp(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("kv_len", [37, 128])
def test_direct_fwd_lse(kv_len):
    from kubeflow_amd.ops import _backend
    lib = _backend.require()
    B, S, Hq, Hkv = 2, 128, 4, 4
    dev = torch.device("cuda", 0)
    q, k, v, _ = _inputs(B, S, Hq, Hkv, kv_len if kv_len < S else None)
    qg, kg, vg = q.to(dev), k.to(dev), v.to(dev)
    o = torch.empty_like(qg)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
    err = lib.kf_attn64_fwd(_p(o), _fp(lse), _p(qg), _p(kg), _p(vg), B, S, Hq,
                            Hkv, 0, 0, D ** -0.5, 0, kv_len, _stream())
    assert err == 0, err
    torch.cuda.synchronize()
    scores = torch.einsum("bqhd,bkhd->bhqk", q.float(),
                          k[:, :kv_len].float()) * D ** -0.5
    want = torch.logsumexp(scores, dim=-1)
    assert torch.allclose(lse.cpu(), want, atol=1e-2), \
        (lse.cpu() - want).abs().max()


def test_direct_fwd_rejects_causal_with_kv_len():
    """Host-side argument check: returns before any launch."""
    from kubeflow_amd.ops import _backend
    lib = _backend.require()
    B, S, Hq, Hkv = 1, 128, 2, 2
    dev = torch.device("cuda", 0)
    q, k, v, _ = _inputs(B, S, Hq, Hkv, None)
    qg, kg, vg = q.to(dev), k.to(dev), v.to(dev)
    o = torch.empty_like(qg)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
    err = lib.kf_attn64_fwd(_p(o), _fp(lse), _p(qg), _p(kg), _p(vg), B, S, Hq,
                            Hkv, 0, 0, D ** -0.5, 1, 64, _stream())
    assert err != 0


def test_masked_attention_shares_the_kernel():
    B, S, H, kv_len = 2, 128, 12, 37
    q, k, v, dout = _inputs(B, S, H, H, kv_len)
    dev = torch.device("cuda", 0)
    qg, kg, vg = q.to(dev), k.to(dev), v.to(dev)
    got = ops.masked_attention(qg, kg, vg, kv_len)
    with torch.no_grad():
        same = ops.flash_attention(qg, kg, vg, causal=False, kv_len=kv_len)
    want = _oracle(q, k, v, dout, False, kv_len)[0]
    assert _relerr(got, want) < FWD_BOUND
    assert torch.equal(got, same)


def test_backward_is_deterministic():
    B, S, Hq, Hkv, causal, kv_len = CASES["causal_gqa"]
    q, k, v, dout = _inputs(B, S, Hq, Hkv, kv_len)
    a = _gpu_run(q, k, v, dout, causal, kv_len)
    b = _gpu_run(q, k, v, dout, causal, kv_len)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_reference_route_switch(monkeypatch):
    """KF_ATTN_D64=0: same call, torch reference math on the GPU."""
    monkeypatch.setenv("KF_ATTN_D64", "0")
    name = "kv_inside_tile"
    B, S, Hq, Hkv, causal, kv_len = CASES[name]
    q, k, v, dout = _inputs(B, S, Hq, Hkv, kv_len)
    got = _gpu_run(q, k, v, dout, causal, kv_len)
    want = _oracle(q, k, v, dout, causal, kv_len)
    assert _relerr(got[0], want[0]) < FWD_BOUND
    for g, w in zip(got[1:], want[1:]):
        assert _relerr(g, w) < BWD_BOUND


def test_d128_with_kv_len_raises():
    dev = torch.device("cuda", 0)
    q = torch.zeros(1, 128, 2, 128, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="masked_attention"):
        ops.flash_attention(q, q, q, causal=False, kv_len=64)


def test_unsupported_head_dim_raises():
    dev = torch.device("cuda", 0)
    q = torch.zeros(1, 128, 2, 32, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="64"):
        ops.flash_attention(q, q, q, causal=False)


# ------------------------------------------------------------- mask probe

def _probe_check(name, o, dv, oracle_o, oracle_dv, hot_o, hot_dv):
    """testing.mask_probe_inputs: per-row FWD_BOUND / BWD_BOUND against the
    fp32 oracle on the probe inputs and against the closed form."""
    from kubeflow_amd.ops import testing as T
    errs = dict(o=T.row_err(o, oracle_o), o_hot=T.row_err(o, hot_o),
                dv=T.row_err(dv, oracle_dv), dv_hot=T.row_err(dv, hot_dv))
    print(f"PARITY {name} probe o row={errs['o']:.5f} "
          f"row_vs_v={errs['o_hot']:.5f} bound={FWD_BOUND} "
          f"dv row={errs['dv']:.5f} row_vs_dout={errs['dv_hot']:.5f} "
          f"bound={BWD_BOUND}")
    assert o.shape == oracle_o.shape and dv.shape == oracle_dv.shape
    assert errs["o"] < FWD_BOUND and errs["o_hot"] < FWD_BOUND, errs
    assert errs["dv"] < BWD_BOUND and errs["dv_hot"] < BWD_BOUND, errs


@pytest.mark.parametrize("causal,kv_len", [(True, None), (False, 137)])
def test_mask_probe(causal, kv_len):
    """Scores 8 * j (testing.mask_probe_inputs) at S = 200, the pad path.
    Causal: o row i is v[i] and dv row j the group's dout rows at j.
    kv_len = 137: every o row is v[136], dv[136] the sum of all dout rows of
    the group, dv rows past kv_len exact zeros. A mask off by one key in one
    row gives a per-row error above 1 (tests/test_attn_probe_cpu.py)."""
    from kubeflow_amd.ops import testing as T
    B, S, Hq, Hkv = 1, 200, 4, 2
    g = Hq // Hkv
    q, k, v, scale = T.mask_probe_inputs(B, S, S, Hq, Hkv, D, seed=61)
    gen = torch.Generator(device="cpu").manual_seed(62)
    dout = torch.randn(B, S, Hq, D, generator=gen).bfloat16()
    oo, _, _, _, odv = T.attention_oracle(q, k, v, dout, causal, scale,
                                          kv_len=kv_len)
    dsum = dout.float().view(B, S, Hkv, g, D).sum(dim=3)
    if causal:
        hot_o = v.float().repeat_interleave(g, dim=2)
        hot_dv = dsum
    else:
        k[:, kv_len:] = GARBAGE
        v[:, kv_len:] = GARBAGE
        hot_o = v.float()[:, kv_len - 1:kv_len].repeat_interleave(
            g, dim=2).expand(B, S, Hq, D)
        hot_dv = torch.zeros(B, S, Hkv, D)
        hot_dv[:, kv_len - 1] = dsum.sum(dim=1)
    dev = torch.device("cuda", 0)
    qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    o = ops.flash_attention(qg, kg, vg, causal=causal, scale=scale,
                            kv_len=kv_len)
    o.backward(dout.to(dev))
    torch.cuda.synchronize()
    _probe_check(f"d64 causal={causal} kv_len={kv_len}", o.detach(), vg.grad,
                 oo, odv, hot_o, hot_dv)
    if kv_len is not None:
        assert not vg.grad[:, kv_len:].any()
