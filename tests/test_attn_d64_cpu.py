"""flash_attention(kv_len=...) on the CPU reference path (no GPU): equals
reference.sdpa over the sliced k/v, k/v gradients are zero past kv_len, and
kv_len is rejected together with causal=True."""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import reference as R

B, S, HQ, HKV, D, N = 2, 24, 4, 2, 64, 9


def _inputs():
    g = torch.Generator(device="cpu").manual_seed(7)
    q = torch.randn(B, S, HQ, D, generator=g)
    k = torch.randn(B, S, HKV, D, generator=g)
    v = torch.randn(B, S, HKV, D, generator=g)
    return q, k, v


def test_kv_len_matches_sliced_sdpa():
    q, k, v = _inputs()
    got = ops.flash_attention(q, k, v, causal=False, kv_len=N)
    want = R.sdpa(q.transpose(1, 2), k[:, :N].transpose(1, 2),
                  v[:, :N].transpose(1, 2), causal=False).transpose(1, 2)
    assert got.shape == q.shape
    assert torch.equal(got, want)
    # kv_len == S is the unmasked call
    assert torch.equal(ops.flash_attention(q, k, v, causal=False, kv_len=S),
                       ops.flash_attention(q, k, v, causal=False))


def test_kv_len_grads_zero_past_n():
    q, k, v = (t.requires_grad_(True) for t in _inputs())
    g = torch.Generator(device="cpu").manual_seed(8)
    dout = torch.randn(B, S, HQ, D, generator=g)
    ops.flash_attention(q, k, v, causal=False, kv_len=N).backward(dout)
    assert torch.equal(k.grad[:, N:], torch.zeros_like(k.grad[:, N:]))
    assert torch.equal(v.grad[:, N:], torch.zeros_like(v.grad[:, N:]))
    assert k.grad[:, :N].abs().max() > 0 and v.grad[:, :N].abs().max() > 0
    assert q.grad.abs().max() > 0


def test_kv_len_with_causal_raises():
    q, k, v = _inputs()
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, causal=True, kv_len=N)
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, causal=False, kv_len=S + 1)
