"""ops.grouped_linear_q4 and ops.moe_experts_q4 off the GPU: the reference
path on the dequantized banks, exactly."""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import reference


def _bank(E, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return ops.quantize_mxfp4_rows(torch.randn(E * N, K, generator=g))


@pytest.mark.parametrize("swiglu", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_grouped_linear_q4_cpu_is_the_reference(gather, swiglu):
    E, N, K = 3, 64, 96
    w4, sc = _bank(E, N, K, 1)
    off = torch.tensor([0, 5, 5, 12], dtype=torch.int32)
    x = torch.randn(6 if gather else 12, K)
    rows = (torch.arange(12) % 6).int() if gather else None
    want = reference.grouped_linear_offsets(
        x, ops.dequantize_mxfp4_rows(w4, sc, x.dtype).view(E, N, K), off, rows)
    if swiglu:
        want = ops.swiglu(want)
    got = ops.grouped_linear_q4(x, w4, sc, off, rows, swiglu=swiglu)
    assert got.shape == (12, N // 2 if swiglu else N)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.grouped_linear_q4(x[:, :64], w4, sc, off, rows)


def test_moe_experts_q4_cpu_is_moe_experts_on_the_dequantized_banks():
    E, h, f, k = 4, 64, 32, 2
    q4 = (_bank(E, 2 * f, h, 2), _bank(E, h, f, 3))
    w13, w2 = (ops.dequantize_mxfp4_rows(*p, torch.float32) for p in q4)
    g = torch.Generator().manual_seed(4)
    x, logits = torch.randn(40, h, generator=g), torch.randn(40, E,
                                                             generator=g)
    want = ops.moe_experts(x, logits, w13.view(E, 2 * f, h),
                           w2.view(E, h, f), k)
    assert torch.equal(ops.moe_experts_q4(x, logits, q4, k), want)
