"""MXFP4 (OCP e2m1 elements, one e8m0 scale per 32 along K) on the CPU: the
quantizer's format and rounding, the public layout, and the fallbacks of the
q4 linears and of the serving engine."""
import pytest
import torch
import torch.nn.functional as F

from kubeflow_amd import ops
from kubeflow_amd.ops import reference as R


def _weights(seed, N=24, K=128):
    """Block magnitudes spread over 2^-8 .. 2^3 so every binade of the grid
    and a wide range of scale bytes occur."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(N, K // 32, 1, generator=g) * 11 - 8)
    return (torch.randn(N, K // 32, 32, generator=g) * mag).reshape(N, K)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dequantized_weights_are_a_fixed_point(dtype):
    w4, sc = ops.quantize_mxfp4_rows(_weights(1).to(dtype))
    assert w4.dtype == sc.dtype == torch.uint8
    assert w4.shape == (24, 64) and sc.shape == (24, 4)
    assert 0 < int(sc.min()) and int(sc.max()) < 255
    dq = ops.dequantize_mxfp4_rows(w4, sc, dtype)
    # exact in bf16: the fp32 and the bf16 dequantization are the same numbers
    assert torch.equal(dq.float(), ops.dequantize_mxfp4_rows(w4, sc,
                                                             torch.float32))
    w4b, scb = ops.quantize_mxfp4_rows(dq)
    assert torch.equal(w4b, w4) and torch.equal(scb, sc)


def test_every_element_is_within_half_a_grid_step():
    w = _weights(2)
    w4, sc = ops.quantize_mxfp4_rows(w)
    dq = ops.dequantize_mxfp4_rows(w4, sc, torch.float32)
    s = torch.exp2(sc.float() - 127).repeat_interleave(32, dim=1)
    a = (w / s).abs()
    half = 0.25 * torch.where(a < 2, 1.0, torch.where(a < 4, 2.0, 4.0))
    ok = ((w - dq).abs() <= half * s) | (a > 6)
    assert bool(ok.all())
    assert bool(((dq / s).abs()[a > 6] == 6).all())   # saturated, not wrapped
    assert float((a > 6).float().mean()) < 0.2


def test_fixed_blocks():
    vals = [0.5, 1, 1.5, 2, 3, 4, 6, -6, -0.5, 0, -0.1] + [0] * 21
    w = torch.zeros(3, 64)
    w[0, :32] = torch.tensor(vals) / 8            # absmax 6 * 2^-3: b = 124
    w[1, 32:] = torch.tensor(vals[::-1]) * 2.0 ** 40
    w[2, 0], w[2, 33] = 7.9, -1e-45               # saturates; b clamps to 1
    w4, sc = ops.quantize_mxfp4_rows(w)
    # element 2i in the low nibble of byte i; -0.1/8 rounds to +0, never -0
    assert w4[0, :6].tolist() == [0x21, 0x43, 0x65, 0xF7, 0x09, 0x00]
    assert w4[1, -6:].tolist() == [0x00, 0x90, 0x7F, 0x56, 0x34, 0x12]
    assert sc.tolist() == [[124, 127], [127, 167], [127, 1]]
    assert not w4[0, 6:].any() and not w4[1, :16].any()
    assert w4[2, 0] == 0x07 and w4[2, 16] == 0x00


def test_q4_linears_fall_back_to_the_dequantized_weights():
    g = torch.Generator().manual_seed(3)
    E, N, K = 3, 16, 64
    w4, sc = ops.quantize_mxfp4_rows(_weights(4, E * N, K))
    dq = ops.dequantize_mxfp4_rows(w4, sc, torch.float32)
    x = torch.randn(5, K, generator=g)
    res = torch.randn(5, N, generator=g)
    assert torch.equal(ops.skinny_linear_q4(x, w4[:N], sc[:N], residual=res),
                       F.linear(x, dq[:N]) + res)
    offsets = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    rows = torch.tensor([4, 0, 3, 3, 1], dtype=torch.int32)
    for r in (None, rows):
        assert torch.equal(
            ops.grouped_skinny_linear_q4(x, w4, sc, offsets, 3, r),
            R.grouped_linear_offsets(x, dq.view(E, N, K), offsets, r))
    with pytest.raises(ValueError):
        ops.skinny_linear_q4(x, w4[:N], sc[:N, :1])
    with pytest.raises(ValueError):
        ops.grouped_skinny_linear_q4(x, w4, sc.float(), offsets, 3)


def test_mxfp4_engine_generates():
    from kubeflow_amd.runtime.serving import InferenceEngine

    torch.manual_seed(11)
    eng = InferenceEngine("llama-tiny", max_slots=4, smax=128, max_batch=4,
                          quant="mxfp4")
    assert eng.quant is True and eng.quant_format == "mxfp4"
    assert eng._qw[0]["wqkv"][1].dtype == torch.uint8
    eng.start(precapture=False)
    try:
        r = eng.generate([5, 3, 8, 1], max_new_tokens=5, timeout=60)
        assert not r.error
        assert len(r.generated) == 5
        assert all(0 <= t < eng.model.cfg.vocab_size for t in r.generated)
    finally:
        eng.stop()
    with pytest.raises(ValueError, match="fp8, mxfp4"):
        InferenceEngine("llama-tiny", max_slots=4, smax=128, quant="int3")
