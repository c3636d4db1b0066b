"""The per-row parity metric of kubeflow_amd/ops/testing.py, on the CPU.

No kernel runs here. For the attention families the tests show that
  1. the all-bf16 emulation passes its own 3 x bound against the fp32 oracle
     (trivially < 1 x: the bound has room for a correct implementation);
  2. two single-tile defects FAIL the per-row bound: one 32-row tile (rows
     32..63 of one head) sees one extra key (causal mask off by one), and one
     row of an output is zero (a dropped store). Both are applied to the fp32
     oracle's outputs and gradients, so nothing but the defect is measured;
  3. the same defects PASS the whole-tensor Frobenius bounds of
     tests/test_ops_gpu.py (2e-2 forward, 4e-2 gradients), which is why the
     per-row metric exists.

1 and 2 run on the smallest causal shape of each family (D = 128 4-wave, D =
128 8-wave, D = 64). 3 is a statement about averaging, so it depends on how
large the tensor is next to one tile: at B1 S128 Hq4 one 32-row tile is 1/16
of the tensor and the extra key alone moves o by 0.049 of its norm. It is
asserted (together with 1 and 2) at the shape it was first measured at, B1
S512 Hq8 Hkv2 D128 causal, where one tile is 1/128 of the tensor: whole-tensor
0.015 / 0.012-0.013 (extra key: o, dv / dq, dk), 0.010-0.020 (zeroed row),
per-row 0.17-0.70.
"""
import pytest
import torch

from kubeflow_amd.ops import testing as T

FWD_BOUND = 2e-2  # tests/test_ops_gpu.py::test_attention_fwd
BWD_BOUND = 4e-2  # tests/test_ops_gpu.py::test_attention_bwd
NAMES = ("o", "dq", "dk", "dv")

# (B, S, Hq, Hkv, D), all causal
SMALLEST = {
    "d128_4wave": (1, 128, 4, 1, 128),   # S % 256 != 0
    "d128_8wave": (1, 256, 4, 2, 128),   # smallest 256 multiple
    "d64": (1, 128, 4, 1, 64),
}
AVERAGING = {
    "d128_table_shape": (1, 512, 8, 2, 128),
}
ALL = {**SMALLEST, **AVERAGING}

_mut = {}


def _case(name):
    B, S, Hq, Hkv, D = ALL[name]
    return T.attention_case(B, S, Hq, Hkv, True, D=D)


def _extra_key(name):
    """fp32 (o, dq, dk, dv) where rows 32..63 of the last head of batch 0 also
    attend key row + 1; everything else is the oracle's math."""
    if name in _mut:
        return _mut[name]
    B, S, Hq, Hkv, D = ALL[name]
    q, k, v, dout = _case(name).inputs
    mask = torch.ones(S, S, dtype=torch.bool).tril().expand(
        B, Hq, S, S).clone()
    for r in range(32, 64):
        mask[0, Hq - 1, r, r + 1] = True
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    g = Hq // Hkv
    s = torch.einsum("bqhd,bkhd->bhqk", qr,
                     kr.repeat_interleave(g, dim=2)) * D ** -0.5
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
    o = torch.einsum("bhqk,bkhd->bqhd", p, vr.repeat_interleave(g, dim=2))
    o.backward(dout.float())
    _mut[name] = dict(zip(NAMES, (o.detach(), qr.grad, kr.grad, vr.grad)))
    return _mut[name]


def _zero_row(name, out):
    """The oracle's `out` with row S/2 of the last head of batch 0 zeroed."""
    S = ALL[name][1]
    z = _case(name).oracle[out].clone()
    z[0, S // 2, -1] = 0
    return z


def _whole_bound(out):
    return FWD_BOUND if out == "o" else BWD_BOUND


def test_mutation_helpers_match_oracle_when_not_mutated():
    """The explicit-mask math used for the extra-key defect is the oracle's
    math: outside the mutated head every output row is the oracle's."""
    name = "d128_4wave"
    c, m = _case(name), _extra_key(name)
    for out in ("o", "dq"):  # per-q-head outputs: other heads untouched
        assert torch.allclose(m[out][:, :, :-1], c.oracle[out][:, :, :-1],
                              rtol=1e-5, atol=1e-6), out


@pytest.mark.parametrize("name", list(ALL))
def test_emulation_passes_its_own_bound(name):
    c = _case(name)
    print(name, "emulated per-row", c.emu_err, "bound", c.bound)
    for out in NAMES:
        assert 0 < c.emu_err[out] < c.bound[out]
        assert c.bound[out] == 3 * c.emu_err[out]
        # an all-bf16 pipeline stays within the whole-tensor bounds too
        assert c.emu_err[out] < 0.1, (out, c.emu_err)


@pytest.mark.parametrize("name", list(ALL))
def test_extra_key_fails_per_row_bound(name):
    c, m = _case(name), _extra_key(name)
    for out in NAMES:
        err = T.row_err(m[out], c.oracle[out])
        print(name, out, "row_err", err, "bound", c.bound[out])
        assert err > c.bound[out], (out, err, c.bound[out])


@pytest.mark.parametrize("name", list(ALL))
def test_zeroed_row_fails_per_row_bound(name):
    c = _case(name)
    for out in NAMES:
        err = T.row_err(_zero_row(name, out), c.oracle[out])
        print(name, out, "row_err", err, "bound", c.bound[out])
        assert err > c.bound[out], (out, err, c.bound[out])


@pytest.mark.parametrize("name", list(AVERAGING))
def test_same_mutations_pass_whole_tensor_bound(name):
    c, m = _case(name), _extra_key(name)
    for out in NAMES:
        e1 = T.rel_err(m[out], c.oracle[out])
        e2 = T.rel_err(_zero_row(name, out), c.oracle[out])
        print(name, out, "whole-tensor: extra key", e1, "zeroed row", e2)
        assert 0 < e1 < _whole_bound(out), (out, e1)
        assert 0 < e2 < _whole_bound(out), (out, e2)


def test_row_err_definition():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0]])   # norms 5, 0; rms = 5/sqrt2
    got = torch.tensor([[3.0, 4.0], [1.0, 0.0]])
    rms = (25.0 / 2) ** 0.5
    assert T.row_err(ref, ref) == 0.0
    assert abs(T.row_err(got, ref) - 1.0 / rms) < 1e-6  # floored by rms
    got2 = torch.tensor([[0.0, 4.0], [0.0, 0.0]])
    assert abs(T.row_err(got2, ref) - 3.0 / 5.0) < 1e-6  # by the row's norm
    nan = got.clone()
    nan[1, 1] = float("nan")
    assert not T.row_err(nan, ref) < 1.0  # NaN fails every bound
    # col_err: the same over columns; a vector's elements are its own rows
    assert abs(T.col_err(got.t().contiguous(), ref.t().contiguous())
               - 1.0 / rms) < 1e-6
    v = torch.tensor([1.0, -1.0, 1.0, -1.0])
    w = torch.tensor([1.0, -1.0, 1.0, 0.0])
    assert abs(T.col_err(w, v) - 1.0) < 1e-6


def test_oracles_agree_with_torch_autograd():
    """Spot-check the thin oracle wrappers against independent torch ops."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(6, 16, generator=g)
    w = torch.randn(16, generator=g)
    b = torch.randn(16, generator=g)
    dy = torch.randn(6, 16, generator=g)
    y, dx, dw, db = T.layer_norm_oracle(x, w, b, dy, eps=1e-6)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = torch.nn.functional.layer_norm(xr, (16,), wr, br, eps=1e-6)
    yr.backward(dy)
    for a, r in ((y, yr), (dx, xr.grad), (dw, wr.grad), (db, br.grad)):
        assert torch.allclose(a, r.detach(), atol=1e-5)
    # all-ignored CE: loss 0, zero grad (the wrapper's semantics)
    loss, dl = T.cross_entropy_oracle(x, torch.full((6,), -100))
    assert loss.item() == 0.0 and not dl.any()
    # masked AdamW = torch.optim.AdamW with decay on the masked elements only
    p0 = torch.randn(8, generator=g)
    gs = [torch.randn(8, generator=g) for _ in range(2)]
    mask = torch.tensor([1.0, 0, 1, 0, 1, 1, 0, 0])
    p, m, v = T.adamw_oracle(p0, gs, mask, 1e-2, 0.9, 0.95, 1e-8, 0.1)
    pa = p0[mask.bool()].clone().requires_grad_(True)
    pb = p0[~mask.bool()].clone().requires_grad_(True)
    opt = torch.optim.AdamW([
        {"params": [pa], "weight_decay": 0.1},
        {"params": [pb], "weight_decay": 0.0}],
        lr=1e-2, betas=(0.9, 0.95), eps=1e-8)
    for gg in gs:
        pa.grad, pb.grad = gg[mask.bool()].clone(), gg[~mask.bool()].clone()
        opt.step()
    assert torch.allclose(p[mask.bool()], pa.detach(), atol=1e-6)
    assert torch.allclose(p[~mask.bool()], pb.detach(), atol=1e-6)
    # decode oracle: len 0 gives a zero row
    q = torch.randn(2, 2, 8, generator=g)
    kc = torch.randn(2, 4, 1, 8, generator=g)
    o = T.decode_oracle(q, kc, kc, torch.tensor([0, 1]), torch.tensor([0, 1]))
    assert not o[0].any()
    assert torch.allclose(o[1], kc[1, 0].expand(2, 8), atol=1e-6)
