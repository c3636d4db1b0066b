"""Routed MoE decode, the parts that run without a GPU: moe_route(sync=False),
the reference grouped linear over offsets, ops.moe_experts_decode against
ops.moe_experts, and MoEMLP.decode_routed, which on the CPU is decode_dense.
"""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.models.llama import LlamaConfig, MoEMLP
from kubeflow_amd.ops import reference as R


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


@pytest.mark.parametrize("T,E,k", [(1, 4, 2), (5, 8, 2), (32, 8, 3)])
def test_route_nosync_returns_the_same_tensors(T, E, k):
    lg = torch.randn(T, E, generator=_gen(T + E))
    a = ops.moe_route(lg, k)
    b = ops.moe_route(lg, k, sync=False)
    for name in ("topi", "topw", "probs", "pos", "src", "offsets"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert b.splits is None
    assert b.rows == T * k == a.rows
    assert (b.e_lo, b.n_local) == (0, E)
    assert isinstance(a.splits, tuple) and sum(a.splits) == T * k


def test_route_nosync_needs_every_expert_local():
    lg = torch.randn(6, 4, generator=_gen(0))
    with pytest.raises(ValueError, match="sync=False"):
        ops.moe_route(lg, 2, 0, 2, sync=False)
    with pytest.raises(ValueError, match="sync=False"):
        ops.moe_route(lg, 2, 2, 2, sync=False)
    assert ops.moe_route(lg, 2, 0, 4, sync=False).rows == 12


def test_grouped_skinny_ok_follows_the_kernels_shape_rules():
    bf = torch.bfloat16
    assert ops.grouped_skinny_ok(32, 1024, 512, bf)
    assert ops.grouped_skinny_ok(16, 1024, 256, bf)       # direct kernel
    assert not ops.grouped_skinny_ok(17, 1024, 256, bf)   # direct: M <= 16
    assert not ops.grouped_skinny_ok(33, 1024, 512, bf)
    assert not ops.grouped_skinny_ok(0, 1024, 512, bf)
    assert not ops.grouped_skinny_ok(4, 1000, 512, bf)    # N % 16
    assert not ops.grouped_skinny_ok(4, 1024, 48, bf)     # K % 32
    assert not ops.grouped_skinny_ok(4, 1024, 512, torch.float32)
    assert ops.grouped_skinny_ok(32, 1024, 2048, bf, q8=True)
    assert not ops.grouped_skinny_ok(4, 1024, 512, bf, q8=True)


# (rows, N, K, q8, accepted), from the "Shapes" rule of docs/KERNELS.md: LDS
# kernel K % 512 (q8: K % 1024) up to 32 rows, direct kernel K % 32 up to 16
# rows, N % 16, at least one row
SHAPE_RULE = [
    (0, 64, 512, False, False), (1, 64, 512, False, True),
    (16, 64, 512, False, True), (17, 64, 512, False, True),
    (32, 64, 512, False, True), (33, 64, 512, False, False),
    (16, 64, 96, False, True), (17, 64, 96, False, False),
    (4, 64, 40, False, False), (4, 24, 512, False, False),
    (4, 64, 512, True, False), (4, 64, 1024, True, True),
]


@pytest.mark.parametrize("rows,N,K,q8,accepted", SHAPE_RULE)
def test_skinny_shape_rule_is_one_predicate(rows, N, K, q8, accepted):
    """The rule skinny_linear, skinny_linear_q8 and grouped_skinny_ok share."""
    assert ops._skinny_shape_ok(rows, N, K, q8) is accepted
    assert ops.grouped_skinny_ok(rows, N, K, torch.bfloat16, q8=q8) is accepted
    # what grouped_skinny_ok asks on top: no empty dimension, bf16 only
    assert ops.grouped_skinny_ok(rows, 0, K, torch.bfloat16, q8=q8) is False
    assert ops.grouped_skinny_ok(rows, N, 0, torch.bfloat16, q8=q8) is False
    assert ops.grouped_skinny_ok(rows, N, K, torch.float16, q8=q8) is False


def test_reference_grouped_linear_empty_and_full_experts():
    g = _gen(3)
    x = torch.randn(6, 16, generator=g)
    bank = torch.randn(3, 8, 16, generator=g)
    # expert 1 empty
    off = torch.tensor([0, 4, 4, 6], dtype=torch.int32)
    y = R.grouped_linear_offsets(x, bank, off)
    assert torch.equal(y[:4], x[:4] @ bank[0].t())
    assert torch.equal(y[4:], x[4:] @ bank[2].t())
    # expert 2 holds every row, read through `rows` (with repeats)
    rows = torch.tensor([5, 0, 0, 3, 2, 5, 1], dtype=torch.int32)
    off = torch.tensor([0, 0, 0, 7], dtype=torch.int32)
    y = R.grouped_linear_offsets(x, bank, off, rows)
    assert y.shape == (7, 8)
    assert torch.equal(y, x[rows.long()] @ bank[2].t())
    # the public op takes the same path off the GPU, with and without out=
    assert torch.equal(ops.grouped_skinny_linear(x, bank, off, 7, rows), y)
    out = torch.full((9, 8), float("nan"))
    got = ops.grouped_skinny_linear(x, bank, off, 7, rows, out=out)
    assert got is out and torch.equal(out[:7], y)
    assert bool(torch.isnan(out[7:]).all())
    # rows past offsets[-1] belong to no expert: zeros in the reference
    off = torch.tensor([0, 2, 2, 3], dtype=torch.int32)
    y = R.grouped_linear_offsets(x, bank, off)
    assert bool((y[3:] == 0).all()) and torch.equal(y[2:3],
                                                    x[2:3] @ bank[2].t())


def test_reference_grouped_linear_q8_dequantizes_the_flat_bank():
    g = _gen(4)
    x = torch.randn(5, 32, generator=g)
    bank = torch.randn(2, 16, 32, generator=g)
    w8, scale = ops.quantize_fp8_rows(bank.reshape(-1, 32))
    off = torch.tensor([0, 2, 5], dtype=torch.int32)
    y = ops.grouped_skinny_linear_q8(x, w8, scale, off, 5)
    deq = ops.dequantize_fp8_rows(w8, scale, x.dtype).view(2, 16, 32)
    assert torch.equal(y[:2], x[:2] @ deq[0].t())
    assert torch.equal(y[2:], x[2:] @ deq[1].t())


@pytest.mark.parametrize("variant", ["plain", "one_pair", "empty_expert"])
def test_experts_decode_equals_experts_on_the_cpu(variant):
    T, E, k, h, f = 7, 8, 2, 32, 48
    g = _gen(11)
    x = torch.randn(T, h, generator=g)
    lg = torch.randn(T, E, generator=g)
    if variant == "one_pair":
        lg[:, 6:] += 100.0          # every token on experts {6, 7}
    elif variant == "empty_expert":
        lg[:, 2] = float("-inf")
    w13 = torch.randn(E, 2 * f, h, generator=g) * 0.1
    w2 = torch.randn(E, h, f, generator=g) * 0.1
    want = ops.moe_experts(x, lg, w13, w2, k)
    got = ops.moe_experts_decode(x, lg, w13, w2, k)
    assert torch.equal(got, want)


def test_decode_routed_matches_decode_dense_on_the_cpu():
    """The bound of test_moe_decode_dense_matches_routed."""
    torch.manual_seed(21)
    cfg = LlamaConfig(vocab_size=64, hidden_size=32, n_layers=1, n_heads=4,
                      n_kv_heads=2, ffn_dim=48, max_seq_len=64,
                      n_experts=4, top_k=2)
    moe = MoEMLP(cfg)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.1)
    x = torch.randn(5, 1, 32)
    assert not moe.routed_decode_ok(x)
    with torch.no_grad():
        routed = moe.decode_routed(x)
        dense = moe.decode_dense(x)
        full = moe(x)
    assert torch.allclose(routed, dense, atol=1e-5, rtol=1e-4), \
        (routed - dense).abs().max()
    assert torch.allclose(routed, full, atol=1e-5, rtol=1e-4)


def test_moe_decode_knob_is_validated(monkeypatch):
    from kubeflow_amd.runtime import serving

    monkeypatch.delenv("KF_MOE_DECODE", raising=False)
    assert serving.moe_decode_mode() == "routed"
    monkeypatch.setenv("KF_MOE_DECODE", "dense")
    assert serving.moe_decode_mode() == "dense"
    monkeypatch.setenv("KF_MOE_DECODE", "sparse")
    with pytest.raises(ValueError, match="KF_MOE_DECODE"):
        serving.moe_decode_mode()


def test_engine_routed_knob_on_the_cpu_decodes_like_the_full_forward(
        monkeypatch):
    """KF_MOE_DECODE=routed off the GPU is the dense path; fp8 stays off for
    an MoE model whose routed fp8 path is not usable."""
    from kubeflow_amd.runtime.serving import InferenceEngine

    monkeypatch.setenv("KF_MOE_DECODE", "routed")
    torch.manual_seed(13)
    eng = InferenceEngine("llama-moe-tiny", device=torch.device("cpu"),
                          max_slots=4, smax=128, max_batch=4, quant="fp8")
    assert eng.quant is False and eng._qw is None
    eng.start(precapture=False)
    try:
        r = eng.generate([5, 3, 8, 1, 9], max_new_tokens=3, timeout=120)
        assert not r.error and len(r.generated) == 3
        with torch.no_grad():
            full = eng.model(torch.tensor([[5, 3, 8, 1, 9]]))
        assert r.generated[0] == int(full[0, -1].argmax())
    finally:
        eng.stop()
