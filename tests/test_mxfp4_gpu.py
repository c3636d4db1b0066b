"""The MXFP4 (W4A16) skinny GEMMs on the GPU: kf_skinny_gemm_q4 and its
grouped form (skinny_gemm.hip), ops.moe_experts_decode on fp4 banks and the
serving engine with quant="mxfp4".

dequantize_mxfp4_rows is exact in bf16, so the kernel computes the product of
x and the dequantized weights with an fp32 accumulation and one bf16 store:
the oracle is that product in float64, the bound the skinny-GEMM per-row one
(2e-2, docs/KERNELS.md), and anything above bf16 rounding is a decode, index
or scale bug. Block magnitudes spread over 2^-6 .. 2^2 within every row, so a
scale taken from a neighbouring block or row reads about 0.18.

Shapes: K = 1024 (one staged chunk), 2048 (both LDS buffers, the second
staging register), 3072 (odd count: the unrolled-by-two loop ends on its first
half); N = 16 and 48 (one and three blocks); M = 1, 16, 17, 32 (both M-tile
templates and their row guards).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import models, ops
from kubeflow_amd.models import llama
from kubeflow_amd.ops import _backend
from kubeflow_amd.ops import testing as T

DEV = torch.device("cuda", 0)
E4 = 4


def _case(N, K):
    """Seeded inputs of one (N, K), fresh for every test (milliseconds at
    these sizes): 64 x rows, a residual, the fp4 pair of E4 * N weight rows
    on the device and its float64 values."""
    g = torch.Generator().manual_seed(N * 7 + K)
    mag = torch.exp2(torch.rand(E4 * N, K // 32, 1, generator=g) * 8 - 6)
    w = (torch.randn(E4 * N, K // 32, 32, generator=g) * mag)
    w4, sc = ops.quantize_mxfp4_rows(w.reshape(E4 * N, K))
    assert int(sc.min()) <= 121 and int(sc.max()) >= 127
    dq = ops.dequantize_mxfp4_rows(w4, sc, torch.float32).double()
    x = (torch.randn(64, K, generator=g) * 0.5).bfloat16()
    res = torch.randn(64, N, generator=g).bfloat16()
    return x.to(DEV), res.to(DEV), w4.to(DEV), sc.to(DEV), dq


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("M", [1, 16, 17, 32])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [1024, 2048, 3072])
def test_q4_parity(K, N, M, with_res):
    lib = _backend.require()
    xs, rs, w4, sc, dq = _case(N, K)
    x, w4, sc, dq = xs[:M], w4[:N], sc[:N], dq[:N]
    res = rs[:M] if with_res else None
    want = x.double().cpu() @ dq.T
    if with_res:
        want = want + res.double().cpu()
    # the entry point itself, into a NaN-filled buffer with a guard row
    out = torch.full((M + 1, N), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    _backend.check(lib.kf_skinny_gemm_q4(
        ops._p(out), ops._p(x), ops._p(w4), ops._p(sc), ops._p(res), M, N, K,
        0, 0, 0, ops._stream()), "skinny_gemm_q4")
    err = T.row_err(out[:M], want)
    print(f"q4 K{K} N{N} M{M} res={with_res}: row_err {err:.3e} (bound 2e-2)")
    assert err < 2e-2
    assert bool(torch.isnan(out[M]).all())
    got = ops.skinny_linear_q4(x.view(M, 1, K), w4, sc,
                               None if res is None else res.view(M, 1, N))
    assert got.shape == (M, 1, N) and torch.equal(got.view(M, N), out[:M])


def test_q4_entry_rejects_what_the_kernel_cannot_take():
    lib = _backend.require()
    x, _, w4, sc, _ = _case(16, 1024)
    out = torch.empty(33, 16, dtype=torch.bfloat16, device=DEV)
    for M, N, K, lda in ((0, 16, 1024, 0), (33, 16, 1024, 0),
                         (1, 16, 512, 0), (1, 24, 1024, 0), (1, 16, 1024, 1028)):
        assert lib.kf_skinny_gemm_q4(
            ops._p(out), ops._p(x), ops._p(w4), ops._p(sc), None, M, N, K,
            lda, 0, 0, ops._stream()) == 1      # hipErrorInvalidValue


@pytest.mark.parametrize("use_rows", [False, True], ids=["inplace", "rows"])
@pytest.mark.parametrize("Tn", [4, 32])
def test_grouped_q4_is_the_plain_kernel_per_expert(Tn, use_rows):
    N, K = 48, 2048
    xs, _, w4, sc, dq = _case(N, K)
    counts = (0, Tn, 1, Tn - 1)
    off = [0, 0, Tn, Tn + 1, 2 * Tn]
    total = off[-1]
    offsets = torch.tensor(off, dtype=torch.int32, device=DEV)
    rows = None
    if use_rows:   # token rows with repeats, as MoeRouting.src has
        rows = torch.randint(0, 9, (total,), dtype=torch.int32,
                             generator=torch.Generator().manual_seed(Tn)
                             ).to(DEV)
    x = xs[:total] if rows is None else xs[:9]
    out = torch.full((total + 3, N), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    got = ops.grouped_skinny_linear_q4(x, w4, sc, offsets, Tn, rows, out=out)
    assert got is out
    want = torch.zeros(total, N, dtype=torch.float64)
    for e in range(E4):
        lo, m = off[e], counts[e]
        if m == 0:
            continue
        xr = x[lo:lo + m] if rows is None else x[rows[lo:lo + m].long()]
        ref = ops.skinny_linear_q4(xr, w4[e * N:(e + 1) * N],
                                   sc[e * N:(e + 1) * N])
        assert torch.equal(out[lo:lo + m], ref), e
        want[lo:lo + m] = xr.double().cpu() @ dq[e * N:(e + 1) * N].T
    assert T.row_err(out[:total], want) < 2e-2
    assert bool(torch.isnan(out[total:]).all())     # rows past the last offset
    # an expert without rows writes nothing: with every expert empty the
    # buffer keeps its NaNs
    out.fill_(float("nan"))
    ops.grouped_skinny_linear_q4(x, w4, sc, torch.zeros_like(offsets), Tn,
                                 rows, out=out)
    assert bool(torch.isnan(out).all())


def _moe_cfg():
    return llama.LlamaConfig(name="llama-moe-q4-test", vocab_size=512,
                             hidden_size=1024, n_layers=1, n_heads=8,
                             n_kv_heads=2, ffn_dim=1024, max_seq_len=256,
                             n_experts=4, top_k=2)


def test_decode_routed_fp4_banks_match_the_dequantized_module():
    """The fp8 sibling's check (tests/test_moe_decode_gpu.py) and bound."""
    from kubeflow_amd.runtime.serving import quantize_moe_banks

    g = torch.Generator().manual_seed(31)
    moe = llama.MoEMLP(_moe_cfg())
    with torch.no_grad():
        for p in moe.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.03)
    moe = moe.to(device=DEV, dtype=torch.bfloat16)
    x = torch.randn(8, 1, 1024, generator=g).bfloat16().to(DEV)
    assert moe.routed_decode_ok(x, q4=True)
    q4 = quantize_moe_banks(moe, "mxfp4")
    (w13_4, s13), (w2_4, s2) = q4
    assert w13_4.shape == (4 * 2048, 512) and s13.shape == (4 * 2048, 32)
    with torch.no_grad():
        got = moe.decode_routed(x, q4=q4)
        moe.experts_w13.copy_(ops.dequantize_mxfp4_rows(w13_4, s13).view(
            moe.experts_w13.shape))
        moe.experts_w2.copy_(ops.dequantize_mxfp4_rows(w2_4, s2).view(
            moe.experts_w2.shape))
        want = moe.decode_routed(x)
    err = T.rel_err(got, want)
    print(f"decode_routed fp4 vs dequantized bf16: rel_err {err:.3e}")
    assert err < 2e-2


def test_engine_mxfp4_graph_replays_equal_the_eager_step(monkeypatch):
    """h = f = 1024, so wqkv, wo and both expert banks run the fp4 kernels;
    three replays of the captured decode step give the eager step's bits."""
    from kubeflow_amd.runtime.serving import InferenceEngine, Request

    monkeypatch.setitem(models.MODEL_REGISTRY, "llama-moe-q4-test",
                        models._llama(_moe_cfg))
    monkeypatch.setenv("KF_MOE_DECODE", "routed")
    torch.manual_seed(5)
    eng = InferenceEngine("llama-moe-q4-test", device=DEV, max_slots=4,
                          smax=128, max_batch=2, quant="mxfp4")
    assert eng.quant is True and eng.quant_format == "mxfp4"
    assert set(eng._qw[0]) == {"wqkv", "wo", "moe"}
    assert eng._qw[0]["moe"][1][1].shape == (4 * 1024, 32)
    reqs = [Request(rid=str(i), prompt=p, max_new_tokens=4)
            for i, p in enumerate(([3, 14, 15, 9, 2], [6, 1, 2]))]
    for r in reqs:
        r.slot = eng.cache.alloc()
        eng._prefill(r)
    step = {
        "tokens": torch.tensor([[r.generated[-1]] for r in reqs], device=DEV),
        "positions": torch.tensor([r.pos for r in reqs], device=DEV),
        "slots": torch.tensor([r.slot for r in reqs], dtype=torch.int32,
                              device=DEV),
        "lens": torch.tensor([r.pos + 1 for r in reqs], dtype=torch.int32,
                             device=DEV)}
    eager = eng._decode_forward(**step).clone()
    assert bool(torch.isfinite(eager).all())
    graph, static = eng._graph_for(2)
    for name, t in step.items():
        static[name].copy_(t)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static["logits"], eager)
