"""kf_gemm_q4_grouped (gemm_q4.hip): the grouped wide-M MXFP4 GEMM over device
offsets, ops.grouped_linear_q4 / moe_experts_q4, MoEMLP.prefill_routed and the
serving engine with quant_prefill on an MoE model.

Inputs as tests/test_gemm_q4_gpu.py builds them (block magnitudes 2^-6 .. 2^2);
the oracle is float64 on the exactly dequantized bank, the bound the q4
kernels' per-row 2e-2. Row counts sit around the 128-row tile: empty experts
(leading, in the middle, all but the last), one row, a partial second tile, an
exact tile, three tiles; K is one, an odd number and nine 128-k iterations.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import models, ops
from kubeflow_amd.models import llama
from kubeflow_amd.ops import _backend
from kubeflow_amd.ops import testing as T

DEV = torch.device("cuda", 0)
INVALID = 1     # hipErrorInvalidValue
SPLITS = [[0, 129, 1, 128], [300, 0, 0, 33], [0, 0, 0, 200], [130]]
GUARD = 3       # rows of `out` past offsets[E]


@functools.lru_cache(maxsize=None)
def _bank(E, N, K):
    """A seeded [E * N, K] MXFP4 bank on the device and its float64 values."""
    g = torch.Generator().manual_seed(E * 1000 + N * 7 + K)
    mag = torch.exp2(torch.rand(E * N, K // 32, 1, generator=g) * 8 - 6)
    w = torch.randn(E * N, K // 32, 32, generator=g) * mag
    w4, sc = ops.quantize_mxfp4_rows(w.reshape(E * N, K))
    dq = ops.dequantize_mxfp4_rows(w4, sc, torch.float32).double()
    return w4.to(DEV), sc.to(DEV), dq.view(E, N, K)


def _rows(splits, K, gather):
    """x, a_rows (or None) and the float64 A rows of the permuted buffer."""
    total = sum(splits)
    g = torch.Generator().manual_seed(total + K)
    n_tok = (total + 1) // 2 if gather else total
    x = (torch.randn(n_tok, K, generator=g) * 0.5).bfloat16()
    rows = None
    if gather:  # every token twice, a_nrows < total
        rows = torch.arange(2 * n_tok)[torch.randperm(2 * n_tok, generator=g)]
        rows = (rows[:total] // 2).int()
    ax = x.double() if rows is None else x.double()[rows.long()]
    return x.to(DEV), None if rows is None else rows.to(DEV), ax


def _offsets(splits):
    return torch.tensor([0] + splits, dtype=torch.int32).cumsum(0).int().to(DEV)


def _nan_out(total, n):
    return torch.full((total + GUARD, n), float("nan"), dtype=torch.bfloat16,
                      device=DEV)


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "rows"])
@pytest.mark.parametrize("N", [32, 160])
@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("splits", SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_grouped_parity(splits, K, N, gather):
    E, total = len(splits), sum(splits)
    w4, sc, dq = _bank(E, N, K)
    x, rows, ax = _rows(splits, K, gather)
    out = _nan_out(total, N)
    ops.grouped_linear_q4(x, w4, sc, _offsets(splits), rows, out=out)
    xg = x if rows is None else x[rows.long()]
    lo, worst = 0, 0.0
    for e, m in enumerate(splits):
        if m:
            raw = torch.empty(m, N, dtype=torch.bfloat16, device=DEV)
            assert _backend.require().kf_gemm_q4(
                ops._p(raw), ops._p(xg[lo:lo + m].contiguous()),
                ops._p(w4[e * N:]), ops._p(sc[e * N:]), None, m, N, K, 0, 0,
                0, ops._stream()) == 0
            assert torch.equal(out[lo:lo + m], raw)
            worst = max(worst, T.row_err(out[lo:lo + m],
                                         ax[lo:lo + m] @ dq[e].T))
        lo += m
    print(f"grouped q4 {splits} K{K} N{N} rows={gather}: row_err "
          f"{worst:.3e} (bound 2e-2)")
    assert worst < 2e-2
    assert bool(torch.isnan(out[total:]).all())


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "rows"])
@pytest.mark.parametrize("f", [32, 160])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("splits", SPLITS[:2],
                         ids=lambda s: "-".join(map(str, s)))
def test_grouped_swiglu_parity(splits, K, f, gather):
    E, total = len(splits), sum(splits)
    w4, sc, dq = _bank(E, 2 * f, K)
    x, rows, ax = _rows(splits, K, gather)
    off = _offsets(splits)
    out = _nan_out(total, f)
    ops.grouped_linear_q4(x, w4, sc, off, rows, swiglu=True, out=out)
    unfused = ops.swiglu(ops.grouped_linear_q4(x, w4, sc, off, rows))
    lo, worst, worst_un = 0, 0.0, 0.0
    for e, m in enumerate(splits):
        if m:
            h = ax[lo:lo + m] @ dq[e].T
            want = torch.nn.functional.silu(h[:, :f]) * h[:, f:]
            worst = max(worst, T.row_err(out[lo:lo + m], want))
            worst_un = max(worst_un, T.row_err(unfused[lo:lo + m], want))
        lo += m
    print(f"grouped q4 swiglu {splits} K{K} f{f} rows={gather}: row_err "
          f"fused {worst:.3e}, unfused {worst_un:.3e} (bound 2e-2)")
    assert worst < 2e-2
    assert out.shape == (total + GUARD, f)
    assert bool(torch.isnan(out[total:]).all())


def test_graph_replay_follows_the_offsets_of_the_day():
    N, K = 160, 384
    w4, sc, _ = _bank(4, N, K)
    x, rows, _ = _rows([258], K, True)
    off = _offsets([0, 129, 1, 128])
    out = _nan_out(258, N)
    ops.grouped_linear_q4(x, w4, sc, off, rows, out=out)    # warm-up
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.grouped_linear_q4(x, w4, sc, off, rows, out=out)
    for splits in ([100, 0, 30, 128], [0, 129, 1, 128], [258, 0, 0, 0]):
        off.copy_(_offsets(splits))
        out.fill_(float("nan"))
        graph.replay()
        eager = ops.grouped_linear_q4(x, w4, sc, off, rows)
        assert torch.equal(out[:258], eager), splits
        assert bool(torch.isnan(out[258:]).all())


@pytest.mark.parametrize("E,N,K,swiglu", [
    (4, 32, 64, 0), (4, 32, 192, 0), (4, 48, 128, 0), (4, 96, 128, 1),
    (65, 32, 128, 0)], ids=["K64", "K192", "N48", "f48", "E65"])
def test_grouped_entry_rejects_what_the_kernel_cannot_take(E, N, K, swiglu):
    w4, sc, _ = _bank(65, 96, 256)      # larger than any case reads
    x = torch.zeros(8, 256, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(8, 96, dtype=torch.bfloat16, device=DEV)
    off = torch.zeros(66, dtype=torch.int32, device=DEV)
    assert _backend.require().kf_gemm_q4_grouped(
        ops._p(out), ops._p(x), ops._p(w4), ops._p(sc), ops._i32p(off), None,
        E, 8, 8, N, K, swiglu, ops._stream()) == INVALID


def _moe_cfg(E, layers=1):
    return llama.LlamaConfig(name="llama-q4-moe-test", vocab_size=512,
                             hidden_size=1024, n_layers=layers, n_heads=8,
                             n_kv_heads=2, ffn_dim=1024, max_seq_len=256,
                             n_experts=E, top_k=2)


def _dequantized(moe, q4):
    """Write the dequantized values of q4 into moe's bf16 banks."""
    with torch.no_grad():
        for w, pair in zip((moe.experts_w13, moe.experts_w2), q4):
            w.copy_(ops.dequantize_mxfp4_rows(*pair).view(w.shape))


def test_moe_mlp_routes_any_row_count_from_the_fp4_banks():
    from kubeflow_amd.runtime.serving import quantize_moe_banks

    torch.manual_seed(3)
    ref = llama.MoEMLP(_moe_cfg(4)).to(DEV, torch.bfloat16)
    for p in ref.parameters():
        torch.nn.init.normal_(p, std=0.03)
    q4 = quantize_moe_banks(ref, "mxfp4")
    _dequantized(ref, q4)
    moe = llama.MoEMLP(_moe_cfg(4)).to(DEV, torch.bfloat16)
    with torch.no_grad():
        moe.gate.weight.copy_(ref.gate.weight)
        moe.experts_w13.fill_(float("nan"))     # must not be read
        moe.experts_w2.fill_(float("nan"))
    x = torch.randn(240, 1, 1024, device=DEV).bfloat16()
    with torch.no_grad():
        for name, got, xs in (
                ("prefill_routed", moe.prefill_routed(x[:200], q4), x[:200]),
                ("decode_routed", moe.decode_routed(x[200:], q4=q4),
                 x[200:])):
            err = T.row_err(got.view(-1, 1024),
                            ref(xs).view(-1, 1024).double().cpu())
            print(f"MoEMLP.{name} {xs.shape[0]} rows: row_err {err:.3e} "
                  "(bound 2e-2)")
            assert err < 2e-2


def test_engine_quant_prefill_serves_an_moe_model_from_the_fp4_banks(
        monkeypatch):
    from kubeflow_amd.runtime.serving import InferenceEngine
    from test_gemm_q4_gpu import _serve

    monkeypatch.setitem(models.MODEL_REGISTRY, "llama-q4-moe-test",
                        models._llama(lambda: _moe_cfg(2, layers=2)))
    engs = []
    for knob in (True, False):
        torch.manual_seed(5)
        engs.append(InferenceEngine(
            "llama-q4-moe-test", device=DEV, max_slots=8, smax=128,
            max_batch=2, quant="mxfp4", quant_prefill=knob))
    eng, ref = engs
    freed = 0
    for li, layer in enumerate(ref.model.layers):
        got = eng.model.layers[li]
        assert got.moe.experts_w13.numel() == 0
        assert got.moe.experts_w2.numel() == 0
        _dequantized(layer.moe, ref._qw[li]["moe"])
        freed += 2 * (layer.moe.experts_w13.numel()
                      + layer.moe.experts_w2.numel())
        for n in ("wqkv", "wo"):
            assert getattr(got, n).weight.numel() == 0
            with torch.no_grad():
                getattr(layer, n).weight.copy_(
                    ops.dequantize_mxfp4_rows(*ref._qw[li][n]))
            freed += getattr(layer, n).weight.numel() * 2
    assert ref.weight_bytes - eng.weight_bytes == freed
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, 512, (n,), generator=g).tolist()
               for n in (40, 5)]
    for mode in ("many", "ragged", "chunked"):
        got, want = _serve(eng, mode, prompts), _serve(ref, mode, prompts)
        e0, e1 = T.rel_err(got[0], want[0]), T.rel_err(got[2], want[2])
        print(f"moe quant_prefill {mode}: first-token logits rel_err "
              f"{e0:.3e}, decode logits {e1:.3e} (bound 2e-2)")
        assert e0 < 2e-2 and e1 < 2e-2
        assert got[1] == want[1]
