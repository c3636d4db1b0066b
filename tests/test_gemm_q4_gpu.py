"""kf_gemm_q4 (gemm_q4.hip), the MXFP4 W4A16 GEMM for any number of rows,
ops.linear_q4 and the serving engine with quant_prefill on the GPU.

Inputs as tests/test_mxfp4_gpu.py builds them (block magnitudes 2^-6 .. 2^2
inside every row: a scale from a neighbouring block or row reads about 0.18);
the oracle is the float64 product on the exactly dequantized weights, the
bound the skinny-GEMM per-row 2e-2 (docs/KERNELS.md).

The block tile is 128 x 128, and M and N sit around it: M = 1, 33 (just past
the skinny range), 127 / 128 / 129 (around one M tile),
300 (three tiles, the last partial); N = 32 (one partial N tile), 160 (two
tiles, the second 32 wide). The K step is 64, not 128, but the K loop is
unrolled over the buffer pair and advances 128 k per iteration, which is the
unit K % 128 == 0 leaves: K = 128 is one iteration (both buffers once), 256
two, 384 an odd count, 1152 nine, more than the pipeline is deep.
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


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """Seeded inputs of one (N, K), built once: 300 x rows, a residual, the
    fp4 pair on the device and its float64 values."""
    g = torch.Generator().manual_seed(N * 7 + K)
    mag = torch.exp2(torch.rand(N, K // 32, 1, generator=g) * 8 - 6)
    w = torch.randn(N, K // 32, 32, generator=g) * mag
    w4, sc = ops.quantize_mxfp4_rows(w.reshape(N, K))
    assert int(sc.min()) <= 121 and int(sc.max()) >= 127
    dq = ops.dequantize_mxfp4_rows(w4, sc, torch.float32).double()
    x = (torch.randn(300, K, generator=g) * 0.5).bfloat16()
    res = torch.randn(300, N, generator=g).bfloat16()
    return x.to(DEV), res.to(DEV), w4.to(DEV), sc.to(DEV), dq


def _gemm(out, x, w4, sc, res, M, N, K, lda=0, ldc=0):
    return _backend.require().kf_gemm_q4(
        ops._p(out), ops._p(x), ops._p(w4), ops._p(sc), ops._p(res), M, N, K,
        lda, 0, ldc, ops._stream())


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("M", [1, 33, 127, 128, 129, 300])
@pytest.mark.parametrize("N", [32, 160])
@pytest.mark.parametrize("K", [128, 256, 384, 1152])
def test_gemm_q4_parity(K, N, M, with_res):
    xs, rs, w4, sc, dq = _case(N, K)
    x = xs[:M]
    want = x.double().cpu() @ dq.T
    # out and res share ldc = N + 8: a guard row and 8 guard columns
    out = torch.full((M + 1, N + 8), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    res = None
    if with_res:
        res = torch.zeros_like(out)
        res[:M, :N] = rs[:M]
        want = want + rs[:M].double().cpu()
    assert _gemm(out, x, w4, sc, res, M, N, K, ldc=N + 8) == 0
    err = T.row_err(out[:M, :N], want)
    print(f"gemm_q4 K{K} N{N} M{M} res={with_res}: row_err {err:.3e} "
          "(bound 2e-2)")
    assert err < 2e-2
    assert bool(torch.isnan(out[M]).all())
    assert bool(torch.isnan(out[:, N:]).all())


def test_gemm_q4_reads_and_writes_column_slices():
    N, K, M = 160, 256, 129
    xs, rs, w4, sc, dq = _case(N, K)
    wide = torch.full((M, K + 64), float("nan"), dtype=torch.bfloat16,
                      device=DEV)
    wide[:, 32:32 + K] = xs[:M]
    out = torch.full((M, N + 96), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    assert _gemm(out[:, 64:], wide[:, 32:], w4, sc, None, M, N, K,
                 lda=K + 64, ldc=N + 96) == 0
    want = xs[:M].double().cpu() @ dq.T
    assert T.row_err(out[:, 64:64 + N], want) < 2e-2
    assert bool(torch.isnan(out[:, :64]).all())
    assert bool(torch.isnan(out[:, 64 + N:]).all())


@pytest.mark.parametrize("M,N,K,lda", [
    (0, 32, 128, 0), (1, 32, 64, 0), (1, 32, 192, 0), (1, 16, 128, 0),
    (1, 48, 128, 0), (1, 32, 128, 132)],
    ids=["M0", "K64", "K192", "N16", "N48", "lda"])
def test_gemm_q4_entry_rejects_what_the_kernel_cannot_take(M, N, K, lda):
    x, _, w4, sc, _ = _case(160, 256)
    out = torch.empty(8, 160, dtype=torch.bfloat16, device=DEV)
    assert _gemm(out, x, w4, sc, None, M, N, K, lda=lda) == INVALID


def test_linear_q4_dispatch():
    # up to 32 rows on a skinny shape: the skinny kernel's bits
    xs, rs, w4, sc, _ = _case(32, 1024)
    got = ops.linear_q4(xs[:32], w4, sc, rs[:32])
    assert torch.equal(got, ops.skinny_linear_q4(xs[:32], w4, sc, rs[:32]))
    # 33 rows, 3-D x: the entry point's bits
    x3 = xs[:33].view(3, 11, 1024)
    raw = torch.empty(33, 32, dtype=torch.bfloat16, device=DEV)
    assert _gemm(raw, xs[:33], w4, sc, rs[:33], 33, 32, 1024) == 0
    got = ops.linear_q4(x3, w4, sc, rs[:33].view(3, 11, 32))
    assert got.shape == (3, 11, 32) and torch.equal(got.view(33, 32), raw)
    # K = 96: neither kernel, F.linear on the dequantized weights
    xs, _, w4, sc, dq = _case(32, 96)
    got = ops.linear_q4(xs[:40], w4, sc)
    assert T.row_err(got, xs[:40].double().cpu() @ dq.T) < 2e-2


def _dense_cfg():
    return llama.LlamaConfig(name="llama-q4-prefill-test", vocab_size=512,
                             hidden_size=1024, n_layers=2, n_heads=8,
                             n_kv_heads=2, ffn_dim=1024, max_seq_len=256)


def _serve(eng, mode, prompts):
    """Prefill `prompts` by `mode`, then one eager decode step: (first-token
    logits, first tokens, decode logits)."""
    from kubeflow_amd.runtime.serving import Request

    seen = []
    first = type(eng)._first_tokens
    eng._first_tokens = lambda logits, reqs: (
        seen.append(logits.float().cpu()), first(eng, logits, reqs))[1]
    reqs = [Request(rid=str(i), prompt=p, max_new_tokens=4)
            for i, p in enumerate(prompts)]
    for r in reqs:
        r.slot = eng.cache.alloc()
    if mode == "ragged":
        eng._prefill_ragged(reqs)
    for r in reqs if mode != "ragged" else ():
        if mode == "many":
            eng._prefill_many([r])
        else:   # chunks of 16 rows
            eng.PREFILL_CHUNK = 16
            eng._chunking = {"req": r, "prompt": r.prompt, "pos": 0}
            while eng._chunking is not None:
                eng._advance_chunk()
            assert r.error == ""
    dec = eng._decode_forward(
        tokens=torch.tensor([[r.generated[-1]] for r in reqs], device=DEV),
        positions=torch.tensor([r.pos for r in reqs], device=DEV),
        slots=torch.tensor([r.slot for r in reqs], dtype=torch.int32,
                           device=DEV),
        lens=torch.tensor([r.pos + 1 for r in reqs], dtype=torch.int32,
                          device=DEV))
    return torch.cat(seen), [r.generated[0] for r in reqs], dec


def test_engine_quant_prefill_serves_from_the_fp4_weights(monkeypatch):
    from kubeflow_amd.runtime.serving import InferenceEngine

    monkeypatch.setitem(models.MODEL_REGISTRY, "llama-q4-prefill-test",
                        models._llama(_dense_cfg))
    engs = []
    for knob in (True, False):
        torch.manual_seed(5)
        engs.append(InferenceEngine(
            "llama-q4-prefill-test", device=DEV, max_slots=8, smax=128,
            max_batch=2, quant="mxfp4", quant_prefill=knob))
    eng, ref = engs
    names = ("wqkv", "wo", "w13", "w2")
    freed = 0
    for li, layer in enumerate(ref.model.layers):
        for n in names:
            assert getattr(eng.model.layers[li], n).weight.numel() == 0
            assert torch.equal(eng._qw[li][n][0], ref._qw[li][n][0])
            with torch.no_grad():   # ref: bf16 paths on the dequantized values
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
        print(f"quant_prefill {mode}: first-token logits rel_err {e0:.3e}, "
              f"decode logits {e1:.3e} (bound 2e-2)")
        assert e0 < 2e-2 and e1 < 2e-2
        assert got[1] == want[1]
