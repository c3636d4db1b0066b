"""ops.linear_q4 off the GPU, and what InferenceEngine(quant_prefill=True)
refuses; none of it needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

from kubeflow_amd import models, ops
from kubeflow_amd.models import llama
from kubeflow_amd.runtime.serving import InferenceEngine

CPU = torch.device("cpu")


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("M", [1, 40])
def test_linear_q4_cpu_is_linear_on_the_dequantized_weights(M, with_res):
    g = torch.Generator().manual_seed(M)
    w4, sc = ops.quantize_mxfp4_rows(torch.randn(64, 256, generator=g))
    x = torch.randn(M, 256, generator=g)
    res = torch.randn(M, 64, generator=g) if with_res else None
    want = F.linear(x, ops.dequantize_mxfp4_rows(w4, sc, torch.float32))
    if with_res:
        want = want + res
    assert torch.equal(ops.linear_q4(x, w4, sc, res), want)
    with pytest.raises(ValueError):     # _check_mxfp4 runs first
        ops.linear_q4(x[:, :128], w4, sc, res)


def _moe_cfg():
    return llama.LlamaConfig(name="llama-q4-prefill-moe-test", vocab_size=64,
                             hidden_size=128, n_layers=1, n_heads=1,
                             n_kv_heads=1, ffn_dim=128, max_seq_len=64,
                             n_experts=2, top_k=1)


@pytest.mark.parametrize("model,quant,skinny", [
    ("llama-tiny", "fp8", "small"), ("llama-tiny", "off", "small"),
    ("llama-q4-prefill-moe-test", "mxfp4", "small"),
    ("llama-tiny", "mxfp4", "qkv,wo")], ids=["fp8", "off", "moe", "skinny"])
def test_quant_prefill_refuses_what_it_cannot_serve(monkeypatch, model, quant,
                                                    skinny):
    monkeypatch.setitem(models.MODEL_REGISTRY, "llama-q4-prefill-moe-test",
                        models._llama(_moe_cfg))
    monkeypatch.setenv("KF_SKINNY", skinny)
    with pytest.raises(ValueError, match="quant_prefill"):
        InferenceEngine(model, device=CPU, max_slots=2, smax=32, quant=quant,
                        quant_prefill=True)


def test_quant_prefill_engine_on_the_cpu_releases_the_weights():
    torch.manual_seed(3)
    eng = InferenceEngine("llama-tiny", device=CPU, max_slots=2, smax=32,
                          quant="mxfp4", quant_prefill=True)
    torch.manual_seed(3)
    ref = InferenceEngine("llama-tiny", device=CPU, max_slots=2, smax=32,
                          quant="mxfp4")
    freed = sum(getattr(layer, n).weight.numel() * 4
                for layer in ref.model.layers
                for n in ("wqkv", "wo", "w13", "w2"))
    assert freed > 0 and ref.weight_bytes - eng.weight_bytes == freed
    assert all(getattr(layer, n).weight.numel() == 0
               for layer in eng.model.layers
               for n in ("wqkv", "wo", "w13", "w2"))
