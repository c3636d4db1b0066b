"""Speculative decoding on the GPU (llama-tiny, bf16): the captured verify
step against the eager one, and the verify step's logits against an fp32 CPU
forward with the one-token step's own error as the yardstick."""
import pytest
import torch

from kubeflow_amd.models import build_model
from kubeflow_amd.ops import testing as T
from kubeflow_amd.runtime.serving import InferenceEngine, Request

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PROMPT = [5, 17, 42, 8, 23, 11, 3, 29] * 3


def _engine(monkeypatch, graphs):
    monkeypatch.setenv("KF_SPEC_TOKENS", "3")
    monkeypatch.setenv("KF_SERVE_GRAPH", graphs)
    torch.manual_seed(0)
    return InferenceEngine("llama-tiny", device=DEV, max_slots=4, smax=256,
                           max_batch=2)


def _generate(monkeypatch, graphs):
    eng = _engine(monkeypatch, graphs)
    reqs = [Request(rid="g", prompt=list(PROMPT), max_new_tokens=20),
            Request(rid="s", prompt=PROMPT[3:], max_new_tokens=20,
                    temperature=0.8, top_k=20, seed=11)]
    for r in reqs:
        r.rng = torch.Generator().manual_seed(r.seed or 0)
        r.slot = eng.cache.alloc()
        eng._prefill(r)
    eng.active = list(reqs)
    while eng.active:
        eng._decode_step()
    return [r.generated for r in reqs], eng


def test_graph_against_eager(monkeypatch):
    """The same kernels in the same order: identical tokens."""
    with_graphs, eng = _generate(monkeypatch, "1")
    assert eng.use_graphs and (2, 4) in eng._graphs
    assert eng.stats["spec_steps"] > 0
    eager, _ = _generate(monkeypatch, "0")
    assert with_graphs == eager


def test_verify_logits_against_fp32_forward(monkeypatch):
    eng = _engine(monkeypatch, "0")
    req = Request(rid="t", prompt=list(PROMPT), max_new_tokens=8)
    req.slot = eng.cache.alloc()
    eng._prefill(req)
    rows = [req.generated[-1], 7, 9, 11]   # the last token and three drafts
    pos, Tn = req.pos, len(rows)
    ref_model = build_model("llama-tiny", device=torch.device("cpu"),
                            dtype=torch.float32)
    ref_model.load_state_dict(
        {k: v.float().cpu() for k, v in eng.model.state_dict().items()})
    with torch.no_grad():
        ref = ref_model.eval()(torch.tensor([PROMPT + rows]))[0, pos:]
    slot = torch.tensor([req.slot], dtype=torch.int32, device=DEV)
    verify = eng._decode_forward(
        torch.tensor(rows, device=DEV).view(Tn, 1),
        pos + torch.arange(Tn, device=DEV), slot.repeat(Tn),
        torch.tensor([pos + 1], dtype=torch.int32, device=DEV), Tn, slot)
    single = torch.cat([eng._decode_forward(
        torch.tensor([[tok]], device=DEV), torch.tensor([pos + t], device=DEV),
        slot, torch.tensor([pos + t + 1], dtype=torch.int32, device=DEV))
        for t, tok in enumerate(rows)])
    e_verify, e_single = T.row_err(verify, ref), T.row_err(single, ref)
    print(f"PARITY spec logits verify row_err={e_verify:.5f} "
          f"one-token row_err={e_single:.5f}")
    # a different summation order in attention and another M-tile in the
    # GEMMs: at most twice the one-token path's own error, plus a floor
    assert e_verify <= 2 * e_single + 1e-3, (e_verify, e_single)
