"""InferenceEngine on a head-dim-64 model (llama-tiny-d64, bf16, g = 4, graphs
on): decode and verify logits against an fp32 CPU forward of the same weights,
and chunked prefill (ragged, kf_attn64_cache) against one-at-a-time prefill."""
import pytest
import torch

from kubeflow_amd.models import build_model
from kubeflow_amd.ops import testing as T
from kubeflow_amd.runtime.serving import InferenceEngine, Request

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LENGTHS = [5, 33, 130]


def _engine(monkeypatch, graphs="1"):
    monkeypatch.setenv("KF_SERVE_GRAPH", graphs)
    monkeypatch.setenv("KF_PREFILL_RAGGED", "0")
    torch.manual_seed(0)
    eng = InferenceEngine("llama-tiny-d64", device=DEV, max_slots=8, smax=256,
                          max_batch=4)
    gen = torch.Generator().manual_seed(5)
    V = eng.model.cfg.vocab_size
    return eng, [torch.randint(0, V, (n,), generator=gen).tolist()
                 for n in LENGTHS]


@pytest.mark.parametrize("which", range(len(LENGTHS)))
def test_step_logits_against_fp32_forward(which, monkeypatch):
    eng, prompts = _engine(monkeypatch)
    assert eng.use_graphs
    prompt = prompts[which]
    req = Request(rid="t", prompt=list(prompt), max_new_tokens=8)
    req.slot = eng.cache.alloc()
    eng._prefill(req)
    rows = [req.generated[-1], 7, 9, 11]   # the last token and three drafts
    pos, Tn = req.pos, len(rows)
    ref_model = build_model("llama-tiny-d64", device=torch.device("cpu"),
                            dtype=torch.float32)
    ref_model.load_state_dict(
        {k: v.float().cpu() for k, v in eng.model.state_dict().items()})
    with torch.no_grad():
        ref = ref_model.eval()(torch.tensor([prompt + rows]))[0, pos:]
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
    print(f"PARITY d64 len{len(prompt)} logits verify row_err={e_verify:.5f} "
          f"one-token row_err={e_single:.5f}")
    # the D = 128 tests' bounds: 2e-2 on a step's logits
    # (test_prefill_ragged_gpu.py) and verify at most twice the one-token
    # path's own error plus a floor (test_spec_decode_gpu.py)
    assert e_single < 2e-2, e_single
    assert e_verify <= 2 * e_single + 1e-3, (e_verify, e_single)


def test_graphed_decode_matches_eager(monkeypatch):
    """The captured one-token and verify steps produce the eager tokens."""
    monkeypatch.setenv("KF_SPEC_TOKENS", "3")
    out = []
    for graphs in ("1", "0"):
        eng, prompts = _engine(monkeypatch, graphs)
        assert eng.use_graphs == (graphs == "1")
        reqs = [Request(rid=str(i), prompt=list(p), max_new_tokens=12)
                for i, p in enumerate(prompts[:2])]
        for r in reqs:
            r.rng = torch.Generator().manual_seed(0)
            r.slot = eng.cache.alloc()
            eng._prefill(r)
        eng.active = list(reqs)
        while eng.active:
            eng._decode_step()
        out.append([r.generated for r in reqs])
    assert out[0] == out[1]


def test_chunked_prefill_matches_one_at_a_time(monkeypatch):
    """_prefill_chunk at head_dim 64 goes ragged whatever KF_PREFILL_RAGGED
    says: the cache rows of 48-token chunks agree with whole-prompt prefill,
    and no other cache row changes."""
    eng, prompts = _engine(monkeypatch)
    assert not eng.prefill_ragged
    whole, chunked = ([Request(rid=t, prompt=list(p), max_new_tokens=4)
                       for p in prompts] for t in "wc")
    for r in whole + chunked:
        r.slot = eng.cache.alloc()
    for r in whole:
        eng._prefill(r)
    before = [(k.clone(), v.clone()) for k, v in zip(eng.cache.k, eng.cache.v)]
    for a, b, n in zip(whole, chunked, LENGTHS):
        for pos in range(0, n, 48):
            eng._prefill_chunk(b, b.prompt[pos:pos + 48], pos)
        worst = 0.0
        for li, (k0, v0) in enumerate(before):
            for new, old in ((eng.cache.k[li], k0), (eng.cache.v[li], v0)):
                worst = max(worst, T.row_err(new[b.slot, :n],
                                             old[a.slot, :n]))
                new[b.slot, :n] = old[b.slot, :n]
        print(f"PARITY d64 chunked len{n} cache row_err={worst:.5f}")
        assert worst < 2e-2, (n, worst)
    for li, (k0, v0) in enumerate(before):
        assert torch.equal(eng.cache.k[li], k0)
        assert torch.equal(eng.cache.v[li], v0)
