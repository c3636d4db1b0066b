"""Speculative decoding in the serving engine (KF_SPEC_TOKENS), llama-tiny on
the CPU in fp32."""
import pytest
import torch

from kubeflow_amd.runtime.serving import (InferenceEngine, Request,
                                          draft_tokens)

BLOCK = [5, 17, 42, 8, 23, 11, 3, 29]
PROMPT = BLOCK * 3          # a repeated block, so prompt lookup finds drafts
SEED = 0                    # of the weights; see test_same_tokens_as_off
GREEDY = dict(max_new_tokens=24)
SAMPLED = dict(max_new_tokens=24, temperature=0.8, top_k=20, seed=11)


@pytest.mark.parametrize("history,want", [
    # the suffix [7, 8, 9] occurred at 1..3; what followed it
    ([1, 7, 8, 9, 4, 5, 6, 2, 7, 8, 9], [4, 5, 6]),
    # no token of the suffix occurs earlier
    ([1, 2, 3, 4], [0, 0, 0]),
    # a match two tokens before the end: two followers, the rest carries 0
    ([1, 2, 3, 9, 3], [9, 3, 0]),
])
def test_draft_tokens(history, want):
    assert draft_tokens(history, 3) == want


def _margin(logits, req):
    """How far the non-speculative engine's next token is from flipping: the
    top-two logit gap (greedy), or the distance of the draw from the chosen
    token's cumulative-mass edges (reference.sample's order: by index)."""
    if req.temperature <= 0:
        top = logits.topk(2).values
        return float(top[0] - top[1])
    kth = logits.topk(req.top_k).values[-1]
    w = torch.where(logits >= kth,
                    torch.exp((logits - logits.max()) / req.temperature),
                    torch.zeros(()))
    c = w.cumsum(0) / w.sum()
    u = req.next_u()
    tok = int((c <= u).sum())
    return min(float(c[tok]) - u, u - (float(c[tok - 1]) if tok else 0.0))


def _generate(monkeypatch, k, kw, smax=256, guard=False, prompt=PROMPT):
    """(tokens, engine steps, stats, smallest margin) of one request driven
    step by step on a fresh engine with KF_SPEC_TOKENS=k."""
    monkeypatch.setenv("KF_SPEC_TOKENS", str(k))
    torch.manual_seed(SEED)
    eng = InferenceEngine("llama-tiny", device=torch.device("cpu"),
                          max_slots=2, smax=smax, max_batch=2)
    req = Request(rid="t", prompt=list(prompt), **kw)
    req.rng = torch.Generator().manual_seed(req.seed or 0)
    req.slot = eng.cache.alloc()
    eng._prefill(req)
    eng.active = [req]
    steps, margin = 0, float("inf")
    while eng.active:
        if guard:  # the step's own logits (it rewrites the same cache row)
            logits = eng._decode_forward(
                torch.tensor([[req.generated[-1]]]), torch.tensor([req.pos]),
                torch.tensor([req.slot], dtype=torch.int32),
                torch.tensor([req.pos + 1], dtype=torch.int32))
            margin = min(margin, _margin(logits[0], req))
        eng._decode_step()
        steps += 1
    return req.generated, steps, eng.stats, margin


@pytest.mark.parametrize("kw", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_same_tokens_as_off(kw, monkeypatch):
    off, off_steps, _, margin = _generate(monkeypatch, 0, kw, guard=True)
    # precondition, from the non-speculative engine alone: no step is a
    # near-tie that another GEMM row count could flip (SEED is chosen so)
    assert margin > 1e-4, margin
    assert off_steps == len(off) - 1          # one token per step + prefill's
    on, on_steps, stats, _ = _generate(monkeypatch, 3, kw)
    assert on == off
    assert stats["spec_steps"] == on_steps
    assert stats["spec_proposed"] == 3 * on_steps
    if kw is GREEDY:   # sampled tokens of random weights match no draft
        assert stats["spec_accepted"] > 0
        assert on_steps < len(on) - 1


def test_stops_at_max_new_tokens_inside_an_accepted_run(monkeypatch):
    full, _, _, _ = _generate(monkeypatch, 0, GREEDY)
    for n in range(2, 12):
        got, _, _, _ = _generate(monkeypatch, 3, dict(max_new_tokens=n))
        assert got == full[:n], n


def test_falls_back_to_one_token_step_near_smax(monkeypatch):
    """pos + T > smax: no verify step, and the same tokens up to the cache's
    end as with the engine off."""
    smax, kw = len(PROMPT) + 3, dict(max_new_tokens=2)  # keeps the prompt
    off, _, _, _ = _generate(monkeypatch, 0, kw, smax=smax)
    on, steps, stats, _ = _generate(monkeypatch, 3, kw, smax=smax)
    assert on == off and len(on) == 2
    assert stats["spec_steps"] == 0 and steps == 1
    # one more row of cache and the same request takes the verify step
    _, _, stats, _ = _generate(monkeypatch, 3, kw, smax=smax + 1)
    assert stats["spec_steps"] == 1
