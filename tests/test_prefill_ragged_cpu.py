"""InferenceEngine._prefill_ragged on the CPU (llama-tiny, fp32) against
_prefill one request at a time, and the ragged prefill group."""
import pytest
import torch

from kubeflow_amd.ops import testing as T
from kubeflow_amd.runtime.serving import InferenceEngine, Request

LENGTHS = [5, 33, 130]


def _engine(monkeypatch, ragged):
    monkeypatch.setenv("KF_PREFILL_RAGGED", ragged)
    torch.manual_seed(0)
    return InferenceEngine("llama-tiny", device=torch.device("cpu"),
                           max_slots=8, smax=256, max_batch=4)


def _requests(eng):
    gen = torch.Generator().manual_seed(5)
    V = eng.model.cfg.vocab_size
    return [Request(rid=f"r{n}", max_new_tokens=4,
                    prompt=torch.randint(0, V, (n,), generator=gen).tolist())
            for n in LENGTHS]


def test_ragged_prefill_matches_one_at_a_time(monkeypatch):
    """fp32: only the GEMM row grouping differs. Measured on these seeded
    inputs: cache rel_err <= 5.5e-7, logits rel_err <= 5.3e-7 (bound 1e-4)."""
    eng = _engine(monkeypatch, "1")
    seen = []
    monkeypatch.setattr(eng, "_first_tokens", lambda logits, reqs: (
        seen.append(logits.clone()), [0] * len(reqs))[1])
    single, ragged = _requests(eng), _requests(eng)
    for r in single + ragged:
        r.slot = eng.cache.alloc()
    for r in single:
        eng._prefill(r)
    before = [(k.clone(), v.clone()) for k, v in zip(eng.cache.k, eng.cache.v)]
    logits = eng._prefill_ragged(ragged)
    for i, (a, b, n) in enumerate(zip(single, ragged, LENGTHS)):
        err = T.rel_err(logits[i], seen[i][0])
        print(f"PARITY ragged cpu len{n} logits rel_err={err:.2e}")
        assert err < 1e-4, (n, err)
        worst = 0.0
        for li, (k0, v0) in enumerate(before):
            for new, old in ((eng.cache.k[li], k0), (eng.cache.v[li], v0)):
                worst = max(worst, T.rel_err(new[b.slot, :n],
                                             old[a.slot, :n]))
                new[b.slot, :n] = old[b.slot, :n]
        print(f"PARITY ragged cpu len{n} cache rel_err={worst:.2e}")
        assert worst < 1e-4, (n, worst)
    for li, (k0, v0) in enumerate(before):
        assert torch.equal(eng.cache.k[li], k0)
        assert torch.equal(eng.cache.v[li], v0)


def test_prefill_group_takes_mixed_lengths(monkeypatch):
    for ragged, want in (("1", LENGTHS), ("0", [])):
        eng = _engine(monkeypatch, ragged)
        for r in _requests(eng):
            eng.pending.put(r)
        group = eng._take_prefill_group()
        assert [len(r.prompt) for r in group] == want
        assert eng.pending.qsize() == 3 - len(want)
