"""Per-sequence lengths (`seq_lens`) on the CPU: the public op's reference
route, the `attention_case_varlen` helper behind the GPU tests, BERT with one
length per row, the worker's `var_len` batches and the serving engine's
length-bucket batching. No kernel runs here.

The per-row bounds of the GPU cases are checked the way
tests/test_parity_metric_cpu.py checks the others: the all-bf16 emulation
stays within them and a one-key defect does not. The defect is an oracle in
which ONE sequence (the longest one that is shorter than S, where one key
weighs least) attends one extra key, row L. Measured here for the three
S % 128 == 0 GPU cases: emulation per-row 0.008-0.011 (bounds 0.025-0.034),
whole-tensor 0.004-0.005 against the project's 2e-2 / 4e-2; the defect reads
0.59-1.87 per row and only 0.045-0.083 whole-tensor, which is why the per-row
metric is the one that matters. (The S = 100 case: emulation 0.007-0.009,
defect 0.66-1.34 per row.)
"""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import testing as T

FWD_BOUND = 2e-2  # tests/test_ops_gpu.py::test_attention_fwd
BWD_BOUND = 4e-2  # tests/test_ops_gpu.py::test_attention_bwd
NAMES = ("o", "dq", "dk", "dv")

# the cases of tests/test_attn_d64_varlen_gpu.py: (B, S, Hq, Hkv, seq_lens)
GPU_CASES = {
    "one_key_to_full_gqa": (4, 256, 4, 2, (1, 37, 129, 256)),
    "single_block": (3, 128, 2, 2, (128, 64, 100)),
    "odd_heads_three_blocks": (2, 384, 3, 3, (65, 300)),
    "wrapper_pad": (1, 100, 2, 2, (70,)),
}


def _masked_softmax_attention(q, k, v, dout, lens):
    """Hand-built fp32 reference: one [S, S] score matrix per (b, head), keys
    >= L at -inf, query rows >= L zeroed after the softmax. Returns
    (o, dq, dk, dv)."""
    B, S, Hq, D = q.shape
    g = Hq // k.shape[2]
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qr,
                     kr.repeat_interleave(g, dim=2)) * D ** -0.5
    live = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]   # [B, S]
    s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1) * live[:, None, :, None]
    o = torch.einsum("bhqk,bkhd->bqhd", p, vr.repeat_interleave(g, dim=2))
    o.backward(dout.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


def _run_op(q, k, v, dout, seq_lens):
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ops.flash_attention(qr, kr, vr, causal=False, seq_lens=seq_lens)
    o.backward(dout)
    return o.detach(), qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("D", [64, 128])
def test_seq_lens_matches_masked_softmax(D):
    B, S, Hq, Hkv, lens = 3, 48, 4, 2, (1, 48, 19)
    q, k, v, dout = (t.float() for t in T.attention_inputs(B, S, Hq, Hkv, D))
    got = _run_op(q, k, v, dout, list(lens))
    want = _masked_softmax_attention(q, k, v, dout, lens)
    for n, a, w in zip(NAMES, got, want):
        assert torch.allclose(a, w, atol=2e-5, rtol=1e-4), \
            (n, (a - w).abs().max())


@pytest.mark.parametrize("as_tensor", [False, True])
def test_rows_past_each_length_are_exact_zeros(as_tensor):
    B, S, Hq, Hkv, lens = 3, 40, 2, 1, (7, 40, 23)
    q, k, v, dout = (t.float() for t in T.attention_inputs(B, S, Hq, Hkv, 64))
    assert all(dout[b, L:].abs().min() > 0 for b, L in enumerate(lens)
               if L < S)  # non-zero dout in the padded rows
    sl = torch.tensor(lens, dtype=torch.int32) if as_tensor else list(lens)
    got = _run_op(q, k, v, dout, sl)
    for n, t in zip(NAMES, got):
        for b, L in enumerate(lens):
            assert torch.equal(t[b, L:], torch.zeros_like(t[b, L:])), (n, b)
            assert t[b, :L].abs().max() > 0, (n, b)


def test_seq_lens_argument_errors():
    q = torch.zeros(2, 16, 2, 64)
    with pytest.raises(ValueError, match="non-causal"):
        ops.flash_attention(q, q, q, causal=True, seq_lens=[3, 4])
    with pytest.raises(ValueError, match="not both"):
        ops.flash_attention(q, q, q, causal=False, kv_len=8, seq_lens=[3, 4])
    for bad in ([0, 4], [3, 17], [-1, 2]):
        with pytest.raises(ValueError, match=r"\[1, 16\]"):
            ops.flash_attention(q, q, q, causal=False,
                                seq_lens=torch.tensor(bad))
    with pytest.raises(ValueError, match="seq_lens"):
        ops.flash_attention(q, q, q, causal=False, seq_lens=[3, 4, 5])
    with pytest.raises(ValueError, match="seq_lens"):
        ops.flash_attention(q, q, q, causal=False, seq_lens=[3.0, 4.0])


# ------------------------------------------------ attention_case_varlen ----

def _extra_key(name):
    """fp32 oracle outputs where one sequence — the longest with L < S —
    attends key/value row L as well (its queries stay [0, L)); everything
    else is the case's oracle."""
    B, S, Hq, Hkv, lens = GPU_CASES[name]
    c = T.attention_case_varlen(B, S, Hq, Hkv, lens)
    q, k, v, dout = c.inputs
    b = max((L, i) for i, L in enumerate(lens) if L < S)[1]
    L = lens[b]
    qr, kr, vr = (t[b:b + 1].float().clone().requires_grad_(True)
                  for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qr[:, :L],
                     kr[:, :L + 1].repeat_interleave(Hq // Hkv, dim=2)
                     ) * 64 ** -0.5
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1),
                     vr[:, :L + 1].repeat_interleave(Hq // Hkv, dim=2))
    o.backward(dout[b:b + 1, :L].float())
    out = {n: c.oracle[n].clone() for n in NAMES}
    out["o"][b, :L] = o.detach()[0]
    out["dq"][b], out["dk"][b], out["dv"][b] = qr.grad[0], kr.grad[0], \
        vr.grad[0]
    return out


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_case_varlen_bounds_and_zero_rows(name):
    B, S, Hq, Hkv, lens = GPU_CASES[name]
    c = T.attention_case_varlen(B, S, Hq, Hkv, lens)
    assert c is T.attention_case_varlen(B, S, Hq, Hkv, lens)  # computed once
    print(name, "emulated per-row", c.emu_err, "bound", c.bound)
    for n in NAMES:
        assert c.oracle[n].shape[:2] == (B, S)
        assert 0 < c.emu_err[n] < c.bound[n] < float("inf")
        assert c.bound[n] == 3 * c.emu_err[n]
        assert c.emu_err[n] < 0.02, (n, c.emu_err)  # all-bf16 per-row ~0.01
        for b, L in enumerate(lens):
            assert not c.oracle[n][b, L:].any(), (n, b)
    # the embedded oracle is the hand-built masked softmax
    want = _masked_softmax_attention(*c.inputs, lens)
    for n, w in zip(NAMES, want):
        assert torch.allclose(c.oracle[n], w, atol=2e-5, rtol=1e-4), n


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_extra_key_fails_per_row_bound(name):
    B, S, Hq, Hkv, lens = GPU_CASES[name]
    c, m = T.attention_case_varlen(B, S, Hq, Hkv, lens), _extra_key(name)
    for n in NAMES:
        err = T.row_err(m[n], c.oracle[n])
        print(name, n, "row_err", err, "bound", c.bound[n], "whole-tensor",
              T.rel_err(m[n], c.oracle[n]))
        assert err > c.bound[n], (n, err, c.bound[n])


def test_case_varlen_emulation_within_whole_tensor_bounds():
    for name, (B, S, Hq, Hkv, lens) in GPU_CASES.items():
        q, k, v, dout = T.attention_inputs(B, S, Hq, Hkv, 64)
        c = T.attention_case_varlen(B, S, Hq, Hkv, lens)
        emu = T._embed_varlen(T.emulated, (q, k, v, dout), lens)
        for n in NAMES:
            e = T.rel_err(emu[n], c.oracle[n])
            print(name, n, "emulated whole-tensor", e)
            assert e < (FWD_BOUND if n == "o" else BWD_BOUND) / 2


# ----------------------------------------------------------------- BERT ----

def _tiny():
    from kubeflow_amd.models import build_model
    torch.manual_seed(5)
    model = build_model("bert-tiny", dtype=torch.float32)
    with torch.no_grad():  # zero-init biases: make every path carry signal
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.02 * torch.randn_like(p))
    return model.eval()


def test_bert_rows_equal_their_unpadded_forward():
    model = _tiny()
    lens = [50, 128, 7]
    g = torch.Generator().manual_seed(6)
    tokens = torch.randint(1, model.cfg.vocab_size, (3, 128), generator=g)
    for b, L in enumerate(lens):
        tokens[b, L:] = 0
    with torch.no_grad():
        alone = torch.cat([model(tokens[b:b + 1, :L])
                           for b, L in enumerate(lens)])
        got = model(tokens, seq_lens=lens)
        assert torch.allclose(got, alone, atol=1e-5), (got, alone)
        # the padding is visible without the lengths
        assert not torch.allclose(model(tokens), alone, atol=1e-5)
        # the same through pad_token_id, lengths derived from the tokens
        assert model.cfg.pad_token_id is None
        model.cfg.pad_token_id = 0
        assert torch.allclose(model(tokens), alone, atol=1e-5)
    with pytest.raises(ValueError, match="seq_lens"):
        model(tokens, seq_lens=[50, 129, 7])


def test_bert_seq_lens_trains():
    model = _tiny().train()
    tokens = torch.randint(1, model.cfg.vocab_size, (2, 64),
                           generator=torch.Generator().manual_seed(7))
    loss = model(tokens, torch.tensor([0, 1]), seq_lens=[9, 64])
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())


# --------------------------------------------------------------- worker ----

def test_synthetic_batch_var_len():
    from kubeflow_amd.models.bert import bert_tiny
    from kubeflow_amd.runtime.worker import synthetic_batch
    cfg = bert_tiny()
    spec = {"task": "classify", "micro_batch": 16, "seq_len": 64,
            "var_len": True, "seed": 3}
    dev = torch.device("cpu")
    x, y = synthetic_batch(spec, cfg, dev, rank=1, step=5)
    x2, y2 = synthetic_batch(spec, cfg, dev, rank=1, step=5)
    assert torch.equal(x, x2) and torch.equal(y, y2)
    assert not torch.equal(x, synthetic_batch(spec, cfg, dev, 1, 6)[0])
    assert not torch.equal(x, synthetic_batch(spec, cfg, dev, 2, 5)[0])
    assert x.shape == (16, 64) and y.shape == (16,)
    lens = (x != 0).sum(1)
    assert lens.min() >= 1 and lens.max() <= 64 and len(set(lens.tolist())) > 1
    for row, L in zip(x, lens.tolist()):  # right-padded with id 0
        assert (row[:L] > 0).all() and (row[:L] < cfg.vocab_size).all()
        assert not row[L:].any()
    # without the key: today's batches, id 0 is an ordinary token
    spec.pop("var_len")
    assert synthetic_batch(spec, cfg, dev, 1, 5)[0].shape == (16, 64)


# --------------------------------------------------------------- engine ----

def test_engine_batches_one_length_bucket_in_one_forward():
    from kubeflow_amd.runtime.serving import InferenceEngine, Request

    torch.manual_seed(9)
    eng = InferenceEngine("bert-tiny", device=torch.device("cpu"),
                          max_batch=4)
    assert eng.classify and eng.stats["classify_batches"] == 0
    prompts = [list(range(3, 40)), list(range(4, 41)), list(range(2, 70)),
               list(range(1, 20))]
    assert [len(p) for p in prompts] == [37, 37, 68, 19]
    reqs = [eng.submit(Request(rid=f"r{i}", prompt=p))
            for i, p in enumerate(prompts)]  # all pending before the thread
    eng.start()
    try:
        for r in reqs:
            assert r.done.wait(60) and not r.error, r.error
        assert eng.stats["classify_batches"] == 1, eng.stats
        assert eng.stats["completed"] == 4
        for r, p in zip(reqs, prompts):
            with torch.no_grad():
                want = torch.softmax(eng.model(torch.tensor([p]))[0].float(),
                                     dim=-1)
            assert torch.allclose(torch.tensor(r.scores), want, atol=1e-4), \
                (len(p), r.scores, want)
    finally:
        eng.stop()
