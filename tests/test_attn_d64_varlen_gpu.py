"""Head-dim-64 attention with per-sequence lengths (kf_attn64_*_varlen)
through the public op, the model and the serving engine.

Inputs are the seeded bf16 tensors of `attention_case_varlen`; on the GPU copy
the k/v rows past each length hold the finite garbage value of
tests/test_attn_d64_gpu.py (never to be read) and dout is random non-zero
everywhere, padded rows included. The oracle is the fp32 reference.sdpa per
sequence, embedded in zeros. Bounds: the whole-tensor ones of
tests/test_attn_d64_gpu.py (2e-2 forward, 4e-2 gradients) and the per-row
bound of the case (3 x the all-bf16 emulation's per-row error; shown to
separate a one-key defect in tests/test_attn_varlen_cpu.py).

Shapes are the smallest that reach each branch: a length of one key, lengths
inside a 64-row tile, on a tile edge, one past a 128 boundary (a block wholly
skipped and a straddling wave), full length, the GQA head loop, an odd head
count over three blocks with the dK/dV q loop ending mid-sequence, and the
wrapper's pad path.
"""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.ops import testing as T

D = 64
FWD_BOUND = 2e-2  # tests/test_attn_d64_gpu.py
BWD_BOUND = 4e-2
GARBAGE = 1e4     # fills k/v rows >= the length: finite, never to be read
GRAD_BOUND = 4e-2  # tests/test_bert_d64_gpu.py
LOSS_BOUND = 1e-2
NAMES = ("o", "dq", "dk", "dv")

# name -> (B, S, Hq, Hkv, seq_lens)
CASES = {
    "one_key_to_full_gqa": (4, 256, 4, 2, (1, 37, 129, 256)),
    "single_block": (3, 128, 2, 2, (128, 64, 100)),
    "odd_heads_three_blocks": (2, 384, 3, 3, (65, 300)),
    "wrapper_pad": (1, 100, 2, 2, (70,)),
}

_cache = {}


def _dev():
    return torch.device("cuda", 0)


def _inputs(name):
    """The case's (q, k, v, dout) with garbage in the padded k/v rows."""
    B, S, Hq, Hkv, lens = CASES[name]
    q, k, v, dout = (t.clone() for t in
                     T.attention_case_varlen(B, S, Hq, Hkv, lens).inputs)
    for b, L in enumerate(lens):
        k[b, L:] = GARBAGE
        v[b, L:] = GARBAGE
        assert L == S or dout[b, L:].abs().min() > 0
    return q, k, v, dout


def _gpu_run(q, k, v, dout, **mask):
    qg, kg, vg = (t.to(_dev()).requires_grad_(True) for t in (q, k, v))
    o = ops.flash_attention(qg, kg, vg, causal=False, **mask)
    o.backward(dout.to(_dev()))
    torch.cuda.synchronize()
    return o.detach(), qg.grad, kg.grad, vg.grad


def _case(name):
    if name not in _cache:
        lens = CASES[name][4]
        sl = torch.tensor(lens, dtype=torch.int32, device=_dev())
        _cache[name] = _gpu_run(*_inputs(name), seq_lens=sl)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_fwd_bwd_matches_oracle(name):
    B, S, Hq, Hkv, lens = CASES[name]
    c = T.attention_case_varlen(B, S, Hq, Hkv, lens)
    got = dict(zip(NAMES, _case(name)))
    whole = {n: T.rel_err(got[n], c.oracle[n]) for n in NAMES}
    rows = {n: T.row_err(got[n], c.oracle[n]) for n in NAMES}
    print(name, "whole-tensor", whole)
    print(name, "per-row", rows, "bound", c.bound)
    for n in NAMES:
        assert got[n].shape == c.oracle[n].shape
        assert whole[n] < (FWD_BOUND if n == "o" else BWD_BOUND), (n, whole)
        assert rows[n] < c.bound[n], (n, rows, c.bound)


@pytest.mark.parametrize("name", list(CASES))
def test_rows_past_each_length_are_exact_zeros(name):
    lens = CASES[name][4]
    for n, t in zip(NAMES, _case(name)):
        for b, L in enumerate(lens):
            assert torch.equal(t[b, L:], torch.zeros_like(t[b, L:])), (n, b, L)


def test_fused_qkv_views_equal_contiguous():
    """q/k/v as the split views of one [B, S, 3*H*64] buffer are read in
    place; values and gradients equal the contiguous call's bit for bit."""
    name = "single_block"
    B, S, H, _, lens = CASES[name]
    q, k, v, dout = _inputs(name)
    qkv = torch.cat([t.reshape(B, S, H * D) for t in (q, k, v)],
                    dim=-1).to(_dev()).requires_grad_(True)
    qv, kv, vv = (t.view(B, S, H, D) for t in qkv.split(H * D, dim=-1))
    assert not qv.is_contiguous()
    sl = torch.tensor(lens, dtype=torch.int32, device=_dev())
    o = ops.flash_attention(qv, kv, vv, causal=False, seq_lens=sl)
    o.backward(dout.to(_dev()))
    torch.cuda.synchronize()
    want = _case(name)
    assert torch.equal(o.detach(), want[0])
    for g, w in zip(qkv.grad.split(H * D, dim=-1), want[1:]):
        assert torch.equal(g.reshape(B, S, H, D), w)


@pytest.mark.parametrize("L", [37, 129])
def test_uniform_lengths_equal_scalar_kv_len(L):
    """seq_lens = [L] * B runs the loops and masks of kv_len = L: o and dq
    rows < L are the scalar path's bits; dk/dv are when dout is zero past L
    (the scalar path lets padded q rows contribute)."""
    B, S, Hq, Hkv = 2, 256, 4, 2
    q, k, v, dout = (t.clone() for t in T.attention_inputs(B, S, Hq, Hkv, D))
    k[:, L:] = GARBAGE
    v[:, L:] = GARBAGE
    sl = torch.full((B,), L, dtype=torch.int32, device=_dev())
    o_v, dq_v, _, _ = _gpu_run(q, k, v, dout, seq_lens=sl)
    o_s, dq_s, _, _ = _gpu_run(q, k, v, dout, kv_len=L)
    assert torch.equal(o_v[:, :L], o_s[:, :L])
    assert torch.equal(dq_v[:, :L], dq_s[:, :L])
    dout[:, L:] = 0
    _, dq_v, dk_v, dv_v = _gpu_run(q, k, v, dout, seq_lens=sl)
    _, dq_s, dk_s, dv_s = _gpu_run(q, k, v, dout, kv_len=L)
    assert torch.equal(dk_v, dk_s)
    assert torch.equal(dv_v, dv_s)
    assert torch.equal(dq_v[:, :L], dq_s[:, :L])


def test_host_list_and_reference_route_agree(monkeypatch):
    """A Python list is validated and moved; KF_ATTN_D64=0 runs the reference
    math per sequence with the same zero rows."""
    name = "single_block"
    B, S, Hq, Hkv, lens = CASES[name]
    c = T.attention_case_varlen(B, S, Hq, Hkv, lens)
    got = _gpu_run(*_inputs(name), seq_lens=list(lens))
    for a, w in zip(got, _case(name)):
        assert torch.equal(a, w)
    monkeypatch.setenv("KF_ATTN_D64", "0")
    ref = dict(zip(NAMES, _gpu_run(*_inputs(name), seq_lens=list(lens))))
    for n in NAMES:
        assert T.rel_err(ref[n], c.oracle[n]) < \
            (FWD_BOUND if n == "o" else BWD_BOUND), n
        for b, L in enumerate(lens):
            assert not ref[n][b, L:].any(), (n, b)


def test_device_lengths_are_clamped_into_range():
    """A device tensor is not validated on the host; the kernels clamp each
    entry into [1, S] as they read it, so 0, a negative and a too-large value
    behave as 1, 1 and S."""
    B, S, Hq, Hkv = 3, 128, 2, 2
    q, k, v, dout = T.attention_inputs(B, S, Hq, Hkv, D)
    raw = torch.tensor([0, S + 1000, -5], dtype=torch.int32, device=_dev())
    ok = torch.tensor([1, S, 1], dtype=torch.int32, device=_dev())
    for a, w in zip(_gpu_run(q, k, v, dout, seq_lens=raw),
                    _gpu_run(q, k, v, dout, seq_lens=ok)):
        assert torch.equal(a, w)


def test_d128_with_seq_lens_raises():
    q = torch.zeros(2, 128, 2, 128, device=_dev(), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head_dim 64"):
        ops.flash_attention(q, q, q, causal=False, seq_lens=[64, 128])


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _fp(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def _ip(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32))


@pytest.mark.parametrize("S,Hq,Hkv", [(192, 2, 2), (128, 3, 2)])
def test_direct_entry_points_reject_bad_shapes(S, Hq, Hkv):
    """Host-side argument checks of both entry points: hipErrorInvalidValue
    is returned before any launch."""
    from kubeflow_amd.ops import _backend
    lib = _backend.require()
    B = 1
    dev = _dev()
    q = torch.zeros(B, S, Hq, D, device=dev, dtype=torch.bfloat16)
    k = torch.zeros(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
    o, dq = torch.zeros_like(q), torch.zeros_like(q)
    dk, dv = torch.zeros_like(k), torch.zeros_like(k)
    lse = torch.zeros(B, Hq, S, device=dev)
    delta = torch.zeros_like(lse)
    sl = torch.full((B,), 64, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    invalid = 1  # hipErrorInvalidValue
    assert lib.kf_attn64_fwd_varlen(_p(o), _fp(lse), _p(q), _p(k), _p(k),
                                    _ip(sl), B, S, Hq, Hkv, 0, 0, D ** -0.5,
                                    stream) == invalid
    assert lib.kf_attn64_bwd_varlen(_p(dq), _p(dk), _p(dv), _p(o), _p(q),
                                    _p(k), _p(k), _p(o), _fp(lse),
                                    _fp(delta), _ip(sl), B, S, Hq, Hkv, 0, 0,
                                    D ** -0.5, stream) == invalid
    torch.cuda.synchronize()


# ------------------------------------------------------ model and engine ----

def _relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _train_step(model, tokens, targets, seq_lens):
    model.zero_grad(set_to_none=True)
    loss = model(tokens, targets, seq_lens=seq_lens)
    loss.backward()
    torch.cuda.synchronize()
    return (float(loss.detach()),
            {n: p.grad.detach().clone() for n, p in model.named_parameters()})


def test_bert_tiny_train_step_matches_reference_route(monkeypatch):
    """bert-tiny, B = 2, S = 128, seq_lens = [50, 128]: loss and every
    parameter gradient on the native kernels against the KF_ATTN_D64=0
    reference route on the same weights."""
    from kubeflow_amd.models import build_model
    torch.manual_seed(3)
    dev = _dev()
    model = build_model("bert-tiny", device=dev)
    with torch.no_grad():  # zero-init biases: make every path carry signal
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.02 * torch.randn_like(p))
    g = torch.Generator(device="cpu").manual_seed(4)
    tokens = torch.randint(0, model.cfg.vocab_size, (2, 128),
                           generator=g).to(dev)
    targets = torch.randint(0, model.cfg.n_classes, (2,), generator=g).to(dev)

    loss_n, grads_n = _train_step(model, tokens, targets, [50, 128])
    monkeypatch.setenv("KF_ATTN_D64", "0")
    loss_r, grads_r = _train_step(model, tokens, targets, [50, 128])

    print("loss native/reference", loss_n, loss_r)
    assert abs(loss_n - loss_r) < LOSS_BOUND, (loss_n, loss_r)
    errs = {n: _relerr(grads_n[n], grads_r[n]) for n in grads_r}
    print(errs)
    assert any(g.abs().max() > 0 for g in grads_r.values())
    bad = {n: e for n, e in errs.items() if not e < GRAD_BOUND}
    assert not bad, bad


def test_bert_base_engine_batches_mixed_lengths():
    """bert-base through InferenceEngine with prompts of 51 / 90 / 128 tokens
    pending together: one forward, class probabilities within
    tests/test_bert_d64_gpu.py's bound of a CPU fp32 clone run per prompt."""
    from kubeflow_amd.runtime.serving import InferenceEngine, Request

    torch.manual_seed(10)
    eng = InferenceEngine("bert-base", device=_dev(), max_batch=4)
    prompts = [list(range(2, 2 + n)) for n in (51, 90, 128)]
    reqs = [eng.submit(Request(rid=f"r{i}", prompt=p))
            for i, p in enumerate(prompts)]
    eng.start()
    try:
        for r in reqs:
            assert r.done.wait(120) and not r.error, r.error
        assert eng.stats["classify_batches"] == 1, eng.stats
        cpu = copy.deepcopy(eng.model).float().cpu()
        for r, p in zip(reqs, prompts):
            with torch.no_grad():
                want = torch.softmax(cpu(torch.tensor([p]))[0].float(),
                                     dim=-1)
            got = torch.tensor(r.scores)
            assert torch.allclose(got, want, atol=0.05), (len(p), got, want)
    finally:
        eng.stop()


# ------------------------------------------------------------- mask probe

def test_mask_probe_each_sequence_ends_at_its_length():
    """Scores 8 * j (testing.mask_probe_inputs), lengths (1, 63, 64, 65, 200)
    at S = 200: every real row of sequence b is v[b, L_b - 1], dv[b, L_b - 1]
    the sum of the group's real dout rows, and rows past the length exact
    zeros. Per-row FWD_BOUND / BWD_BOUND against the fp32 oracle per sequence
    and against the closed form; a length off by one key gives a per-row
    error above 1 (tests/test_attn_probe_cpu.py)."""
    lens = (1, 63, 64, 65, 200)
    B, S, Hq, Hkv = len(lens), 200, 4, 2
    g = Hq // Hkv
    q, k, v, scale = T.mask_probe_inputs(B, S, S, Hq, Hkv, D, seed=71)
    gen = torch.Generator(device="cpu").manual_seed(72)
    dout = torch.randn(B, S, Hq, D, generator=gen).bfloat16()
    oo, odv = torch.zeros(B, S, Hq, D), torch.zeros(B, S, Hkv, D)
    hot_o, hot_dv = torch.zeros(B, S, Hq, D), torch.zeros(B, S, Hkv, D)
    for b, L in enumerate(lens):
        r = T.attention_oracle(q[b:b + 1, :L], k[b:b + 1, :L], v[b:b + 1, :L],
                               dout[b:b + 1, :L], False, scale)
        oo[b, :L], odv[b, :L] = r[0][0], r[4][0]
        hot_o[b, :L] = v[b, L - 1].float().repeat_interleave(g, dim=0)
        hot_dv[b, L - 1] = dout[b, :L].float().view(L, Hkv, g, D).sum(
            dim=(0, 2))
        k[b, L:] = GARBAGE
        v[b, L:] = GARBAGE
    sl = torch.tensor(lens, dtype=torch.int32, device=_dev())
    o, _, _, dv = _gpu_run(q, k, v, dout, scale=scale, seq_lens=sl)
    errs = dict(o=T.row_err(o, oo), o_hot=T.row_err(o, hot_o),
                dv=T.row_err(dv, odv), dv_hot=T.row_err(dv, hot_dv))
    print(f"PARITY varlen probe o row={errs['o']:.5f} "
          f"row_vs_v={errs['o_hot']:.5f} bound={FWD_BOUND} "
          f"dv row={errs['dv']:.5f} row_vs_dout={errs['dv_hot']:.5f} "
          f"bound={BWD_BOUND}")
    assert errs["o"] < FWD_BOUND and errs["o_hot"] < FWD_BOUND, errs
    assert errs["dv"] < BWD_BOUND and errs["dv_hot"] < BWD_BOUND, errs
    for b, L in enumerate(lens):
        assert not o[b, L:].any() and not dv[b, L:].any(), (b, L)
