"""Fused dK/dV backward pass and the RoPE adjoint folded into the dq/dk store
epilogues (attention_bwd8.hip).

Every case checks two things on seeded bf16 randn inputs (D = 128):
  * the new entry points give exactly (torch.equal) what the split
    dv8 + dk8 pair gives, and for the RoPE case what "kf_attn_bwd, then
    kf_rope(backward=1)" gives — the fused kernel keeps the split kernels'
    summation order and the epilogue rotation performs the same two bf16
    roundings as the separate pass;
  * dq, dk, dv stay within test_attention_bwd's bound (rel. error < 4e-2)
    of the fp32 oracle in ops/reference.py.
Shapes are the smallest that reach every branch of the kernels.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.ops import reference as R

D = 128
BOUND = 4e-2  # test_attention_bwd's bound

# name -> (B, S, Hq, Hkv, causal)
PLAIN_CASES = {
    # diagonal sub-blocks only; g = 2 head loop
    "causal_one_kv_block": (1, 256, 4, 2, True),
    # unmasked + diagonal + skipped sub-blocks; g = 4; batch stride;
    # kt-major block decode
    "causal_two_kv_blocks": (2, 512, 4, 1, True),
    # g = 1; no mask path
    "non_causal": (1, 512, 2, 2, False),
}
ROPE_CASE = (2, 512, 4, 2)  # strided fused-qkv + RoPE, causal
ROPE_TABLE_LEN = 640        # cos/sin table longer than S

_cache = {}


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _fp(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def _null_i64():
    return ctypes.cast(0, ctypes.POINTER(ctypes.c_int64))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ok(err, name):
    assert err == 0, f"{name} failed with hipError_t={err}"


def _plain(name):
    """Run one contiguous-bshd case once: split path, new paths, oracle."""
    if name in _cache:
        return _cache[name]
    from kubeflow_amd.ops import _backend
    lib = _backend.require()
    B, S, Hq, Hkv, causal = PLAIN_CASES[name]
    dev = torch.device("cuda", 0)
    scale = D ** -0.5
    g = torch.Generator(device="cpu").manual_seed(1234)
    q = torch.randn(B, S, Hq, D, generator=g).to(dev, torch.bfloat16)
    k = torch.randn(B, S, Hkv, D, generator=g).to(dev, torch.bfloat16)
    v = torch.randn(B, S, Hkv, D, generator=g).to(dev, torch.bfloat16)
    dout = torch.randn(B, S, Hq, D, generator=g).to(dev, torch.bfloat16)
    o = torch.empty_like(q)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
    _ok(lib.kf_attn_fwd(_p(o), _fp(lse), _p(q), _p(k), _p(v), B, S, Hq, Hkv,
                        D, 0, 0, scale, int(causal), _stream()), "attn_fwd")

    # new: kf_attn_bwd (always routes S % 256 == 0 to the fused dK/dV
    # kernel); it also leaves delta for the per-pass calls
    delta = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
    new = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    _ok(lib.kf_attn_bwd(_p(new[0]), _p(new[1]), _p(new[2]), _p(dout), _p(q),
                        _p(k), _p(v), _p(o), _fp(lse), _fp(delta), B, S, Hq,
                        Hkv, D, 0, 0, 0, 0, scale, int(causal), _stream()),
        "attn_bwd")
    # new: the fused kernel called directly (independent of the env switch)
    fused = [torch.full_like(t, float("nan")) for t in (k, v)]
    _ok(lib.kf_attn_bwd8_dkv_fused(
        _p(fused[0]), _p(fused[1]), _p(q), _p(k), _p(v), _p(dout), _fp(lse),
        _fp(delta), B, S, Hq, Hkv, Hq * D, Hkv * D, Hkv * D, scale,
        int(causal), _stream()), "dkv_fused")
    # parent path: the split entry points on the same delta
    old = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    _ok(lib.kf_attn_bwd8_dq(
        _p(old[0]), _p(q), _p(k), _p(v), _p(dout), _fp(lse), _fp(delta), B,
        S, Hq, Hkv, Hq * D, Hkv * D, Hq * D, scale, int(causal), _stream()),
        "dq8")
    _ok(lib.kf_attn_bwd8_dkv(
        _p(old[1]), _p(old[2]), _p(q), _p(k), _p(v), _p(dout), _fp(lse),
        _fp(delta), B, S, Hq, Hkv, Hq * D, Hkv * D, Hkv * D, scale,
        int(causal), _stream()), "dkv8")
    torch.cuda.synchronize()

    # fp32 oracle
    qr = q.float().cpu().transpose(1, 2).requires_grad_(True)
    kr = k.float().cpu().transpose(1, 2).requires_grad_(True)
    vr = v.float().cpu().transpose(1, 2).requires_grad_(True)
    R.sdpa(qr, kr, vr, causal=causal, scale=scale).backward(
        dout.float().cpu().transpose(1, 2))
    ref = [t.grad.transpose(1, 2) for t in (qr, kr, vr)]
    _cache[name] = dict(new=[t.cpu() for t in new],
                        fused=[t.cpu() for t in fused],
                        old=[t.cpu() for t in old], ref=ref)
    return _cache[name]


@pytest.mark.parametrize("name", list(PLAIN_CASES))
def test_fused_dkv_equals_split(name, gpu_device):
    r = _plain(name)
    for what, a, b in zip(("dq", "dk", "dv"), r["new"], r["old"]):
        assert torch.equal(a, b), f"kf_attn_bwd {what} differs from split"
    for what, a, b in zip(("dk", "dv"), r["fused"], r["old"][1:]):
        assert torch.equal(a, b), f"dkv_fused {what} differs from split"


@pytest.mark.parametrize("name", list(PLAIN_CASES))
def test_fused_dkv_within_oracle_bound(name, gpu_device):
    r = _plain(name)
    for what, a, b in zip(("dq", "dk", "dv"), r["new"], r["ref"]):
        err = _relerr(a, b)
        print(f"{name} kf_attn_bwd {what} relerr={err:.5f}")
        assert err < BOUND, (what, err)
    for what, a, b in zip(("dk", "dv"), r["fused"], r["ref"][1:]):
        err = _relerr(a, b)
        print(f"{name} dkv_fused {what} relerr={err:.5f}")
        assert err < BOUND, (what, err)


def _rope():
    """Strided fused-qkv layout + RoPE, run once."""
    if "rope" in _cache:
        return _cache["rope"]
    from kubeflow_amd.ops import _backend
    lib = _backend.require()
    B, S, Hq, Hkv = ROPE_CASE
    dev = torch.device("cuda", 0)
    scale = D ** -0.5
    ts = (Hq + 2 * Hkv) * D  # token stride of q, k, v and of dq, dk, dv
    ko, vo = Hq * D, (Hq + Hkv) * D
    g = torch.Generator(device="cpu").manual_seed(4321)
    qkv_raw = torch.randn(B, S, ts, generator=g).to(dev, torch.bfloat16)
    dout = torch.randn(B, S, Hq * D, generator=g).to(dev, torch.bfloat16)
    cos, sin = ops.rope_cos_sin(ROPE_TABLE_LEN, D, device=dev)

    qkv = qkv_raw.clone()  # rotated in place, as the fused forward does
    _ok(lib.kf_rope(_p(qkv), _p(qkv, ko), _fp(cos), _fp(sin), _null_i64(), B,
                    S, Hq, Hkv, D, ts, ts, 0, 0, _stream()), "rope_fwd")
    o = torch.empty(B, S, Hq * D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
    _ok(lib.kf_attn_fwd(_p(o), _fp(lse), _p(qkv), _p(qkv, ko), _p(qkv, vo),
                        B, S, Hq, Hkv, D, ts, ts, scale, 1, _stream()),
        "attn_fwd")
    delta = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)

    def buf():
        return torch.full_like(qkv, float("nan"))

    def rope_bwd(t):
        _ok(lib.kf_rope(_p(t), _p(t, ko), _fp(cos), _fp(sin), _null_i64(), B,
                        S, Hq, Hkv, D, ts, ts, 0, 1, _stream()), "rope_bwd")

    # new: one call, rotation in the store epilogues
    new = buf()
    _ok(lib.kf_attn_bwd_rope(
        _p(new), _p(new, ko), _p(new, vo), _p(dout), _p(qkv), _p(qkv, ko),
        _p(qkv, vo), _p(o), _fp(lse), _fp(delta), B, S, Hq, Hkv, D, ts, ts,
        ts, ts, scale, 1, _fp(cos), _fp(sin), 0, _stream()), "attn_bwd_rope")
    # new, per pass: dq8 / split dk8 / fused dkv with the rotation on
    split_rope, fused_rope = buf(), buf()
    for out, dkv in ((split_rope, lib.kf_attn_bwd8_dkv_rope),
                     (fused_rope, lib.kf_attn_bwd8_dkv_fused_rope)):
        _ok(lib.kf_attn_bwd8_dq_rope(
            _p(out), _p(qkv), _p(qkv, ko), _p(qkv, vo), _p(dout), _fp(lse),
            _fp(delta), B, S, Hq, Hkv, ts, ts, ts, scale, 1, _fp(cos),
            _fp(sin), 0, _stream()), "dq8_rope")
        _ok(dkv(_p(out, ko), _p(out, vo), _p(qkv), _p(qkv, ko), _p(qkv, vo),
                _p(dout), _fp(lse), _fp(delta), B, S, Hq, Hkv, ts, ts, ts,
                scale, 1, _fp(cos), _fp(sin), 0, _stream()), "dkv_rope")
    # parent path: kf_attn_bwd, then the separate adjoint pass
    old = buf()
    _ok(lib.kf_attn_bwd(
        _p(old), _p(old, ko), _p(old, vo), _p(dout), _p(qkv), _p(qkv, ko),
        _p(qkv, vo), _p(o), _fp(lse), _fp(delta), B, S, Hq, Hkv, D, ts, ts,
        ts, ts, scale, 1, _stream()), "attn_bwd")
    rope_bwd(old)
    # parent path with the split kernels named explicitly
    old_split = buf()
    _ok(lib.kf_attn_bwd8_dq(
        _p(old_split), _p(qkv), _p(qkv, ko), _p(qkv, vo), _p(dout), _fp(lse),
        _fp(delta), B, S, Hq, Hkv, ts, ts, ts, scale, 1, _stream()), "dq8")
    _ok(lib.kf_attn_bwd8_dkv(
        _p(old_split, ko), _p(old_split, vo), _p(qkv), _p(qkv, ko),
        _p(qkv, vo), _p(dout), _fp(lse), _fp(delta), B, S, Hq, Hkv, ts, ts,
        ts, scale, 1, _stream()), "dkv8")
    rope_bwd(old_split)
    torch.cuda.synchronize()

    # fp32 oracle: autograd through rope_apply + sdpa on the raw qkv
    ccpu, scpu = cos.cpu(), sin.cpu()
    ref_in = qkv_raw.float().cpu().requires_grad_(True)
    qc, kc, vc = ref_in.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q2 = R.rope_apply(qc.reshape(B, S, Hq, D), ccpu, scpu)
    k2 = R.rope_apply(kc.reshape(B, S, Hkv, D), ccpu, scpu)
    R.sdpa(q2.transpose(1, 2), k2.transpose(1, 2),
           vc.reshape(B, S, Hkv, D).transpose(1, 2), causal=True,
           scale=scale).transpose(1, 2).reshape(B, S, Hq * D).backward(
               dout.float().cpu())
    _cache["rope"] = dict(new=new.cpu(), split_rope=split_rope.cpu(),
                          fused_rope=fused_rope.cpu(), old=old.cpu(),
                          old_split=old_split.cpu(), ref=ref_in.grad,
                          split=[Hq * D, Hkv * D, Hkv * D])
    return _cache["rope"]


def test_rope_epilogue_equals_separate_pass(gpu_device):
    r = _rope()
    # the whole dqkv buffer: dq, dk rotated identically, dv byte-identical
    # and untouched by the rotation
    assert torch.equal(r["old"], r["old_split"])
    for name in ("new", "split_rope", "fused_rope"):
        for what, a, b in zip(("dq", "dk", "dv"),
                              r[name].split(r["split"], dim=-1),
                              r["old_split"].split(r["split"], dim=-1)):
            assert torch.equal(a, b), f"{name}: {what} differs"


def test_rope_epilogue_within_oracle_bound(gpu_device):
    r = _rope()
    for name in ("new", "split_rope", "fused_rope"):
        for what, a, b in zip(("dq", "dk", "dv"),
                              r[name].split(r["split"], dim=-1),
                              r["ref"].split(r["split"], dim=-1)):
            err = _relerr(a, b)
            print(f"rope {name} {what} relerr={err:.5f}")
            assert err < BOUND, (name, what, err)
