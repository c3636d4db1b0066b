"""The decode write path: kf_kv_store and kf_decode_rope_store against CPU
expectations over whole caches, one composed decode step (writer + reader),
and the index-tensor guard of the ctypes wrappers.

Caches start as seeded randn, never zeros, and the WHOLE cache is compared
with torch.equal against an expectation built on the CPU by advanced indexing,
so a stray write to any other row (a zero included) shows. kf_kv_store copies
a row of Hkv * D bf16 in passes of 128 lanes x 8 elements = 1024: the shapes
cover a row shorter than one pass, exactly one, two, and a partial second.
kf_decode_rope_store is compared with testing.rope_store_oracle (fp32
reference.rope_apply): q and the written k rows under rope's 2e-2 per row
(test_rope_fwd_bwd's bound), the written v rows bit for bit.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.ops import testing as T

DEV = torch.device("cuda", 0)
SLOTS, SMAX, TABLE = 8, 48, 64
ROPE_BOUND = 2e-2    # test_rope_fwd_bwd's bound, per row
DECODE_BOUND = 2e-2  # test_ops_branches_gpu.py::_check_decode's bounds
GARBAGE = 1e4        # cache rows >= len: finite, must never be read


@pytest.fixture(autouse=True)
def _require_native():
    from kubeflow_amd.ops import _backend
    _backend.require()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).bfloat16()


def _index(N):
    """(slots int32 [N], positions int64 [N]): distinct (slot, position)
    pairs, positions 0 and SMAX - 1 included, one slot used at two
    positions."""
    if N == 1:
        slots, pos = [SLOTS - 1], [SMAX - 1]   # the cache's last row
    else:
        slots = [7, 0, 3, 3, 5] + [(5 * i + 3) % SLOTS for i in range(5, N)]
        pos = [0, SMAX - 1, 10, 11, 32] + [(7 * i + 5) % SMAX
                                           for i in range(5, N)]
        assert 0 in pos and SMAX - 1 in pos
    assert len(set(zip(slots, pos))) == N
    return (torch.tensor(slots, dtype=torch.int32),
            torch.tensor(pos, dtype=torch.int64))


def _caches(g, Hkv, D):
    return (_randn(g, SLOTS, SMAX, Hkv, D), _randn(g, SLOTS, SMAX, Hkv, D))


# ---------------------------------------------------------------- kv_store

# (Hkv, D): row = Hkv * D elements against the 1024-element pass
KV_SHAPES = [
    (1, 128),    # a row shorter than one pass: lanes 16..127 idle
    (8, 128),    # exactly one pass
    (16, 128),   # two passes
    (9, 128),    # a partial second pass
    (2, 64),     # D = 64
]


@pytest.mark.parametrize("N", [1, 5, 33])
@pytest.mark.parametrize("Hkv,D", KV_SHAPES)
def test_kv_store_whole_cache(Hkv, D, N):
    g = _gen(80)
    ck0, cv0 = _caches(g, Hkv, D)
    row = Hkv * D
    # k and v as the split views of one fused [N, 1, 3 * row] buffer
    fused = _randn(g, N, 1, 3 * row)
    _, k, v = fused.split(row, dim=-1)
    slots, pos = _index(N)
    want_k, want_v = ck0.clone(), cv0.clone()
    want_k[slots.long(), pos] = k.reshape(N, Hkv, D)
    want_v[slots.long(), pos] = v.reshape(N, Hkv, D)
    fd = fused.to(DEV)
    _, ks, vs = fd.split(row, dim=-1)
    assert N == 1 or not ks.is_contiguous()
    layouts = {
        "[N,1,Hkv,D]": (k.reshape(N, 1, Hkv, D).to(DEV),
                        v.reshape(N, 1, Hkv, D).to(DEV)),
        "[N,Hkv,D]": (k.reshape(N, Hkv, D).to(DEV),
                      v.reshape(N, Hkv, D).to(DEV)),
        "split view": (ks.view(N, 1, Hkv, D), vs.view(N, 1, Hkv, D)),
    }
    for name, (kk, vv) in layouts.items():
        ck, cv = ck0.to(DEV), cv0.to(DEV)
        ops.kv_store(ck, cv, kk, vv, slots.to(DEV), pos.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(ck.cpu(), want_k), name
        assert torch.equal(cv.cpu(), want_v), name


def test_kv_store_row_not_multiple_of_8_is_still_exact():
    """row = 3 * 20 = 60: not a multiple of the 8-element vector, so the
    wrapper takes the indexing fallback."""
    Hkv, D, N = 3, 20, 5
    g = _gen(81)
    ck0, cv0 = _caches(g, Hkv, D)
    k, v = _randn(g, N, 1, Hkv, D), _randn(g, N, 1, Hkv, D)
    slots, pos = _index(N)
    want_k, want_v = ck0.clone(), cv0.clone()
    want_k[slots.long(), pos] = k[:, 0]
    want_v[slots.long(), pos] = v[:, 0]
    ck, cv = ck0.to(DEV), cv0.to(DEV)
    ops.kv_store(ck, cv, k.to(DEV), v.to(DEV), slots.to(DEV), pos.to(DEV))
    assert torch.equal(ck.cpu(), want_k) and torch.equal(cv.cpu(), want_v)


# ------------------------------------------------------- decode_rope_store

@pytest.mark.parametrize("N", [1, 5, 33])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 1), (8, 2), (4, 4)])
def test_decode_rope_store_against_oracle(Hq, Hkv, N):
    D = 128
    W = (Hq + 2 * Hkv) * D
    g = _gen(82)
    ck0, cv0 = _caches(g, Hkv, D)
    wide = _randn(g, N, 1, W + 64)
    qkv = wide[..., :W]                       # non-contiguous rows
    cos, sin = ops.rope_cos_sin(TABLE, D)
    slots, pos = _index(N)
    qo, ko, vo = T.rope_store_oracle(qkv, cos, sin, pos, Hq, Hkv, D)

    ck, cv = ck0.to(DEV), cv0.to(DEV)
    qd = wide.to(DEV)[..., :W]
    assert N == 1 or not qd.is_contiguous()
    cosd, sind, sd, pd = cos.to(DEV), sin.to(DEV), slots.to(DEV), pos.to(DEV)
    q = ops.decode_rope_store(qd, ck, cv, cosd, sind, sd, pd, Hq, Hkv)
    torch.cuda.synchronize()
    ck, cv = ck.cpu(), cv.cpu()
    sl = slots.long()
    eq, ek = T.row_err(q, qo), T.row_err(ck[sl, pos], ko)
    print(f"PARITY decode_rope_store Hq{Hq} Hkv{Hkv} N{N} q row={eq:.5f} "
          f"k row={ek:.5f} bound={ROPE_BOUND}")
    assert q.shape == (N, Hq, D)
    assert eq < ROPE_BOUND and ek < ROPE_BOUND
    assert torch.equal(cv[sl, pos].float(), vo)
    untouched = torch.ones(SLOTS, SMAX, dtype=torch.bool)
    untouched[sl, pos] = False
    assert torch.equal(ck[untouched], ck0[untouched])
    assert torch.equal(cv[untouched], cv0[untouched])

    # and bit-equal to the composition it replaces: rope + kv_store
    qq, kk, vv = qd.contiguous().split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    qr, kr = ops.rope(qq.view(N, 1, Hq, D), kk.view(N, 1, Hkv, D), cosd,
                      sind, positions=pd)
    ck2, cv2 = ck0.to(DEV), cv0.to(DEV)
    ops.kv_store(ck2, cv2, kr, vv.view(N, 1, Hkv, D), sd, pd)
    assert torch.equal(q, qr.reshape(N, Hq, D))
    assert torch.equal(ck2.cpu(), ck) and torch.equal(cv2.cpu(), cv)


def test_decode_step_writer_and_reader_agree():
    """decode_rope_store, then attention_decode with lens = positions + 1,
    over a cache prefilled on the CPU, against rope_store_oracle +
    decode_oracle: a writer and a reader that disagree on the cache layout
    fail here while each passes alone. Positions 0 (the new token is the only
    key), 63 / 64 (the decode kernel's tile edge) and 130."""
    N, Hq, Hkv, D, smax = 4, 8, 2, 128, 192
    positions = (0, 63, 64, 130)
    g = _gen(83)
    qkv = _randn(g, N, 1, (Hq + 2 * Hkv) * D)
    kc = _randn(g, N, smax, Hkv, D)
    vc = _randn(g, N, smax, Hkv, D)
    slots = torch.tensor([2, 0, 3, 1], dtype=torch.int32)
    pos = torch.tensor(positions, dtype=torch.int64)
    lens = (pos + 1).to(torch.int32)
    for s, p in zip(slots.tolist(), positions):
        kc[s, p:] = GARBAGE    # row p is the one the step writes
        vc[s, p:] = GARBAGE
    cos, sin = ops.rope_cos_sin(smax, D)
    qo, ko, vo = T.rope_store_oracle(qkv, cos, sin, pos, Hq, Hkv, D)
    kref, vref = kc.float(), vc.float()
    kref[slots.long(), pos] = ko
    vref[slots.long(), pos] = vo
    ref = T.decode_oracle(qo, kref, vref, slots, lens)

    kd, vd = kc.to(DEV), vc.to(DEV)
    q = ops.decode_rope_store(qkv.to(DEV), kd, vd, cos.to(DEV), sin.to(DEV),
                              slots.to(DEV), pos.to(DEV), Hq, Hkv)
    out = ops.attention_decode(q, kd, vd, slots.to(DEV), lens.to(DEV))
    torch.cuda.synchronize()
    out = out.float().cpu()
    row = T.row_err(out, ref)
    per_seq = [T.rel_err(out[i], ref[i]) for i in range(N)]
    print(f"PARITY decode step row_err={row:.5f} per_seq="
          f"{[round(e, 5) for e in per_seq]} bound={DECODE_BOUND}")
    assert row < DECODE_BOUND
    assert max(per_seq) < DECODE_BOUND


# ------------------------------------------------------ index-tensor guard

def _store_args(N=5, Hq=2, Hkv=2, D=128):
    g = _gen(84)
    ck, cv = (t.to(DEV) for t in _caches(g, Hkv, D))
    slots, pos = (t.to(DEV) for t in _index(N))
    return g, ck, cv, slots, pos


@pytest.mark.parametrize("bad", ["positions_int32", "slots_int64",
                                 "positions_on_cpu", "slots_too_short",
                                 "positions_strided"])
def test_store_ops_reject_wrong_index_tensors(bad):
    """The kernels read slots as int and positions as long long through bare
    pointers: anything else raises on the host and the caches keep their
    bits."""
    N, Hq, Hkv, D = 5, 2, 2, 128
    g, ck, cv, slots, pos = _store_args(N, Hq, Hkv, D)
    ck0, cv0 = ck.clone(), cv.clone()
    exc = ValueError
    if bad == "positions_int32":
        pos, exc = pos.int(), TypeError
    elif bad == "slots_int64":
        slots, exc = slots.long(), TypeError
    elif bad == "positions_on_cpu":
        pos = pos.cpu()
    elif bad == "slots_too_short":
        slots = slots[:N - 1]
    else:
        pos = torch.stack([pos, pos], dim=1)[:, 0]
        assert not pos.is_contiguous()
    k = _randn(g, N, 1, Hkv, D).to(DEV)
    with pytest.raises(exc, match="kv_store: "):
        ops.kv_store(ck, cv, k, k, slots, pos)
    qkv = _randn(g, N, 1, (Hq + 2 * Hkv) * D).to(DEV)
    cos, sin = (t.to(DEV) for t in ops.rope_cos_sin(TABLE, D))
    with pytest.raises(exc, match="decode_rope_store: "):
        ops.decode_rope_store(qkv, ck, cv, cos, sin, slots, pos, Hq, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(ck, ck0) and torch.equal(cv, cv0)


def test_attention_decode_rejects_wrong_index_tensors():
    N, Hq, Hkv, D = 5, 2, 2, 128
    g, ck, cv, slots, pos = _store_args(N, Hq, Hkv, D)
    q = _randn(g, N, Hq, D).to(DEV)
    lens = (pos + 1).int()
    with pytest.raises(TypeError, match="attention_decode: lens .*int32"):
        ops.attention_decode(q, ck, cv, slots, lens.long())
    with pytest.raises(TypeError, match="attention_decode: slots .*int32"):
        ops.attention_decode(q, ck, cv, slots.long(), lens)
    with pytest.raises(ValueError, match="attention_decode: lens .*shape"):
        ops.attention_decode(q, ck, cv, slots, lens[:N - 1])
    assert ops.attention_decode(q, ck, cv, slots, lens).shape == (N, Hq, D)


def test_rope_and_cross_entropy_reject_wrong_index_tensors():
    B, Hq, Hkv, D = 3, 2, 2, 128
    g = _gen(85)
    q, k = _randn(g, B, 1, Hq, D).to(DEV), _randn(g, B, 1, Hkv, D).to(DEV)
    cos, sin = (t.to(DEV) for t in ops.rope_cos_sin(TABLE, D))
    pos = torch.tensor([0, 17, TABLE - 1], dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError, match="rope: positions .*int64"):
        ops.rope(q, k, cos, sin, positions=pos.int())
    with pytest.raises(ValueError, match="rope: positions .*shape"):
        ops.rope(q, k, cos, sin, positions=pos[:2])
    logits = _randn(g, 8, 1000).to(DEV)
    targets = torch.arange(8, device=DEV)
    with pytest.raises(TypeError, match="cross_entropy: targets .*int64"):
        ops.cross_entropy(logits, targets.int())
    with pytest.raises(ValueError, match="cross_entropy: targets .*shape"):
        ops.cross_entropy(logits, targets[:7])
    assert torch.isfinite(ops.cross_entropy(logits, targets))
