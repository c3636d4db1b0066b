"""kf_attn_fwd4_rect (attention_fwd4.hip) through ops.flash_attention_rect
(chunked prefill), ops.masked_attention at D = 128 (padded BERT) and the entry
point itself, against the fp32 oracle and against the mask probe.

Random-input cases (testing.attention_case_rect / attention_case with kv_len):
seeded on the CPU, whole-tensor rel. error < 2e-2 (test_attention_fwd's bound)
and per-row error < 3 x the all-bf16 emulation's per-row error, derived from
the reference alone.

Probe cases (testing.mask_probe_inputs): key j scores 8 * j, so every query
row must come out as the v row of its LAST visible key; per-row 2e-2 against
attention_oracle on the probe inputs and against v[limit] itself. A mask off
by one key in one row gives a per-row error above 1 (test_attn_probe_cpu.py).

The kernel: 256 q rows per block (A4_QT), 8 waves of 32 rows, 64-key tiles
(A4_KT) double-buffered, each processed as two 32-key sub-blocks. Per wave a
sub-block is skipped when it starts past wave_qmax + qoff (do0 / do1) and
masked only when it crosses the wave's diagonal or skv; last_kt clips the
tile loop per block; a wave that skips a whole tile still has to write the
staged next tile; pad q rows clamp their limit to skv - 1. k/v rows that must
not count hold 1e4 where the case allows it: finite, so they would show.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.ops import testing as T

D = 128
FWD_BOUND = 2e-2   # test_attention_fwd's bound, whole tensor and probe rows
LSE_ATOL = 1e-2    # test_attn_d128_paths_gpu.py's LSE_ATOL
GARBAGE = 1e4      # finite, must contribute exactly nothing
DEV = torch.device("cuda", 0)

# name -> (B, C, Skv, q_offset, Hq, Hkv)
RECT_CASES = {
    # first chunk shorter than one tile: the tail sub-block (32..39) is masked
    # both by skv and by the diagonal; 216 pad q rows clamp to skv - 1
    "short_first_chunk": (1, 40, 40, 0, 2, 1),
    # the plain causal square, skv = S and qoff = 0
    "square_256": (1, 256, 256, 0, 4, 2),
    # odd offset: the diagonal crosses sub-blocks inside a wave; g = 4
    "odd_offset_gqa4": (1, 100, 133, 33, 4, 1),
    # wave 1 (limits 63..94) needs tile 1, wave 0 (limits 31..62) does not:
    # per-wave skip + the "staged tile still lands" branch; g = 8
    "per_wave_skip_gqa8": (1, 64, 95, 31, 8, 1),
    # a second q block holding one real row (and its own last_kt)
    "second_block_one_row": (1, 257, 321, 64, 2, 2),
    # B = 2: the repack path, kv batch stride = padded Sq
    "batch2_repack": (2, 300, 300, 0, 4, 2),
    # Skv % 64 = 27 with an odd offset, 18 kv tiles
    "long_odd": (1, 300, 1115, 815, 2, 1),
}
# long prefix: ten full unmasked tiles, then the diagonal; zero-copy path
SLAB_CASE = (1, 96, 737, 641, 8, 2)
SLAB_ROWS = 768
# Skv > q_offset + C: keys 114..199 are inside skv, masked by causality alone
PAST_END_CASE = (1, 64, 200, 50, 2, 2)

# (C, Skv, q_offset), Hq, Hkv = 4, 2; the 737 case runs in the slab
PROBE_CASES = [(256, 256, 0), (100, 133, 33), (64, 95, 31), (96, 737, 641),
               (300, 1115, 815)]
PROBE_HQ, PROBE_HKV = 4, 2

# ops.masked_attention at D = 128: (S, kv_len); B = 2, Hq = Hkv = 2. One key,
# the sub-block edge 32 and both neighbours, the tile edge 64 and one past
# it, the whole sequence; S = 300 pads q to 512 (two blocks) with 4 kv tiles
MASKED_CASES = [(128, 1), (128, 31), (128, 32), (128, 33), (128, 64),
                (128, 65), (128, 128), (300, 200)]
MASKED_B, MASKED_H = 2, 2


@pytest.fixture(autouse=True)
def _require_native():
    from kubeflow_amd.ops import _backend
    _backend.require()


def _check_o(name, got, want, bound):
    whole, row = T.rel_err(got, want), T.row_err(got, want)
    print(f"PARITY {name} o whole={whole:.5f} (<{FWD_BOUND}) row={row:.5f} "
          f"bound={bound:.5f}")
    assert got.shape == want.shape, name
    assert whole < FWD_BOUND, (name, whole)
    assert row < bound, (name, row, bound)


def _slab(k, v):
    """k/v [1, Skv, Hkv, D] as the [1:2, :Skv] view of a [3, SLAB_ROWS, Hkv,
    D] slab whose every other row holds GARBAGE (the zero-copy path of
    ops.flash_attention_rect)."""
    Skv, Hkv = k.shape[1], k.shape[2]
    views = []
    for t in (k, v):
        slab = torch.full((3, SLAB_ROWS, Hkv, D), GARBAGE,
                          dtype=torch.bfloat16, device=DEV)
        slab[1, :Skv] = t[0].to(DEV)
        views.append(slab[1:2, :Skv])
    return views


# ------------------------------------------------------- random-input cases

def test_one_key_is_exact():
    """(1, 1, 1, 0, 2, 2): the only key gets weight 1, so o is its v row
    whatever q and k hold (attention_case_rect refuses the case: its bound
    would be zero)."""
    B, C, Skv, off, Hq, Hkv = 1, 1, 1, 0, 2, 2
    g = torch.Generator(device="cpu").manual_seed(31)
    q = torch.randn(B, C, Hq, D, generator=g).bfloat16()
    k = torch.randn(B, Skv, Hkv, D, generator=g).bfloat16()
    v = torch.randn(B, Skv, Hkv, D, generator=g).bfloat16()
    o = ops.flash_attention_rect(q.to(DEV), k.to(DEV), v.to(DEV), off)
    assert torch.equal(o.cpu(), v[:, :1].repeat_interleave(Hq // Hkv, dim=2))


@pytest.mark.parametrize("name", list(RECT_CASES))
def test_rect_both_metrics(name):
    B, C, Skv, off, Hq, Hkv = RECT_CASES[name]
    case = T.attention_case_rect(B, C, Skv, off, Hq, Hkv)
    q, k, v = (t.to(DEV) for t in case.inputs)
    o = ops.flash_attention_rect(q, k, v, off)
    torch.cuda.synchronize()
    _check_o(name, o, case.oracle["o"], case.bound["o"])


def test_square_is_bit_equal_to_fwd4():
    """skv = S, qoff = 0 is kf_attn_fwd4 itself: same bits."""
    from kubeflow_amd.ops import _backend
    lib = _backend.require()
    B, C, Skv, off, Hq, Hkv = RECT_CASES["square_256"]
    case = T.attention_case_rect(B, C, Skv, off, Hq, Hkv)
    q, k, v = (t.to(DEV) for t in case.inputs)
    o = ops.flash_attention_rect(q, k, v, off)
    o4 = _nan(B, C, Hq, D)
    lse4 = _nan(B, Hq, C, dtype=torch.float32)
    _ok(lib.kf_attn_fwd4(_p(o4), _fp(lse4), _p(q), _p(k), _p(v), B, C, Hq,
                         Hkv, D, 0, 0, D ** -0.5, 1, _stream()), "attn_fwd4")
    torch.cuda.synchronize()
    assert torch.equal(o, o4)


def test_long_prefix_in_slab():
    B, C, Skv, off, Hq, Hkv = SLAB_CASE
    case = T.attention_case_rect(B, C, Skv, off, Hq, Hkv)
    q, k, v = case.inputs
    kv, vv = _slab(k, v)
    o = ops.flash_attention_rect(q.to(DEV), kv, vv, off)
    torch.cuda.synchronize()
    _check_o("long_prefix_slab", o, case.oracle["o"], case.bound["o"])


def test_keys_past_chunk_end_masked_by_causality():
    B, C, Skv, off, Hq, Hkv = PAST_END_CASE
    case = T.attention_case_rect(B, C, Skv, off, Hq, Hkv)
    q, k, v = (t.clone() for t in case.inputs)
    k[:, off + C:] = GARBAGE
    v[:, off + C:] = GARBAGE
    o = ops.flash_attention_rect(q.to(DEV), k.to(DEV), v.to(DEV), off)
    torch.cuda.synchronize()
    _check_o("skv_past_chunk_end", o, case.oracle["o"], case.bound["o"])


# -------------------------------------------------------------- probe cases

def _check_probe(name, o, oracle, hot):
    e_or, e_hot = T.row_err(o, oracle), T.row_err(o, hot)
    print(f"PARITY {name} probe row_vs_oracle={e_or:.5f} "
          f"row_vs_v={e_hot:.5f} bound={FWD_BOUND}")
    assert o.shape == oracle.shape, name
    assert e_or < FWD_BOUND, (name, e_or)
    assert e_hot < FWD_BOUND, (name, e_hot)


@pytest.mark.parametrize("C,Skv,off", PROBE_CASES)
def test_rect_probe_every_row_is_its_last_key(C, Skv, off):
    q, k, v, scale = T.mask_probe_inputs(1, C, Skv, PROBE_HQ, PROBE_HKV, D,
                                         seed=41)
    n = off + C
    oracle = T.attention_oracle(q, k[:, :n], v[:, :n],
                                torch.zeros(1, C, PROBE_HQ, D), True,
                                scale)[0]
    hot = v.float()[:, off:n].repeat_interleave(PROBE_HQ // PROBE_HKV, dim=2)
    if Skv == SLAB_CASE[2]:
        kv, vv = _slab(k, v)
    else:
        kv, vv = k.to(DEV), v.to(DEV)
    o = ops.flash_attention_rect(q.to(DEV), kv, vv, off, scale=scale)
    torch.cuda.synchronize()
    _check_probe(f"rect C{C} Skv{Skv} off{off}", o, oracle, hot)


# ------------------------------------------------------- direct entry point

def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _fp(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(err, name):
    assert err == 0, f"{name} failed with hipError_t={err}"


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@pytest.mark.parametrize("name", ["per_wave_skip_gqa8", "batch2_repack"])
def test_direct_entry_stores_every_real_row(name):
    """kf_attn_fwd4_rect on NaN-filled o and lse: every real row is stored,
    o and lse match the oracle; pad rows are ignored. The kv buffers have the
    kernel's own layout ([B, padded Sq, Hkv, D]), GARBAGE past Skv."""
    from kubeflow_amd.ops import _backend
    lib = _backend.require()
    B, C, Skv, off, Hq, Hkv = RECT_CASES[name]
    case = T.attention_case_rect(B, C, Skv, off, Hq, Hkv)
    q, k, v = case.inputs
    Sp = (C + 255) // 256 * 256
    assert (Skv + 63) // 64 * 64 <= Sp   # every tile read stays in the buffer
    qp = torch.zeros(B, Sp, Hq, D, dtype=torch.bfloat16, device=DEV)
    qp[:, :C] = q.to(DEV)
    kp = torch.full((B, Sp, Hkv, D), GARBAGE, dtype=torch.bfloat16,
                    device=DEV)
    vp = kp.clone()
    kp[:, :Skv], vp[:, :Skv] = k.to(DEV), v.to(DEV)
    o = _nan(B, Sp, Hq, D)
    lse = _nan(B, Hq, Sp, dtype=torch.float32)
    _ok(lib.kf_attn_fwd4_rect(_p(o), _fp(lse), _p(qp), _p(kp), _p(vp), B, Sp,
                              Skv, Hq, Hkv, D, 0, 0, D ** -0.5, off,
                              _stream()), "attn_fwd4_rect")
    torch.cuda.synchronize()
    o, lse = o[:, :C].cpu(), lse[:, :, :C].cpu()
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    _check_o(f"direct {name}", o, case.oracle["o"], case.bound["o"])
    d = (lse - case.oracle["lse"]).abs().max().item()
    print(f"PARITY direct {name} lse maxabs={d:.6f} atol={LSE_ATOL}")
    assert torch.allclose(lse, case.oracle["lse"], atol=LSE_ATOL), d


def test_batched_skv_longer_than_padded_chunk_raises():
    """The kernel's kv batch stride is the padded Sq: B = 2 with more kv rows
    than that cannot be laid out; the wrapper raises before any launch."""
    q = torch.zeros(2, 64, 2, D, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros(2, 300, 2, D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="batched rectangular attention"):
        ops.flash_attention_rect(q, k, k, 236)


# --------------------------------------------- ops.masked_attention, D = 128

@pytest.mark.parametrize("S,kv_len", MASKED_CASES)
def test_masked_attention_d128_both_metrics(S, kv_len):
    B, H = MASKED_B, MASKED_H
    if kv_len == 1:   # one key: weight 1, no rounding, and no emulation error
        q, k, v, _ = T.attention_inputs(B, S, H, H, D)
        want, bound = v[:, :1].expand(B, S, H, D), None
    else:
        case = T.attention_case(B, S, H, H, False, kv_len=kv_len)
        q, k, v, _ = case.inputs
        want, bound = case.oracle["o"], case.bound["o"]
    k, v = k.clone(), v.clone()
    k[:, kv_len:] = GARBAGE
    v[:, kv_len:] = GARBAGE
    o = ops.masked_attention(q.to(DEV), k.to(DEV), v.to(DEV), kv_len)
    torch.cuda.synchronize()
    if bound is None:
        assert torch.equal(o.cpu(), want)
    else:
        _check_o(f"masked S{S} kv_len{kv_len}", o, want, bound)


@pytest.mark.parametrize("S,kv_len", MASKED_CASES)
def test_masked_attention_d128_probe(S, kv_len):
    """Every row is v[kv_len - 1]."""
    B, H = MASKED_B, MASKED_H
    q, k, v, scale = T.mask_probe_inputs(B, S, S, H, H, D, seed=43)
    oracle = T.attention_oracle(q, k, v, torch.zeros(B, S, H, D), False,
                                scale, kv_len=kv_len)[0]
    hot = v.float()[:, kv_len - 1:kv_len].expand(B, S, H, D)
    k[:, kv_len:] = GARBAGE
    v[:, kv_len:] = GARBAGE
    o = ops.masked_attention(q.to(DEV), k.to(DEV), v.to(DEV), kv_len,
                             scale=scale)
    torch.cuda.synchronize()
    _check_probe(f"masked S{S} kv_len{kv_len}", o, oracle, hot)
