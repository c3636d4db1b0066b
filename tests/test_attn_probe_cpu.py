"""The mask probe, the rectangular-attention oracle, the decode-store oracle
and the index-tensor guard, checked on the CPU from the reference alone.

The GPU files (test_attn_rect_gpu.py, test_decode_store_gpu.py and the probe
cases of the test_attn_d*_gpu.py files) rely on three claims made here:
  * testing.mask_probe_inputs gives key j the score 8 * j, every query's
    output row is its last visible key's v row, and a mask that is off by one
    key -- for every row or for one row among 300 -- fails the fixed per-row
    bounds by a wide margin (the figures are printed);
  * testing.attention_case_rect is the rectangular-causal attention that
    ops.flash_attention_rect and ops.masked_attention compute off the GPU;
  * testing.rope_store_oracle is what ops.decode_rope_store and ops.kv_store
    write off the GPU.
"""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import testing as T

O_BOUND = 2e-2    # test_attention_fwd's bound, per row
DV_BOUND = 4e-2   # test_attention_bwd's bound, per row
# fp32 math rounded once to bf16: half an ulp, 2^-8 relative per element
BF16_ROUND = 2.0 ** -8

# (D, C, Skv, q_offset): the rect shapes of the GPU file and the D = 64 square
PROBE_SHAPES = [(128, 300, 1115, 815), (128, 256, 256, 0),
                (128, 100, 133, 33), (64, 200, 200, 0)]
HQ, HKV = 2, 1


def _brute(q, k, v, scale, limits):
    """fp32 masked softmax, row i of every head attending keys <= limits[i].
    Written out here, sharing nothing with reference.sdpa's mask."""
    g = q.shape[2] // k.shape[2]
    kk = k.float().repeat_interleave(g, dim=2)
    vv = v.float().repeat_interleave(g, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), kk) * scale
    keys = torch.arange(k.shape[1]).view(1, 1, 1, -1)
    s = s.masked_fill(keys > limits.view(1, 1, -1, 1), float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), vv)


def _hot_rows(v, limits, Hq):
    """[B, C, Hq, D]: v[limit_i] of each head's kv head."""
    g = Hq // v.shape[2]
    return v.float()[:, limits].repeat_interleave(g, dim=2)


@pytest.mark.parametrize("D,C,Skv,off", PROBE_SHAPES)
def test_probe_scores_are_8j(D, C, Skv, off):
    q, k, v, scale = T.mask_probe_inputs(1, C, Skv, HQ, HKV, D, seed=7)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16 and scale == 0.125
    want = (8.0 * torch.arange(Skv)).view(1, 1, 1, Skv).expand(1, HQ, C, Skv)
    kk = k.float().repeat_interleave(HQ // HKV, dim=2)
    # the two structured dims give exactly 8 j ...
    s2 = torch.einsum("bqhd,bkhd->bhqk", q.float()[..., :2],
                      kk[..., :2]) * scale
    assert torch.equal(s2, want)
    # ... and the random dims move it by far less than the gap of 8
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), kk) * scale
    noise = (s - want).abs().max().item()
    print(f"PROBE D{D} C{C} Skv{Skv} off{off} score noise={noise:.4f}")
    assert noise < 0.25


@pytest.mark.parametrize("D,C,Skv,off", PROBE_SHAPES)
def test_probe_pins_every_row(D, C, Skv, off):
    """Hot-row property and the mutation figures against the fixed bounds."""
    q, k, v, scale = T.mask_probe_inputs(1, C, Skv, HQ, HKV, D, seed=7)
    n = off + C
    gen = torch.Generator(device="cpu").manual_seed(8)
    dout = torch.randn(1, C, HQ, D, generator=gen).bfloat16()
    o, _, _, _, dv = T.attention_oracle(q, k[:, :n], v[:, :n], dout, True,
                                        scale)
    limits = off + torch.arange(C)
    hot = T.row_err(o, _hot_rows(v, limits, HQ))
    same = T.row_err(_brute(q, k, v, scale, limits), o)
    # mask off by one key for every row, either way
    up = T.row_err(_brute(q, k, v, scale, (limits + 1).clamp_max(Skv - 1)), o)
    down = T.row_err(_brute(q, k, v, scale, (limits - 1).clamp_min(0)), o)
    # ... and for one row only, in the middle of the chunk
    one = limits.clone()
    one[C // 2] += 1 if off + C // 2 + 1 < Skv else -1
    single = T.row_err(_brute(q, k, v, scale, one), o)
    # dv[j] = the group's dout rows whose last visible key is j
    dv_want = torch.zeros(1, n, HKV, D)
    dv_want[:, off:] = dout.float().view(1, C, HKV, HQ // HKV, D).sum(dim=3)
    dv_hot = T.row_err(dv, dv_want)
    dv_shift = T.row_err(dv, torch.roll(dv_want, 1, dims=1))
    print(f"PROBE D{D} C{C} Skv{Skv} off{off} hot={hot:.2e} brute={same:.2e} "
          f"mask+1={up:.3f} mask-1={down:.3f} one_row={single:.3f} "
          f"dv_hot={dv_hot:.2e} dv_shift={dv_shift:.3f}")
    assert hot < O_BOUND / 10 and same < 1e-5
    assert dv_hot < DV_BOUND / 10
    for mutated in (up, down, single):
        assert mutated > 1.0 > O_BOUND
    assert dv_shift > 1.0 > DV_BOUND


def test_probe_breaks_emulated():
    """emulated() rounds the scores to bf16, whose spacing near 8 * 1115 is
    64: the order of neighbouring keys is lost, so it must not set a bound on
    the probe."""
    C, Skv, off = 300, 1115, 815
    q, k, v, scale = T.mask_probe_inputs(1, C, Skv, HQ, HKV, 128, seed=7)
    dout = torch.zeros(1, Skv, HQ, 128)
    qn = torch.zeros(1, Skv, HQ, 128, dtype=q.dtype)
    qn[:, off:] = q
    o = T.attention_oracle(qn, k, v, dout, True, scale)[0]
    e = T.emulated(qn, k, v, dout, True, scale)[0]
    err = T.row_err(e[:, off:], o[:, off:])
    print(f"PROBE emulated row_err={err:.3f}")
    assert err > 0.5


# (B, C, Skv, q_offset, Hq, Hkv): a short first chunk, an odd offset, B = 2,
# and Skv past the chunk's end
RECT_CASES = [(1, 40, 40, 0, 2, 1), (1, 100, 133, 33, 4, 1),
              (2, 70, 70, 0, 4, 2), (1, 64, 200, 50, 2, 2)]


@pytest.mark.parametrize("B,C,Skv,off,Hq,Hkv", RECT_CASES)
def test_rect_case_matches_brute_force_and_cpu_path(B, C, Skv, off, Hq, Hkv):
    case = T.attention_case_rect(B, C, Skv, off, Hq, Hkv)
    q, k, v = case.inputs
    assert q.shape == (B, C, Hq, 128) and k.shape == (B, Skv, Hkv, 128)
    assert set(case.oracle) == {"o", "lse"} and set(case.bound) == {"o"}
    assert case.oracle["lse"].shape == (B, Hq, C)
    limits = off + torch.arange(C)
    brute = T.row_err(_brute(q, k, v, 128 ** -0.5, limits), case.oracle["o"])
    cpu = T.row_err(ops.flash_attention_rect(q, k, v, off), case.oracle["o"])
    print(f"RECT B{B} C{C} Skv{Skv} off{off} brute={brute:.2e} cpu={cpu:.5f} "
          f"emu={case.emu_err['o']:.5f} bound={case.bound['o']:.5f}")
    assert brute < 1e-5
    assert cpu < BF16_ROUND < case.bound["o"]
    assert case.bound["o"] == T.ROW_BOUND_FACTOR * case.emu_err["o"]
    assert T.attention_case_rect(B, C, Skv, off, Hq, Hkv) is case  # cached


def test_rect_case_rejects_a_zero_bound():
    with pytest.raises(AssertionError):
        T.attention_case_rect(1, 1, 1, 0, 2, 2)   # one key: no error at all


def test_rect_case_matches_masked_attention_cpu_path():
    """One query row at offset kv_len - 1 sees keys [0, kv_len): the same
    rows ops.masked_attention attends, and attention_case's kv_len oracle."""
    kv_len = 37
    case = T.attention_case_rect(2, 1, 50, kv_len - 1, 2, 2)
    q, k, v = case.inputs
    got = ops.masked_attention(q, k, v, kv_len)
    assert T.row_err(got, case.oracle["o"]) < BF16_ROUND
    sq = T.attention_case(2, 128, 2, 2, False, kv_len=kv_len)
    q, k, v, _ = sq.inputs
    got = ops.masked_attention(q, k, v, kv_len)
    assert T.row_err(got, sq.oracle["o"]) < BF16_ROUND


@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 2)])
def test_rope_store_oracle_matches_cpu_fallbacks(Hq, Hkv):
    N, D, SLOTS, SMAX, TABLE = 5, 128, 4, 48, 64
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = torch.randn(N, 1, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    ck0 = torch.randn(SLOTS, SMAX, Hkv, D, generator=g).bfloat16()
    cv0 = torch.randn(SLOTS, SMAX, Hkv, D, generator=g).bfloat16()
    cos, sin = ops.rope_cos_sin(TABLE, D)
    slots = torch.tensor([3, 0, 2, 2, 1], dtype=torch.int32)
    pos = torch.tensor([0, SMAX - 1, 10, 11, 32], dtype=torch.int64)
    qo, ko, vo = T.rope_store_oracle(qkv, cos, sin, pos, Hq, Hkv, D)
    assert qo.dtype == ko.dtype == vo.dtype == torch.float32
    assert qo.shape == (N, Hq, D) and ko.shape == vo.shape == (N, Hkv, D)
    assert torch.equal(qo[0], qkv[0, 0, :Hq * D].float().view(Hq, D))  # pos 0

    ck, cv = ck0.clone(), cv0.clone()
    q = ops.decode_rope_store(qkv, ck, cv, cos, sin, slots, pos, Hq, Hkv)
    written = torch.zeros(SLOTS, SMAX, dtype=torch.bool)
    written[slots.long(), pos] = True
    assert T.row_err(q, qo) < BF16_ROUND
    assert T.row_err(ck[slots.long(), pos], ko) < BF16_ROUND
    assert torch.equal(cv[slots.long(), pos].float(), vo)
    assert torch.equal(ck[~written], ck0[~written])
    assert torch.equal(cv[~written], cv0[~written])

    # kv_store of the oracle's rows writes the same cache
    ck2, cv2 = ck0.clone(), cv0.clone()
    ops.kv_store(ck2, cv2, ko.bfloat16().view(N, 1, Hkv, D),
                 vo.bfloat16(), slots, pos)
    assert torch.equal(ck2, ck) and torch.equal(cv2, cv)


def test_index_arg_guard():
    like = torch.zeros(4, 2)
    ok = torch.zeros(4, dtype=torch.int32)
    assert ops._index_arg("kv_store", "slots", ok, torch.int32, 4, like) \
        is None
    with pytest.raises(TypeError, match="kv_store: positions .*int64"):
        ops._index_arg("kv_store", "positions", ok, torch.int64, 4, like)
    with pytest.raises(TypeError, match="attention_decode: lens .*int32"):
        ops._index_arg("attention_decode", "lens", ok.long(), torch.int32, 4,
                       like)
    with pytest.raises(TypeError, match="rope: positions must be a tensor"):
        ops._index_arg("rope", "positions", [0, 1, 2, 3], torch.int64, 4,
                       like)
    with pytest.raises(ValueError, match=r"cross_entropy: targets .*\[5\]"):
        ops._index_arg("cross_entropy", "targets", ok.long(), torch.int64, 5,
                       like)
    with pytest.raises(ValueError, match=r"shape \[4\]"):
        ops._index_arg("kv_store", "slots", ok.view(4, 1), torch.int32, 4,
                       like)
    strided = torch.zeros(8, dtype=torch.int32)[::2]
    with pytest.raises(ValueError, match="decode_rope_store: slots .*contig"):
        ops._index_arg("decode_rope_store", "slots", strided, torch.int32, 4,
                       like)
    elsewhere = torch.zeros(4, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="kv_store: slots must be on cpu"):
        ops._index_arg("kv_store", "slots", elsewhere, torch.int32, 4, like)
