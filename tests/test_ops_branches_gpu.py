"""Kernel branches and loops that tests/test_ops_gpu.py never enters, against
the fp32 oracles of kubeflow_amd/ops/testing.py.

Two kinds of case:
  * loop-entering shapes: the smallest sizes above each capped grid
    (kf_grid_for caps at 2048 blocks, the norm backward kernels at 1024), so
    the grid-stride loop, its trailing barrier and the multi-chunk LDS slot
    indexing of the norm backward kernels run more than one iteration;
  * dispatch branches: decode attention over g / splits / VDIRECT / len edges,
    the direct-load skinny GEMM templates and M edges, the CE scalar row loop.

Every comparison uses the op's whole-tensor bound from test_ops_gpu.py and the
same number as a per-row (row_err) or per-column (col_err) bound: a correctly
rounded bf16 row sits near 2^-9 ~ 0.002, a wrong or missing row near 1.
Inputs are seeded on the CPU; each case's comment names the branch it enters.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.ops import testing as T

DEV = torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_native():
    from kubeflow_amd.ops import _backend
    _backend.require()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).bfloat16()


def _both(name, got, ref, bound, metric=T.row_err):
    """Whole-tensor and per-row (or per-column) error under the same bound."""
    whole, row = T.rel_err(got, ref), metric(got, ref)
    print(f"PARITY {name} whole={whole:.5f} {metric.__name__}={row:.5f} "
          f"bound={bound}")
    assert got.shape == ref.shape, name
    assert whole < bound, (name, whole)
    assert row < bound, (name, row)


# ------------------------------------------------------------ norm kernels

NORM_SHAPES = [
    # rows > 2048: forward row loop; rows > 1024: backward row loop + barrier;
    # cols/8 = 33 < 256: threads without a slot
    (2051, 264),
    # cols = 2056 > 2048: 257 vectors, a second slot chunk for thread 0 only
    (1100, 2056),
    # the production width: two full slot chunks per thread, rows > 2048
    (2051, 4096),
]


@pytest.mark.parametrize("rows,cols", NORM_SHAPES)
def test_rmsnorm_loop_shapes(rows, cols):
    g = _gen(10)
    x, w, dy = _randn(g, rows, cols), _randn(g, cols), _randn(g, rows, cols)
    xg, wg = (t.to(DEV).requires_grad_(True) for t in (x, w))
    y = ops.rms_norm(xg, wg)
    y.backward(dy.to(DEV))
    yr, dxr, dwr = T.rms_norm_oracle(x, w, dy)
    _both("rmsnorm y", y, yr, 2e-2)            # test_rmsnorm_fwd's bound
    _both("rmsnorm dx", xg.grad, dxr, 3e-2)    # test_rmsnorm_bwd's bounds
    _both("rmsnorm dw", wg.grad, dwr, 3e-2, T.col_err)


@pytest.mark.parametrize("rows,cols", NORM_SHAPES)
def test_layernorm_loop_shapes(rows, cols):
    g = _gen(11)
    x, w, b = _randn(g, rows, cols), _randn(g, cols), _randn(g, cols)
    dy = _randn(g, rows, cols)
    xg, wg, bg = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = ops.layer_norm(xg, wg, bg, eps=1e-6)
    y.backward(dy.to(DEV))
    yr, dxr, dwr, dbr = T.layer_norm_oracle(x, w, b, dy, eps=1e-6)
    # test_layernorm_fwd_bwd's bounds
    _both("layernorm y", y, yr, 2e-2)
    _both("layernorm dx", xg.grad, dxr, 5e-2)
    _both("layernorm dw", wg.grad, dwr, 3e-2, T.col_err)
    _both("layernorm db", bg.grad, dbr, 3e-2, T.col_err)


def test_norms_reject_cols_not_multiple_of_8():
    """Host-side argument check: returns before any launch."""
    x = torch.zeros(4, 12, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(12, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="rmsnorm_fwd"):
        ops.rms_norm(x, w)
    with pytest.raises(RuntimeError, match="layernorm_fwd"):
        ops.layer_norm(x, w, w)


# -------------------------------------------------------------------- rope

def test_rope_grid_stride_with_pos_offset():
    """B1 S1100 Hq24 Hkv8 D128: 563 200 work items > 2048 x 256, so the
    grid-stride loop runs twice for the first blocks; pos_offset = 5 with a
    table of exactly S + 5 rows (the last row is used)."""
    B, S, Hq, Hkv, D, off = 1, 1100, 24, 8, 128, 5
    g = _gen(20)
    q, k = _randn(g, B, S, Hq, D), _randn(g, B, S, Hkv, D)
    dq2, dk2 = _randn(g, B, S, Hq, D), _randn(g, B, S, Hkv, D)
    cos, sin = ops.rope_cos_sin(S + off, D)
    qg, kg = (t.to(DEV).requires_grad_(True) for t in (q, k))
    q2, k2 = ops.rope(qg, kg, cos.to(DEV), sin.to(DEV), pos_offset=off)
    ((q2 * dq2.to(DEV)).sum() + (k2 * dk2.to(DEV)).sum()).backward()
    q2r, k2r, dqr, dkr = T.rope_oracle(q, k, cos, sin, off, None, dq2, dk2)
    # test_rope_fwd_bwd's bound
    _both("rope q", q2, q2r, 2e-2)
    _both("rope k", k2, k2r, 2e-2)
    _both("rope dq", qg.grad, dqr, 2e-2)
    _both("rope dk", kg.grad, dkr, 2e-2)


def test_rope_positions_against_reference():
    """positions= (serving decode: B sequences, S = 1, one base position per
    batch row) against reference.rope_apply per row — the oracle that
    test_decode_rope_store_parity does not have. Positions include 0 and the
    table's last row."""
    B, S, Hq, Hkv, D, TABLE = 3, 1, 8, 2, 128, 64
    g = _gen(21)
    q, k = _randn(g, B, S, Hq, D), _randn(g, B, S, Hkv, D)
    dq2, dk2 = _randn(g, B, S, Hq, D), _randn(g, B, S, Hkv, D)
    cos, sin = ops.rope_cos_sin(TABLE, D)
    pos = torch.tensor([0, 17, TABLE - 1], dtype=torch.int64)
    qg, kg = (t.to(DEV).requires_grad_(True) for t in (q, k))
    q2, k2 = ops.rope(qg, kg, cos.to(DEV), sin.to(DEV),
                      positions=pos.to(DEV))
    ((q2 * dq2.to(DEV)).sum() + (k2 * dk2.to(DEV)).sum()).backward()
    q2r, k2r, dqr, dkr = T.rope_oracle(q, k, cos, sin, 0, pos, dq2, dk2)
    assert torch.equal(q2[0].cpu(), q[0])  # position 0 is the identity
    _both("rope positions q", q2, q2r, 2e-2)
    _both("rope positions k", k2, k2r, 2e-2)
    _both("rope positions dq", qg.grad, dqr, 2e-2)
    _both("rope positions dk", kg.grad, dkr, 2e-2)


# ------------------------------------------------------------------ swiglu

def test_swiglu_grid_stride():
    """T1030 F4104: 528 390 vectors > 2048 x 256 in forward and backward. F is
    an 8 multiple (every row and half-row start stays 16-byte aligned) but not
    a 64 one, so the t / f decode of a vector index is not a shift."""
    Tn, Fn = 1030, 4104
    g = _gen(30)
    h, dy = _randn(g, Tn, 2 * Fn), _randn(g, Tn, Fn)
    hg = h.to(DEV).requires_grad_(True)
    y = ops.swiglu(hg)
    y.backward(dy.to(DEV))
    yr, dhr = T.swiglu_oracle(h, dy)
    _both("swiglu y", y, yr, 2e-2)          # test_swiglu_fwd_bwd's bounds
    _both("swiglu dh", hg.grad, dhr, 3e-2)


# ------------------------------------------------------------------- adamw

ADAMW_N = 2 * 1024 * 1024 + 4 * 257  # n/4 = 524 545 vectors > 2048 x 256


def _pad_rows(t, width=4096):
    t = t.detach().float().cpu().flatten()
    pad = (-t.numel()) % width
    return torch.cat([t, t.new_zeros(pad)]).view(-1, width)


@pytest.mark.parametrize("masked", [False, True])
def test_fused_adamw_grid_stride(masked):
    """Two steps over a shard longer than one pass of the capped grid, with
    wd_mask=None (null-pointer branch) and with a {0,1} mask."""
    n = ADAMW_N
    g = _gen(40)
    p0 = torch.randn(n, generator=g)
    grads = [_randn(g, n) for _ in range(2)]
    mask = (torch.rand(n, generator=g) > 0.5).float() if masked else None
    p32 = p0.to(DEV)
    p16 = p32.to(torch.bfloat16)
    m, v = torch.zeros_like(p32), torch.zeros_like(p32)
    mg = mask.to(DEV) if masked else None
    hp = (1e-2, 0.9, 0.95, 1e-8, 0.1)
    for step, gr in enumerate(grads, 1):
        ops.fused_adamw(p16, p32, gr.to(DEV), m, v, mg, *hp, step)
    pr, mr, vr = T.adamw_oracle(p0, grads, mask, *hp)
    for name, got, ref in (("p32", p32, pr), ("m", m, mr), ("v", v, vr)):
        # test_fused_adamw_matches_reference's bound, whole and per 4096 row
        _both(f"adamw {name}", _pad_rows(got), _pad_rows(ref), 1e-4)
        # and per element: one skipped vector is 4 of 2M elements
        assert torch.allclose(got.cpu(), ref, rtol=1e-4, atol=1e-6), name
    _both("adamw p16", _pad_rows(p16), _pad_rows(pr), 1e-2)
    # p16 = bf16(p32): within one bf16 ulp (2^-7 relative) of the oracle
    assert torch.allclose(p16.float().cpu(), pr, rtol=2.0 ** -7, atol=1e-6)


def test_fused_adamw_rejects_n_not_multiple_of_4():
    p32 = torch.zeros(6, device=DEV)
    p16 = p32.to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="adamw"):
        ops.fused_adamw(p16, p32, p16.clone(), p32.clone(), p32.clone(), None,
                        1e-2, 0.9, 0.95, 1e-8, 0.1, 1)
    assert not p32.any()


# ----------------------------------------------------------- cross entropy

CE_SHAPES = [
    (2100, 1000),  # T > 2048: the strided row loop; V % 8 == 0 vector path
    (64, 1003),    # V % 8 != 0: whole rows in the scalar loop (rows start at
                   # 2-byte-aligned addresses, no 16-byte access is legal)
]


def _ce_inputs(Tn, V, seed=50):
    g = _gen(seed)
    logits = _randn(g, Tn, V)
    targets = torch.randint(0, V, (Tn,), generator=g)
    targets[::7] = -100
    return logits, targets


@pytest.mark.parametrize("Tn,V", CE_SHAPES)
@pytest.mark.parametrize("grad_out", [1.0, 0.25])
def test_cross_entropy_loop_and_tail(Tn, V, grad_out):
    logits, targets = _ce_inputs(Tn, V)
    lg = logits.to(DEV).requires_grad_(True)
    loss = ops.cross_entropy(lg, targets.to(DEV))
    loss.backward(torch.tensor(grad_out, device=DEV))
    lr, dlr = T.cross_entropy_oracle(logits, targets, grad_out=grad_out)
    print(f"PARITY ce loss got={loss.item():.6f} ref={lr.item():.6f}")
    # test_cross_entropy's bounds
    assert abs(loss.item() - lr.item()) / abs(lr.item()) < 1e-2
    _both("ce dlogits", lg.grad, dlr, 2e-2)
    # ignored rows get an exactly zero gradient
    assert not lg.grad[::7].any()


@pytest.mark.parametrize("Tn,V", CE_SHAPES)
def test_cross_entropy_all_ignored(Tn, V):
    """The wrapper's inv_valid = 0 semantics: loss exactly 0.0 and an exactly
    zero gradient (not F.cross_entropy's NaN)."""
    logits, _ = _ce_inputs(Tn, V)
    lg = logits.to(DEV).requires_grad_(True)
    loss = ops.cross_entropy(lg, torch.full((Tn,), -100, device=DEV))
    loss.backward()
    assert loss.item() == 0.0
    assert torch.equal(lg.grad, torch.zeros_like(lg.grad))


@pytest.mark.parametrize("Tn,V", CE_SHAPES)
def test_cross_entropy_inplace_non_leaf(Tn, V):
    """Non-leaf logits take the in-place dlogits path (kf_ce_bwd writes into
    the saved logits buffer); the gradient must equal the leaf path's."""
    logits, targets = _ce_inputs(Tn, V)
    tg = targets.to(DEV)
    leaf = logits.to(DEV).requires_grad_(True)
    ops.cross_entropy(leaf, tg).backward()
    x = logits.to(DEV).requires_grad_(True)
    nonleaf = x * 1.0
    assert not nonleaf.is_leaf
    ops.cross_entropy(nonleaf, tg).backward()
    assert torch.equal(x.grad, leaf.grad)
    _, dlr = T.cross_entropy_oracle(logits, targets)
    _both("ce in-place dlogits", x.grad, dlr, 2e-2)


# -------------------------------------------------------- decode attention

DEC_LENS = [0, 1, 63, 64, 65, 128, 200, 256]  # empty, tile edges, mid-tile
DEC_SLOTS = [5, 0, 3, 7, 1, 6, 2, 4]
DEC_SMAX = 256
GARBAGE = 1e4  # cache rows >= len: finite, must never be read
_dec_cache = {}


def _decode_inputs(N, Hq, Hkv, smax, lens, slots, seed=60):
    key = (N, Hq, Hkv, smax, tuple(lens), tuple(slots))
    if key not in _dec_cache:
        g = _gen(seed)
        D = 128
        q = _randn(g, N, Hq, D)
        kc = _randn(g, N, smax, Hkv, D)
        vc = _randn(g, N, smax, Hkv, D)
        for s, L in zip(slots, lens):
            kc[s, L:] = GARBAGE
            vc[s, L:] = GARBAGE
        st = torch.tensor(slots, dtype=torch.int32)
        lt = torch.tensor(lens, dtype=torch.int32)
        ref = T.decode_oracle(q, kc, vc, st, lt)
        _dec_cache[key] = (q, kc, vc, st, lt, ref)
    return _dec_cache[key]


def _check_decode(name, out, ref, lens):
    out = out.float().cpu()
    # per-row metric over the (n, hq) rows, test_attention_decode's bound
    row = T.row_err(out, ref)
    print(f"PARITY {name} row_err={row:.5f}")
    assert row < 2e-2, (name, row)
    # the existing per-sequence check (long sequences have small rows, which
    # the rms floor of row_err would otherwise judge leniently)
    for i, L in enumerate(lens):
        if L == 0:
            assert torch.equal(out[i], torch.zeros_like(out[i])), name
        else:
            assert T.rel_err(out[i], ref[i]) < 2e-2, (name, i, L)


@pytest.mark.parametrize("vdirect", [None, "1"])
# splits 1: direct-store epilogue; 2, 3: empty (lo >= hi) and mid-tile split
# ends, combine kernel; 8: the serving default
@pytest.mark.parametrize("splits", [1, 2, 3, 8])
# g = 1 and 2: idle waves; g = 4: one head per wave; g = 8: the hbase outer
# loop (two passes over the cache)
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 2), (8, 2), (8, 1)])
def test_attention_decode_branches(Hq, Hkv, splits, vdirect, monkeypatch):
    monkeypatch.setenv("KF_DECODE_SPLITS", str(splits))
    if vdirect is None:
        monkeypatch.delenv("KF_DECODE_VDIRECT", raising=False)
    else:
        monkeypatch.setenv("KF_DECODE_VDIRECT", vdirect)  # read on each call
    q, kc, vc, st, lt, ref = _decode_inputs(8, Hq, Hkv, DEC_SMAX, DEC_LENS,
                                            DEC_SLOTS)
    out = ops.attention_decode(q.to(DEV), kc.to(DEV), vc.to(DEV), st.to(DEV),
                               lt.to(DEV))
    _check_decode(f"decode Hq{Hq} Hkv{Hkv} splits{splits} vd{vdirect}", out,
                  ref, DEC_LENS)


def test_attention_decode_wrapper_picks_one_split(monkeypatch):
    """N = 33, Hkv = 16: 512 // (N * Hkv) == 0, so the wrapper itself chooses
    splits == 1 (no workspaces, direct-store epilogue)."""
    monkeypatch.delenv("KF_DECODE_SPLITS", raising=False)
    monkeypatch.delenv("KF_DECODE_VDIRECT", raising=False)
    N, Hq, Hkv, smax = 33, 16, 16, 64
    assert min(8, max(1, 512 // (N * Hkv))) == 1
    # empty, a full tile, both neighbours, then a spread over 0 .. 64
    lens = [0, 64, 1, 63] + [(11 * i + 5) % 65 for i in range(N - 4)]
    slots = [(5 * i + 3) % N for i in range(N)]    # a permutation
    assert 0 in lens and 64 in lens and sorted(slots) == list(range(N))
    q, kc, vc, st, lt, ref = _decode_inputs(N, Hq, Hkv, smax, lens, slots)
    out = ops.attention_decode(q.to(DEV), kc.to(DEV), vc.to(DEV), st.to(DEV),
                               lt.to(DEV))
    _check_decode("decode wrapper splits=1", out, ref, lens)


# ------------------------------------------------------------- skinny GEMM

def _gemm_inputs(M, N, K, seed=70):
    g = _gen(seed)
    x = (torch.randn(M, 1, K, generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    r = torch.randn(M, 1, N, generator=g).bfloat16()
    return x, w, r


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("M,N,K", [
    # ---- direct-load fallback (K % 512 != 0) ----
    (1, 64, 32),       # kf_skinny_gemm_kernel<8>: one wave has work, tail loop
    (16, 64, 96),      # <8>: three waves have work, full M tile
    (7, 8192, 1056),   # N/16 = 512 -> <4>: unrolled 8-deep loop + tail step
    # ---- LDS-staged templates at the M edges ----
    (17, 64, 512),     # <32>: one row in the second A tile, one K chunk
    (31, 64, 1024),    # <32>: last row of the second tile masked, two chunks
    (32, 16, 512),     # <32>: full tile, a single block
    (16, 16, 512),     # <16>: full tile, a single block
])
def test_skinny_linear_branches(M, N, K, residual):
    x, w, r = _gemm_inputs(M, N, K)
    rg = r.to(DEV) if residual else None
    got = ops.skinny_linear(x.to(DEV), w.to(DEV), residual=rg)
    want = T.linear_residual_oracle(x, w, r if residual else None)
    # test_skinny_gemm_parity's bound, whole and over the M rows
    _both(f"skinny M{M} N{N} K{K} res{int(residual)}", got, want, 2e-2)


@pytest.mark.parametrize("M,N,K", [
    (17, 64, 1024),   # kf_skinny_q8_kernel<32>, one 1024-k chunk
    (1, 16, 2048),    # <16>, two chunks, a single block
])
def test_skinny_q8_branches(M, N, K):
    x, w, r = _gemm_inputs(M, N, K)
    w8, sc = ops.quantize_fp8_rows(w.to(DEV))
    wd = ops.dequantize_fp8_rows(w8, sc, torch.float32)
    got = ops.skinny_linear_q8(x.to(DEV), w8, sc, residual=r.to(DEV))
    want = T.linear_residual_oracle(x, wd, r)
    _both(f"skinny q8 M{M} N{N} K{K}", got, want, 2e-2)


@pytest.mark.parametrize("M,N,K", [
    (33, 64, 512),   # M > 32
    (4, 64, 40),     # K % 32 != 0
    (4, 24, 512),    # N % 16 != 0
    (17, 64, 96),    # M > 16 needs the LDS kernel, K % 512 != 0 rules it out
])
def test_skinny_linear_wrapper_fallbacks_are_exact(M, N, K):
    """Unsupported shapes go to F.linear: bit-equal to the same composed
    expression, with and without residual."""
    x, w, r = (t.to(DEV) for t in _gemm_inputs(M, N, K))
    assert torch.equal(ops.skinny_linear(x, w), F.linear(x, w))
    assert torch.equal(ops.skinny_linear(x, w, residual=r),
                       F.linear(x, w) + r)
