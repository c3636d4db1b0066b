"""Routed MoE decode on the GPU: the grouped skinny GEMM over device offsets
(skinny_gemm.hip), ops.moe_experts_decode, its replay from a captured graph
under a routing that differs from the captured one, and the serving engine
with KF_MOE_DECODE=routed, in bf16 and with fp8 expert banks.

The grouped kernels are the skinny kernels with a per-block prologue, so each
expert's rows are compared bit for bit with ops.skinny_linear /
ops.skinny_linear_q8 on the same rows; the 2e-2 whole-tensor bounds of
test_skinny_gemm_parity / test_skinny_q8_parity against fp32 F.linear hold on
top. Shapes are the smallest that enter each loop of each kernel:
  LDS kernel     K = 512 (one staged chunk), 1024 (two: both buffers);
                 q8: K = 1024 (one) and 2048 (two)
  direct <8>     K = 96 (tail loop only), 2080 (one pass of the 8-deep
                 unrolled loop, then the tail)
  direct <4>     N = 8192 (N/16 = 512 blocks), K = 1056: one pass of the
                 8-deep loop, then a tail step in wave 0 only; one pattern
  N = 32 and 48: two and three 16-column blocks per expert
  max_rows <= 16 and 17..32: the two M-tile templates.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from kubeflow_amd import models, ops
from kubeflow_amd.models import llama
from kubeflow_amd.ops import _backend
from kubeflow_amd.ops import reference as R
from kubeflow_amd.ops import testing as T

DEV = torch.device("cuda", 0)
E4 = 4
GUARD = 3

# (max_rows, rows per expert). One expert empty; one expert holding all T
# rows for T = 1, 16, 17, 32; all rows on the last expert; one row each.
PATTERNS = [
    (16, (5, 0, 7, 4)), (32, (20, 0, 32, 3)),
    (1, (0, 1, 0, 0)), (16, (0, 16, 0, 0)), (17, (0, 17, 0, 0)),
    (32, (0, 32, 0, 0)),
    (16, (0, 0, 0, 16)), (32, (0, 0, 0, 32)),
    (16, (1, 1, 1, 1)), (32, (1, 1, 1, 1)),
]
PAT_IDS = ["T{}-{}".format(t, "_".join(map(str, c))) for t, c in PATTERNS]
SMALL = [p for p in PATTERNS if p[0] <= 16]
SMALL_IDS = [i for p, i in zip(PATTERNS, PAT_IDS) if p[0] <= 16]


@pytest.fixture(autouse=True)
def _require_native():
    _backend.require()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


_BANKS = {}


def _bank(N, K):
    """Seeded inputs of one (N, K), built once: 64 source rows, the bf16 bank
    and its fp8 form, on the device."""
    if (N, K) not in _BANKS:
        g = _gen(N * 7 + K)
        x = (torch.randn(64, K, generator=g) * 0.5).bfloat16().to(DEV)
        bank = (torch.randn(E4, N, K, generator=g) * K ** -0.5).bfloat16()
        bank = bank.to(DEV)
        w8, sc = ops.quantize_fp8_rows(bank.reshape(E4 * N, K))
        _BANKS[(N, K)] = (x, bank, w8, sc)
    return _BANKS[(N, K)]


def _offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off


def _check_grouped(N, K, max_rows, counts, q8):
    xs, bank, w8, sc = _bank(N, K)
    off = _offsets(counts)
    total = off[-1]
    offsets = torch.tensor(off, dtype=torch.int32, device=DEV)
    # a permutation of token rows with repeats, as MoeRouting.src has
    src = torch.randint(0, 9, (total,), generator=_gen(total + max_rows),
                        dtype=torch.int32).to(DEV)
    deq = ops.dequantize_fp8_rows(w8, sc, torch.float32).view(E4, N, K)
    for rows in (None, src):
        x = xs[:total] if rows is None else xs[:9]
        out = torch.full((total + GUARD, N), float("nan"),
                         dtype=torch.bfloat16, device=DEV)
        if q8:
            got = ops.grouped_skinny_linear_q8(x, w8, sc, offsets, max_rows,
                                               rows, out=out)
        else:
            got = ops.grouped_skinny_linear(x, bank, offsets, max_rows, rows,
                                            out=out)
        assert got is out
        want32 = torch.zeros(total, N, device=DEV)
        for e in range(E4):
            lo, m = off[e], counts[e]
            if m == 0:
                continue
            xr = x[lo:lo + m] if rows is None else x[rows[lo:lo + m].long()]
            if q8:
                ref = ops.skinny_linear_q8(xr, w8[e * N:(e + 1) * N],
                                           sc[e * N:(e + 1) * N])
                want32[lo:lo + m] = F.linear(xr.float(), deq[e])
            else:
                ref = ops.skinny_linear(xr, bank[e])
                want32[lo:lo + m] = F.linear(xr.float(), bank[e].float())
            assert torch.equal(out[lo:lo + m], ref), (e, rows is None)
        assert bool(torch.isfinite(out[:total]).all())
        assert bool(torch.isnan(out[total:]).all())      # guard rows untouched
        err = T.rel_err(out[:total], want32)
        print(f"grouped{'_q8' if q8 else ''} N{N} K{K} T{max_rows} {counts} "
              f"rows={'src' if rows is not None else 'None'}: rel_err "
              f"{err:.3e} (bound 2e-2)")
        assert err < 2e-2


@pytest.mark.parametrize("pat", PATTERNS, ids=PAT_IDS)
@pytest.mark.parametrize("N", [32, 48])
@pytest.mark.parametrize("K", [512, 1024])
def test_grouped_lds_kernel_matches_skinny_linear_bits(K, N, pat):
    _check_grouped(N, K, pat[0], pat[1], q8=False)


# every small pattern at the <8> shapes, one at the <4> shape; the ids are
# those of the stacked pat / N / K parametrisation this list replaces
DIRECT = [(K, N, p, i) for K in (96, 2080) for N in (32, 48)
          for p, i in zip(SMALL, SMALL_IDS)]
DIRECT.append((1056, 8192, SMALL[0], SMALL_IDS[0]))


@pytest.mark.parametrize("K,N,pat", [c[:3] for c in DIRECT],
                         ids=["{0}-{1}-{3}".format(*c) for c in DIRECT])
def test_grouped_direct_kernel_matches_skinny_linear_bits(K, N, pat):
    _check_grouped(N, K, pat[0], pat[1], q8=False)


@pytest.mark.parametrize("pat", PATTERNS, ids=PAT_IDS)
@pytest.mark.parametrize("N", [32, 48])
@pytest.mark.parametrize("K", [1024, 2048])
def test_grouped_q8_kernel_matches_skinny_linear_q8_bits(K, N, pat):
    _check_grouped(N, K, pat[0], pat[1], q8=True)


def test_shapes_the_kernel_rejects_take_the_reference():
    """K = 96 with 17 rows has no kernel (the direct kernel stops at 16): the
    op runs the reference loop instead of failing, and agrees with it."""
    xs, bank, _, _ = _bank(32, 96)
    assert not ops.grouped_skinny_ok(17, 32, 96, torch.bfloat16)
    off = torch.tensor([0, 17, 17, 17, 20], dtype=torch.int32, device=DEV)
    got = ops.grouped_skinny_linear(xs[:20], bank, off, 17)
    assert torch.equal(got, R.grouped_linear_offsets(xs[:20], bank, off))


# ----------------------------------------------------------- whole block --

BT, BE, BK, BH = 8, 8, 2, 512


def _block_inputs():
    g = _gen(77)
    x = (torch.randn(BT, BH, generator=g)).bfloat16()
    gate = (torch.randn(BE, BH, generator=g) * 0.05).bfloat16()
    w13 = (torch.randn(BE, 2 * BH, BH, generator=g) * 0.05).bfloat16()
    w2 = (torch.randn(BE, BH, BH, generator=g) * 0.05).bfloat16()
    dout = torch.randn(BT, BH, generator=g).bfloat16()
    return x, gate, w13, w2, dout


def test_block_matches_moe_experts_and_the_fp32_oracle():
    x, gate, w13, w2, dout = _block_inputs()
    xd, w13d, w2d = x.to(DEV), w13.to(DEV), w2.to(DEV)
    logits = F.linear(xd, gate.to(DEV))
    got = ops.moe_experts_decode(xd, logits, w13d, w2d, BK)
    again = ops.moe_experts_decode(xd, logits, w13d, w2d, BK)
    with torch.no_grad():
        sync = ops.moe_experts(xd, logits, w13d, w2d, BK)
    assert torch.equal(got, again)
    # oracle and bound on the CPU, routing from the logits the kernels saw
    topi = R.moe_route(logits.cpu(), BK)[0]
    oracle = T.moe_mlp_oracle(x, gate, w13, w2, topi, dout)[0]
    emu = T.moe_mlp_emulated(x, gate, w13, w2, topi, dout)[0]
    bound = T.ROW_BOUND_FACTOR * T.row_err(emu, oracle)
    for name, ref in (("moe_experts", sync), ("oracle", oracle)):
        rel, per_row = T.rel_err(got, ref), T.row_err(got, ref)
        print(f"moe_experts_decode vs {name}: rel_err {rel:.3e} (bound 2e-2),"
              f" per-row {per_row:.3e} (bound {bound:.3e})")
        assert rel < 2e-2, name
        assert per_row < bound, name


def _logits_pair(lo):
    """[BT, BE] logits that send every token to experts {lo, lo + 1}."""
    lg = torch.randn(BT, BE, generator=_gen(lo + 1))
    lg[:, lo:lo + 2] += 100.0
    return lg.bfloat16()


def _logits_spread():
    """Token t on experts t % 8 and (t + 3) % 8: two rows on every expert."""
    lg = torch.zeros(BT, BE)
    for t in range(BT):
        lg[t, t % BE] = 5.0
        lg[t, (t + 3) % BE] = 4.0
    return lg.bfloat16()


def test_graph_replay_follows_routing_that_differs_from_capture():
    """Captured while experts 2..7 were empty; replayed with every expert in
    use and with only {6, 7}: each replay must give the bits of an eager
    call on the same inputs."""
    x, _, w13, w2, _ = _block_inputs()
    w13d, w2d = w13.to(DEV), w2.to(DEV)
    sx = x.to(DEV).clone()
    slg = _logits_pair(0).to(DEV)
    off = ops.moe_route(slg, BK, sync=False).offsets.tolist()
    assert off == [0, BT, 2 * BT] + [2 * BT] * (BE - 2)
    # the capture pattern of InferenceEngine._graph_for
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.moe_experts_decode(sx, slg, w13d, w2d, BK)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sout = ops.moe_experts_decode(sx, slg, w13d, w2d, BK)
    graph.replay()
    captured = sout.clone()
    assert torch.equal(captured,
                       ops.moe_experts_decode(sx, slg, w13d, w2d, BK))
    x2 = torch.randn(BT, BH, generator=_gen(5)).bfloat16().to(DEV)
    for name, lg, xn in (("spread", _logits_spread(), sx.clone()),
                         ("pair67", _logits_pair(6), x2)):
        lg = lg.to(DEV)
        counts = ops.moe_route(lg, BK, sync=False).offsets.diff().tolist()
        if name == "spread":
            assert counts == [2] * BE
        else:
            assert counts == [0] * 6 + [BT, BT]
        eager = ops.moe_experts_decode(xn, lg, w13d, w2d, BK)
        sx.copy_(xn)
        slg.copy_(lg)
        graph.replay()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(sout).all()), name
        assert torch.equal(sout, eager), name
        assert not torch.equal(sout, captured), name


# ---------------------------------------------------------------- engine --

def test_engine_routed_decode_under_graphs(monkeypatch):
    """llama-moe-tiny has h = 256, f = 512: w13 (K = 256) takes the direct
    kernel and w2 (K = 512) the LDS kernel."""
    from kubeflow_amd.runtime.serving import InferenceEngine, Request

    monkeypatch.setenv("KF_MOE_DECODE", "routed")
    monkeypatch.setenv("KF_PREFIX_CACHE", "0")
    monkeypatch.delenv("KF_SERVE_GRAPH", raising=False)
    monkeypatch.delenv("KF_SERVE_QUANT", raising=False)
    torch.manual_seed(13)
    eng = InferenceEngine("llama-moe-tiny", max_slots=4, smax=128,
                          max_batch=4)
    assert eng.use_graphs
    probe = torch.empty(4, 1, 256, device=DEV, dtype=torch.bfloat16)
    assert all(l.moe.routed_decode_ok(probe) for l in eng.model.layers)
    eng.start()
    try:
        p1, p2 = [5, 3, 8, 1, 9], [7, 2, 11, 4, 6, 13, 10]
        r = eng.generate(p1, max_new_tokens=4, timeout=120)
        assert not r.error and len(r.generated) == 4
        with torch.no_grad():
            full = eng.model(torch.tensor([p1], device=DEV))
        assert r.generated[0] == int(full[0, -1].argmax())
        assert eng.stats["graph_replays"] > 0
        # two requests in flight (prompts of different length, so each
        # prefills alone) reproduce their single-request greedy output
        a1 = eng.generate(p1, max_new_tokens=8, timeout=120)
        a2 = eng.generate(p2, max_new_tokens=8, timeout=120)
        assert not a1.error and not a2.error
        b1 = eng.submit(Request(rid="b1", prompt=list(p1), max_new_tokens=8))
        b2 = eng.submit(Request(rid="b2", prompt=list(p2), max_new_tokens=8))
        assert b1.done.wait(120) and b2.done.wait(120)
        assert not b1.error and not b2.error
        assert b1.generated == a1.generated
        assert b2.generated == a2.generated
    finally:
        eng.stop()


def _moe_module(h, f, E, seed):
    cfg = llama.LlamaConfig(name="moe-q8-test", vocab_size=512,
                            hidden_size=h, n_layers=1, n_heads=h // 128,
                            n_kv_heads=2, ffn_dim=f, max_seq_len=256,
                            n_experts=E, top_k=2)
    moe = llama.MoEMLP(cfg)
    g = _gen(seed)
    with torch.no_grad():
        for p in moe.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.03)
    return cfg, moe.to(device=DEV, dtype=torch.bfloat16)


def test_decode_routed_fp8_banks_match_the_dequantized_module():
    """h = f = 1024 (K % 1024 for both banks), E = 4: the routed block on fp8
    banks against the same module holding the dequantized weights, under the
    2e-2 bound of test_skinny_q8_parity."""
    from kubeflow_amd.runtime.serving import quantize_moe_banks

    cfg, moe = _moe_module(1024, 1024, 4, 31)
    x = torch.randn(8, 1, 1024, generator=_gen(32)).bfloat16().to(DEV)
    assert moe.routed_decode_ok(x, q8=True)
    q8 = quantize_moe_banks(moe)
    (w13_8, s13), (w2_8, s2) = q8
    assert w13_8.shape == (4 * 2048, 1024) and s13.shape == (4 * 2048,)
    assert w2_8.shape == (4 * 1024, 1024) and s2.shape == (4 * 1024,)
    with torch.no_grad():
        got = moe.decode_routed(x, q8=q8)
        moe.experts_w13.copy_(ops.dequantize_fp8_rows(w13_8, s13).view(
            moe.experts_w13.shape))
        moe.experts_w2.copy_(ops.dequantize_fp8_rows(w2_8, s2).view(
            moe.experts_w2.shape))
        want = moe.decode_routed(x)
        dense = moe.decode_dense(x)
    err = T.rel_err(got, want)
    print(f"decode_routed fp8 vs dequantized bf16: rel_err {err:.3e}, routed "
          f"vs dense (bf16) {T.rel_err(want, dense):.3e} (bounds 2e-2)")
    assert err < 2e-2
    assert T.rel_err(want, dense) < 2e-2


def test_engine_keeps_fp8_on_for_a_qualifying_moe_model(monkeypatch):
    """The engine takes model names: a config with h = f = 1024 is registered
    for the test. fp8 stays on with the routed path, and goes off (today's
    behaviour) under the dense path or with shapes the q8 kernel rejects."""
    from kubeflow_amd.runtime.serving import InferenceEngine

    def cfg_fn():
        return llama.LlamaConfig(name="llama-moe-q8-test", vocab_size=512,
                                 hidden_size=1024, n_layers=1, n_heads=8,
                                 n_kv_heads=2, ffn_dim=1024, max_seq_len=256,
                                 n_experts=4, top_k=2)

    monkeypatch.setitem(models.MODEL_REGISTRY, "llama-moe-q8-test",
                        models._llama(cfg_fn))
    monkeypatch.setenv("KF_MOE_DECODE", "routed")
    torch.manual_seed(5)
    eng = InferenceEngine("llama-moe-q8-test", max_slots=4, smax=128,
                          max_batch=4, quant="fp8")
    assert eng.quant is True
    assert set(eng._qw[0]) == {"wqkv", "wo", "moe"}
    (w13_8, s13), (w2_8, s2) = eng._qw[0]["moe"]
    assert w13_8.dtype == torch.uint8 and w13_8.shape == (4 * 2048, 1024)
    assert s2.shape == (4 * 1024,)
    eng.start(precapture=False)
    try:
        r = eng.generate([5, 3, 8, 1, 9], max_new_tokens=3, timeout=120)
        assert not r.error and len(r.generated) == 3
        assert eng.stats["graph_replays"] > 0
    finally:
        eng.stop()
    tiny = InferenceEngine("llama-moe-tiny", max_slots=4, smax=128,
                           max_batch=4, quant="fp8")
    assert tiny.quant is False and tiny._qw is None
    monkeypatch.setenv("KF_MOE_DECODE", "dense")
    dense = InferenceEngine("llama-moe-q8-test", max_slots=4, smax=128,
                            max_batch=4, quant="fp8")
    assert dense.quant is False and dense._qw is None
