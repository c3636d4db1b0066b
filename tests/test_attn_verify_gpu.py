"""ops.attention_verify (kf_attn_verify) against the fp32 CPU oracle on the
expanded rows, under the project's decode bounds: row_err < 2e-2 over all
rows, rel_err < 2e-2 per sequence, exact zeros where a row sees no key."""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import _backend
from kubeflow_amd.ops import testing as T

pytestmark = pytest.mark.gpu

D, HKV, SMAX = 128, 2, 264
LENS = [0, 1, 31, 32, 33, 127, 128, 129, 200, 256]
SLOTS = [3, 7, 0, 9, 1, 5, 8, 2, 6, 4]
GARBAGE = 1e4  # cache rows no token may see: finite, must not matter
_cache = {}


def _inputs(g, Tn, lens=LENS, slots=SLOTS):
    """(q, kcache, vcache, slots, lens, oracle [N,Tn,Hq,D], vis [N,Tn]), CPU,
    built once per case."""
    key = (g, Tn, tuple(lens))
    if key not in _cache:
        gen = torch.Generator().manual_seed(61)
        N, Hq = len(lens), g * HKV
        q = torch.randn(N, Tn, Hq, D, generator=gen).bfloat16()
        kc = torch.randn(N, SMAX, HKV, D, generator=gen).bfloat16()
        vc = torch.randn(N, SMAX, HKV, D, generator=gen).bfloat16()
        for s, L in zip(slots, lens):
            kc[s, L + Tn - 1:] = GARBAGE
            vc[s, L + Tn - 1:] = GARBAGE
        st = torch.tensor(slots, dtype=torch.int32)
        lt = torch.tensor(lens, dtype=torch.int32)
        vis = lt[:, None] + torch.arange(Tn)
        ref = T.decode_oracle(q.view(N * Tn, Hq, D), kc, vc,
                              st.repeat_interleave(Tn), vis.reshape(-1))
        _cache[key] = (q, kc, vc, st, lt, ref.view(N, Tn, Hq, D), vis)
    return _cache[key]


def _check(name, out, ref, vis):
    out = out.float().cpu()
    row = T.row_err(out, ref)
    worst = max((T.rel_err(out[i], ref[i]) for i in range(len(ref))
                 if int(vis[i, -1]) > 0), default=0.0)
    print(f"PARITY {name} row_err={row:.5f} seq_rel_err={worst:.5f}")
    assert row < 2e-2, (name, row)
    assert worst < 2e-2, (name, worst)
    dark = vis == 0
    assert torch.equal(out[dark], torch.zeros_like(out[dark])), name


# splits 1: direct store; 2, 3: empty slices and slice ends inside a wave's
# stride, combine kernel; 8: the serving default
@pytest.mark.parametrize("splits", [1, 2, 3, 8])
# (4,8): a full 32-row tile; (2,5): rows no multiple of g or 8
@pytest.mark.parametrize("g,Tn", [(4, 8), (4, 1), (1, 8), (8, 4), (2, 5)])
def test_oracle_parity(g, Tn, splits, monkeypatch):
    monkeypatch.setenv("KF_DECODE_SPLITS", str(splits))
    q, kc, vc, st, lt, ref, vis = _inputs(g, Tn)
    q, kc, vc, st, lt = (t.cuda() for t in (q, kc, vc, st, lt))
    out = ops.attention_verify(q, kc, vc, st, lt)
    _check(f"verify g{g} T{Tn} splits{splits}", out, ref, vis)
    # the entry point on NaN-filled output and workspaces: every row and every
    # partial is stored, and the wrapper's result is this one bit for bit
    N, Hq = len(LENS), g * HKV
    nan = lambda *s, dt: torch.full(s, float("nan"), dtype=dt, device="cuda")
    o = nan(N, Tn, Hq, D, dt=torch.bfloat16)
    po = nan(N, Tn * Hq, splits, D, dt=torch.float32)
    pm = nan(N, Tn * Hq, splits, 2, dt=torch.float32)
    err = _backend.require().kf_attn_verify(
        ops._p(o), ops._p(po), ops._p(pm), ops._p(q), ops._p(kc), ops._p(vc),
        ops._i32p(st), ops._i32p(lt), N, Tn, SMAX, Hq, HKV, D, splits,
        D ** -0.5, ops._stream())
    assert err == 0, err
    assert torch.equal(o, out)


@pytest.mark.parametrize("splits", [1, 3])
def test_mask_probe(splits, monkeypatch):
    """Every row's weight sits on its LAST visible key: a draft token that
    sees its successor (mask one key off) moves its row by >= 1.5."""
    monkeypatch.setenv("KF_DECODE_SPLITS", str(splits))
    lens = [1, 31, 32, 33, 128, 129]
    N, Tn, Hq = len(lens), 8, 4 * HKV
    q, k, v, scale = T.mask_probe_inputs(B=N, Sq=Tn, Skv=SMAX, Hq=Hq, Hkv=HKV)
    out = ops.attention_verify(
        q.cuda(), k.cuda(), v.cuda(),
        torch.arange(N, dtype=torch.int32).cuda(),
        torch.tensor(lens, dtype=torch.int32).cuda(), scale=scale)
    last = torch.tensor(lens)[:, None] + torch.arange(Tn) - 1       # [N,Tn]
    want = v[torch.arange(N)[:, None], last].float()         # [N,Tn,Hkv,D]
    want = want.repeat_interleave(Hq // HKV, dim=2)
    err = T.row_err(out, want)
    print(f"PARITY verify mask_probe splits{splits} row_err={err:.5f}")
    assert err < 2e-2, err


def test_t1_against_attention_decode():
    q, kc, vc, st, lt, ref, vis = _inputs(4, 1)
    dev = [t.cuda() for t in (kc, vc, st, lt)]
    _check("verify T1", ops.attention_verify(q.cuda(), *dev), ref, vis)
    dec = ops.attention_decode(q[:, 0].cuda(), *dev)
    _check("decode T1", dec[:, None], ref, vis)


def test_graph_capture_reads_lens_on_device():
    q, kc, vc, st, lt, _, _ = _inputs(4, 8)
    q, kc, vc, st = (t.cuda() for t in (q, kc, vc, st))
    lens = lt.cuda()
    other = torch.tensor(LENS[::-1], dtype=torch.int32).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.attention_verify(q, kc, vc, st, lens)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attention_verify(q, kc, vc, st, lens)
    lens.copy_(other)
    eager = ops.attention_verify(q, kc, vc, st, other)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        assert torch.equal(out, eager)


def test_wrapper_rejects():
    q, kc, vc, st, lt, _, _ = _inputs(4, 8)
    q, kc, vc, st, lt = (t.cuda() for t in (q, kc, vc, st, lt))
    for s, l, exc in ((st.long(), lt, TypeError), (st, lt.long(), TypeError),
                      (st[:-1], lt, ValueError), (st, lt[None], ValueError)):
        with pytest.raises(exc):
            ops.attention_verify(q, kc, vc, s, l)


# beyond the kernel's tile: the reference path, same oracle, same bound
@pytest.mark.parametrize("g,Tn", [(2, 9), (8, 5)])
def test_reference_path_beyond_the_tile(g, Tn):
    lens, slots = [1, 33, 200], [2, 0, 1]
    q, kc, vc, st, lt, ref, vis = _inputs(g, Tn, lens, slots)
    out = ops.attention_verify(q.cuda(), kc.cuda(), vc.cuda(), st.cuda(),
                               lt.cuda())
    _check(f"verify ref-path g{g} T{Tn}", out, ref, vis)
