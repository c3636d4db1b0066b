"""ops.attention_prefill (kf_attn_prefill) against the fp32 CPU oracle on the
expanded rows, under the project's decode bounds: row_err < 2e-2 over all
rows, rel_err < 2e-2 per sequence, exact zeros where a row sees no key."""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import _backend
from kubeflow_amd.ops import testing as T

pytestmark = pytest.mark.gpu

D, HKV, SMAX, NSLOTS = 128, 2, 400, 12
# (C, lens): around a wave's and a block's rows at every g and a 64-key tile
# edge; a first token; lens = 0 (first row sees nothing); an empty range
SEQS = [(1, 1), (5, 1), (33, 1), (130, 1), (31, 64), (32, 65), (65, 200),
        (16, 0), (0, 7)]
SLOTS = [3, 7, 0, 9, 1, 11, 8, 2, 6]
VERIFY_LENS = [0, 1, 31, 32, 33, 127, 128, 129, 200, 256]  # verify's LENS
GARBAGE = 1e4  # cache rows no token may see: finite, must not matter
PAD = 2        # rows of q / out in front of the first range, and one behind
_cache = {}


def _inputs(g, seqs=SEQS, slots=SLOTS):
    """(..., oracle [R,Hq,D], vis [R], seq id [R], -1 outside every range)"""
    key = (g, tuple(seqs))
    if key not in _cache:
        gen = torch.Generator().manual_seed(67)
        Hq, R = g * HKV, PAD + sum(c for c, _ in seqs) + 1
        q = torch.randn(R, Hq, D, generator=gen).bfloat16()
        kc = torch.randn(NSLOTS, SMAX, HKV, D, generator=gen).bfloat16()
        vc = torch.randn(NSLOTS, SMAX, HKV, D, generator=gen).bfloat16()
        starts, vis, sid, rslot = [PAD], [0] * PAD, [-1] * PAD, [0] * PAD
        for n, ((c, L), s) in enumerate(zip(seqs, slots)):
            kc[s, max(L + c - 1, 0):] = GARBAGE
            vc[s, max(L + c - 1, 0):] = GARBAGE
            starts.append(starts[-1] + c)
            vis += [L + i for i in range(c)]
            sid += [n] * c
            rslot += [s] * c
        vis, sid, rslot = (torch.tensor(x + [0]) for x in (vis, sid, rslot))
        sid[-1] = -1
        ref = T.decode_oracle(q, kc, vc, rslot, vis)
        i32 = lambda x: torch.tensor(x, dtype=torch.int32)
        _cache[key] = (q, kc, vc, i32(slots[:len(seqs)]), i32(starts),
                       i32([L for _, L in seqs]), ref, vis, sid)
    return _cache[key]


def _check(name, out, ref, vis, sid):
    out = out.float().cpu()
    cov = sid >= 0
    row = T.row_err(out[cov], ref[cov])
    worst = max(T.rel_err(out[sid == n], ref[sid == n])
                for n in sid[cov].unique().tolist())
    print(f"PARITY {name} row_err={row:.5f} seq_rel_err={worst:.5f}")
    assert row < 2e-2, (name, row)
    assert worst < 2e-2, (name, worst)
    dark = cov & (vis == 0)
    assert torch.equal(out[dark], torch.zeros_like(out[dark])), name


# 256 > max C = 130: the grid's tail blocks are wholly empty
@pytest.mark.parametrize("max_rows", [130, 256])
@pytest.mark.parametrize("g", [1, 2, 4, 8])
def test_oracle_parity(g, max_rows):
    q, kc, vc, st, ss, lt, ref, vis, sid = _inputs(g)
    q, kc, vc, st, ss, lt = (t.cuda() for t in (q, kc, vc, st, ss, lt))
    out = ops.attention_prefill(q, kc, vc, st, ss, lt, max_rows)
    _check(f"prefill g{g} max_rows{max_rows}", out, ref, vis, sid)
    # raw entry point, NaN-filled out: covered rows stored, no others
    o = torch.full_like(q, float("nan"))
    err = _backend.require().kf_attn_prefill(
        ops._p(o), ops._p(q), ops._p(kc), ops._p(vc), ops._i32p(st),
        ops._i32p(ss), ops._i32p(lt), len(SEQS), q.shape[0], max_rows, SMAX,
        NSLOTS, g * HKV, HKV, D, D ** -0.5, ops._stream())
    assert err == 0, err
    cov = (sid >= 0).cuda()
    assert torch.isfinite(o[cov].float()).all()
    assert torch.equal(o[cov], out[cov])
    assert torch.isnan(o[~cov].float()).all()


def test_mask_probe():
    """All weight on the LAST visible key: a mask one key off reads >= 1.5."""
    lens, C, Hq = [1, 31, 32, 33, 64, 65, 129], 40, 4 * HKV
    N = len(lens)
    q, k, v, scale = T.mask_probe_inputs(B=N, Sq=C, Skv=200, Hq=Hq, Hkv=HKV)
    out = ops.attention_prefill(
        q.view(N * C, Hq, D).cuda(), k.cuda(), v.cuda(),
        torch.arange(N, dtype=torch.int32).cuda(),
        (torch.arange(N + 1, dtype=torch.int32) * C).cuda(),
        torch.tensor(lens, dtype=torch.int32).cuda(), C, scale=scale)
    last = torch.tensor(lens)[:, None] + torch.arange(C) - 1        # [N,C]
    want = v[torch.arange(N)[:, None], last].float()          # [N,C,Hkv,D]
    want = want.repeat_interleave(Hq // HKV, dim=2).view(N * C, Hq, D)
    err = T.row_err(out, want)
    print(f"PARITY prefill mask_probe row_err={err:.5f}")
    assert err < 2e-2, err


def test_t8_is_verify_contract():
    seqs = [(8, L) for L in VERIFY_LENS]
    q, kc, vc, st, ss, lt, ref, vis, sid = _inputs(4, seqs, SLOTS + [4])
    out = ops.attention_prefill(q.cuda(), kc.cuda(), vc.cuda(), st.cuda(),
                                ss.cuda(), lt.cuda(), 8)
    _check("prefill T8", out, ref, vis, sid)


def test_graph_capture_reads_index_tensors_on_device():
    q, kc, vc, st, ss, lt, _, _, _ = _inputs(4)
    q, kc, vc, st, ss, lt = (t.cuda() for t in (q, kc, vc, st, ss, lt))
    counts = [c for c, _ in SEQS][::-1]
    ss2 = torch.tensor([PAD] + counts, dtype=torch.int32).cumsum(0).int()
    st2, lt2 = st.flip(0).contiguous(), (lt + 3).contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.attention_prefill(q, kc, vc, st, ss, lt, 130)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attention_prefill(q, kc, vc, st, ss, lt, 130)
    for t, other in ((st, st2), (ss, ss2), (lt, lt2)):
        t.copy_(other)
    eager = ops.attention_prefill(q, kc, vc, st2, ss2.cuda(), lt2, 130)
    cov = slice(PAD, q.shape[0] - 1)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        assert torch.equal(out[cov], eager[cov])


def test_wrapper_rejects():
    q, kc, vc, st, ss, lt, _, _, _ = _inputs(4)
    q, kc, vc, st, ss, lt = (t.cuda() for t in (q, kc, vc, st, ss, lt))
    for a, b, c, exc in (
            (st.long(), ss, lt, TypeError), (st, ss.long(), lt, TypeError),
            (st, ss, lt.long(), TypeError), (st[:-1], ss, lt, ValueError),
            (st, ss[:-1], lt, ValueError), (st, ss, lt[None], ValueError)):
        with pytest.raises(exc):
            ops.attention_prefill(q, kc, vc, a, b, c, 130)
