"""moe.hip on the GPU against ops/reference.py run on the CPU.

Everything that is a copy, an exact product or a fixed-order fp32 sum (topi,
the sort, gather, gather_bwd, combine, dy, and the zero entries of dw and
dlogits) is compared bit for bit and run twice; the two reductions of
unspecified lane order (dw, dlogits) are held to bounds derived from the
formats; the whole block is held to the per-row rule of docs/KERNELS.md.

Shapes: one wave handles a row and a block has four, so T = 8300 (and its
16600 permuted rows) exceeds the 2048-block grid cap for every row kernel;
2100 x 2 rows do so for a one-row-per-block reading of the cap. 1500 x 2 pairs
span three 1024-pair count chunks with a partial last one; E = 64 / k = 8 and
h = 2048 are the width limits, T = 1 the partial wave.

Measured maxima on one MI355X (also in docs/KERNELS.md): topw 3.9e-3 relative
(bound 2^-7), probs 1.7e-7 (bound 1e-6), dw and dlogits 0.99 of their bounds
(one bf16 rounding at its worst case). In the one_expert variant slot 1 holds
exp(-98) ~ 3e-43, a subnormal of both output formats: measured 19% relative
error in probs (less than one fp32 quantum 2^-149) and topw flushed to 0, which
no kernel can improve, so test_route bounds references below 2^-126 by one
quantum of the format and everything else by the relative bounds.
"""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.models import llama
from kubeflow_amd.ops import _backend
from kubeflow_amd.ops import reference as R
from kubeflow_amd.ops import testing as T

DEV = torch.device("cuda", 0)
INF = float("inf")

SHAPES = [(1, 4, 2, 256), (333, 8, 2, 256), (1500, 8, 2, 64),
          (2100, 8, 2, 128), (257, 64, 8, 64), (200, 4, 2, 2048),
          (8300, 4, 2, 64)]
CASES = []
for _s in SHAPES:
    for _v in ("plain", "one_expert", "empty_expert"):
        CASES.append((*_s, _v, 0, _s[1]))
    if _s[1] == 4:
        CASES += [(*_s, "plain", 0, 2), (*_s, "plain", 2, 2)]
IDS = ["T{}-E{}-k{}-h{}-{}-lo{}n{}".format(*c) for c in CASES]


@pytest.fixture(autouse=True)
def _require_native():
    _backend.require()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _tie_rows(E, k):
    """[3, E]: all equal; rank k tied with rank k + 1 (the lower index must
    take the last slot); one finite value among -inf."""
    equal = torch.ones(E)
    tie = torch.arange(E, dtype=torch.float32)
    tie[E - k - 1] = tie[E - k] if k < E else tie[0]
    ninf = torch.full((E,), -INF)
    ninf[E // 2 + 1] = 2.0
    return torch.stack([equal, tie, ninf])


def _logits(Tn, E, k, variant, seed):
    lg = torch.randn(Tn, E, generator=_gen(seed))
    if variant == "one_expert":
        lg[:, 1] += 100.0
    elif variant == "empty_expert":
        lg[:, 2] = -INF
    elif Tn >= 4:
        lg[:3] = _tie_rows(E, k)
    return lg.bfloat16()


def _gpu_run(c, lg_cpu, x, dxp, y, dout, dw_up):
    """Every kernel once, through the public ops. Returns CPU tensors."""
    Tn, E, k, h, _, e_lo, n_local = c
    lg = lg_cpu.to(DEV).requires_grad_(True)
    r = ops.moe_route(lg, k, e_lo, n_local)
    M = r.rows
    xg = x.to(DEV).requires_grad_(True)
    xp = ops.moe_gather(xg, r)
    xp.backward(dxp[:M].to(DEV))
    yg = y[:M].to(DEV).requires_grad_(True)
    wleaf = r.topw.detach().clone().requires_grad_(True)
    out = ops.moe_combine(yg, dataclasses.replace(r, topw=wleaf))
    out.backward(dout.to(DEV))
    r.topw.backward(dw_up.to(DEV))
    torch.cuda.synchronize()
    res = dict(topi=r.topi, topw=r.topw.detach(), probs=r.probs, pos=r.pos,
               src=r.src[:M], offsets=r.offsets, xp=xp.detach(), dx=xg.grad,
               out=out.detach(), dy=yg.grad, dw=wleaf.grad, dlogits=lg.grad)
    res = {n: t.cpu() for n, t in res.items()}
    res["splits"] = r.splits
    return res


_RUNS = {}


def _run(c):
    """Inputs, two GPU runs and the CPU reference of one case, computed
    once."""
    if c in _RUNS:
        return _RUNS[c]
    Tn, E, k, h, variant, e_lo, n_local = c
    seed = Tn * 7 + E
    g = _gen(seed + 1)
    lg = _logits(Tn, E, k, variant, seed)
    x = torch.randn(Tn, h, generator=g).bfloat16()
    dxp = torch.randn(Tn * k, h, generator=g).bfloat16()
    y = torch.randn(Tn * k, h, generator=g).bfloat16()
    dout = torch.randn(Tn, h, generator=g).bfloat16()
    dw_up = torch.randn(Tn, k, generator=g).bfloat16()
    a = _gpu_run(c, lg, x, dxp, y, dout, dw_up)
    b = _gpu_run(c, lg, x, dxp, y, dout, dw_up)
    # reference, downstream of the GPU's own routing values (topw may differ
    # from the CPU's by a bf16 ulp; the route test bounds that separately)
    M = sum(a["splits"])
    pos, src, offsets = R.moe_sort(a["topi"], e_lo, n_local)
    ref = dict(pos=pos, src=src[:M], offsets=offsets,
               xp=R.moe_gather(x, src, M),
               dx=R.moe_gather_bwd(dxp[:M], pos),
               out=R.moe_combine(y[:M], a["topw"], pos))
    ref["dy"], ref["dw"] = R.moe_combine_bwd(dout, y[:M], a["topw"], pos)
    ref["dlogits"] = R.moe_route_bwd(dw_up, a["probs"], a["topi"], E)
    _RUNS[c] = dict(inputs=(lg, x, dxp, y, dout, dw_up), a=a, b=b, ref=ref,
                    M=M)
    return _RUNS[c]


def _biteq(a, b):
    """Same bits (NaN-free tensors): torch.equal plus the sign of zeros."""
    return torch.equal(a, b) and torch.equal(torch.signbit(a.float()),
                                             torch.signbit(b.float()))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_route(c):
    Tn, E, k, h, variant, e_lo, n_local = c
    run = _run(c)
    lg = run["inputs"][0]
    a = run["a"]
    topi_ref, _, _ = R.moe_route(lg, k)
    assert torch.equal(a["topi"], topi_ref)
    if variant == "plain" and Tn >= 4:
        want = _tie_rows(E, k).sort(dim=-1, descending=True,
                                    stable=True).indices[:, :k]
        assert torch.equal(a["topi"][:3].long(), want)
    sel = lg.double().gather(1, a["topi"].long())
    ref = torch.softmax(sel, dim=-1)
    err_w = (a["topw"].double() - ref).abs()
    err_p = (a["probs"].double() - ref).abs()
    print(f"route {IDS[CASES.index(c)]}: max topw err/ref "
          f"{(err_w / ref.clamp_min(1e-300)).max().item():.3e} (bound "
          f"{2 ** -7:.3e}), probs {(err_p / ref.clamp_min(1e-300)).max().item():.3e}"
          " (bound 1e-6)")
    # A probability below 2^-126 is a subnormal in both output formats (the
    # one_expert variant puts exp(-98) ~ 3e-43 in slot 1): there one ulp is
    # the format's fixed quantum, 2^-133 in bf16 and 2^-149 in fp32, and no
    # kernel can be relatively more accurate than that. Everywhere else the
    # bounds are the relative ones.
    sub = (ref < 2.0 ** -126).double()
    assert bool((err_w <= 2.0 ** -7 * ref + sub * 2.0 ** -133).all())
    assert bool((err_p <= 1e-6 * ref + sub * 2.0 ** -149).all())
    assert torch.equal(a["topw"], a["probs"].bfloat16())


@pytest.mark.parametrize("E,k", [(4, 2), (8, 2), (64, 8), (8, 8), (2, 1)])
def test_route_is_memory_safe_on_nan_inf_and_equal_rows(E, k):
    lg = torch.randn(70, E, generator=_gen(E + k))
    lg[0, 1] = float("nan")
    lg[1] = float("nan")
    lg[2] = INF
    lg[3] = -INF
    lg[4] = 0.0
    lg[5, ::2] = float("nan")
    lg[6, 0], lg[6, 1] = 0.0, -0.0
    r = ops.moe_route(lg.bfloat16().to(DEV), k)
    topi = r.topi.cpu()
    assert bool(((topi >= 0) & (topi < E)).all())
    assert bool((topi.sort(dim=-1).values.diff(dim=-1) > 0).all())  # distinct
    pos = r.pos.cpu().reshape(-1).long()
    assert sorted(pos.tolist()) == list(range(70 * k))
    # rows without a NaN follow the stable descending sort
    ok = ~torch.isnan(lg).any(dim=1)
    assert torch.equal(topi[ok], R.moe_route(lg.bfloat16(), k)[0][ok])


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_sort_gather_combine_match_reference_bits(c):
    Tn, E, k, h, variant, e_lo, n_local = c
    run = _run(c)
    a, b, ref = run["a"], run["b"], run["ref"]
    off = ref["offsets"].tolist()
    assert a["splits"] == tuple(off[i + 1] - off[i] for i in range(n_local))
    if variant == "one_expert" and e_lo == 0:
        assert a["splits"][1] == Tn
    if variant == "empty_expert":
        assert a["splits"][2] == 0
    for name in ("pos", "src", "offsets"):
        assert torch.equal(a[name], ref[name]), name
    for name in ("xp", "dx", "out", "dy"):
        assert _biteq(a[name], ref[name]), name
    no_local = (ref["pos"] < 0).all(dim=1)
    assert bool((a["dx"][no_local] == 0).all())
    assert bool((a["out"][no_local] == 0).all())
    # zero entries of dw (slots that are not local) and of dlogits
    assert bool((a["dw"][ref["pos"] < 0] == 0).all())
    unrouted = torch.ones(Tn, E, dtype=torch.bool)
    unrouted.scatter_(1, a["topi"].long(), False)
    assert bool((a["dlogits"][unrouted] == 0).all())
    assert not bool(torch.signbit(a["dlogits"][unrouted].float()).any())
    # the same inputs give the same bits, in every output
    for name in a:
        if name != "splits":
            assert _biteq(a[name], b[name]), name


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_combine_bwd_dw_within_derived_bound(c):
    run = _run(c)
    _, _, _, y, dout, _ = run["inputs"]
    a, pos = run["a"], run["ref"]["pos"].long()
    M = run["M"]
    if M == 0:
        return
    rows = y[:M].double()[pos.clamp_min(0)]              # [T, k, h]
    prod = dout.double().unsqueeze(1) * rows
    live = (pos >= 0)
    ref = prod.sum(dim=-1) * live
    mag = prod.abs().sum(dim=-1) * live
    err = (a["dw"].double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * mag
    print(f"dw {IDS[CASES.index(c)]}: max err/bound "
          f"{(err / bound.clamp_min(1e-300))[live].max().item():.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_route_bwd_dlogits_within_derived_bound(c):
    Tn, E, k, h, variant, e_lo, n_local = c
    run = _run(c)
    dw_up = run["inputs"][5].double()
    a = run["a"]
    p = a["probs"].double()
    g = p * (dw_up - (p * dw_up).sum(dim=-1, keepdim=True))
    mag = (p * dw_up.abs()).sum(dim=-1, keepdim=True).expand(Tn, k)
    got = a["dlogits"].double().gather(1, a["topi"].long())
    err = (got - g).abs()
    bound = 2.0 ** -8 * g.abs() + 2.0 ** -20 * mag
    print(f"dlogits {IDS[CASES.index(c)]}: max err/bound "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    # and the CPU reference (fp32, its own summation order) agrees to a bf16
    # ulp of the same bound
    ref = run["ref"]["dlogits"].double().gather(1, a["topi"].long())
    assert bool(((got - ref).abs() <= 2 * bound).all())


# ----------------------------------------------------------- whole block --

def _block_inputs():
    cfg = llama.llama_moe_tiny()          # E = 4, k = 2, h = 256, f = 512
    g = _gen(99)
    moe = llama.MoEMLP(cfg)
    with torch.no_grad():
        for p in moe.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    moe = moe.to(device=DEV, dtype=torch.bfloat16)
    x = torch.randn(2, 167, cfg.hidden_size, generator=g).bfloat16()
    dout = torch.randn(2, 167, cfg.hidden_size, generator=g).bfloat16()
    return cfg, moe, x, dout


def _block_run(moe, x, dout):
    captured = []
    hook = moe.gate.register_forward_hook(
        lambda mod, inp, out: captured.append(out.detach()))
    moe.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    out = moe(xg)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    hook.remove()
    assert len(captured) == 1
    res = dict(out=out.detach(), dx=xg.grad, gate=moe.gate.weight.grad,
               w13=moe.experts_w13.grad, w2=moe.experts_w2.grad)
    return {n: t.cpu().clone() for n, t in res.items()}, captured[0].cpu()


def test_whole_block_bf16(monkeypatch):
    cfg, moe, x, dout = _block_inputs()
    monkeypatch.delenv("KF_MOE_NATIVE", raising=False)
    got, logits = _block_run(moe, x, dout)
    again, logits2 = _block_run(moe, x, dout)
    monkeypatch.setenv("KF_MOE_NATIVE", "0")
    loop, logits3 = _block_run(moe, x, dout)
    assert torch.equal(logits, logits2) and torch.equal(logits, logits3)

    # routing for the oracle from the captured logits, on the CPU
    topi = R.moe_route(logits, cfg.top_k)[0]
    top = logits.float().sort(dim=-1, descending=True).values
    ties = int((top[:, cfg.top_k - 1] == top[:, cfg.top_k]).sum())
    h = cfg.hidden_size
    args = (x.reshape(-1, h), moe.gate.weight, moe.experts_w13,
            moe.experts_w2, topi, dout.reshape(-1, h))
    names = ("out", "dx", "gate", "w13", "w2")
    oracle = dict(zip(names, T.moe_mlp_oracle(*args)))
    emu = dict(zip(names, T.moe_mlp_emulated(*args)))
    for n in names:
        metric = T.row_err if n in ("out", "dx") else T.col_err
        ref = oracle[n].reshape(got[n].shape)
        bound = T.ROW_BOUND_FACTOR * metric(emu[n].reshape(got[n].shape), ref)
        rel, per_row = T.rel_err(got[n], ref), metric(got[n], ref)
        rel_loop = T.rel_err(got[n], loop[n])
        print(f"moe block {n}: rel_err {rel:.3e} (bound 2e-2), per-row "
              f"{per_row:.3e} (bound {bound:.3e}), native vs loop "
              f"{rel_loop:.3e}; rows tied at the top-k edge: {ties}")
        assert rel < 2e-2, n
        assert per_row < bound, n
        # the loop path routes with torch.topk; on a row tied at the edge of
        # the top-k it may pick the other expert, which the whole-tensor
        # metric absorbs
        assert rel_loop < 2e-2, n
        # two native runs: identical bits, in the output and every gradient
        assert torch.equal(got[n], again[n]), n
