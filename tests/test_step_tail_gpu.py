"""Step tail and residual backward on the GPU: kf_grad_sumsq, kf_adamw_clip
and kf_rmsnorm_bwd_res against the passes they replace.

Bit equality wherever the parent sequence is deterministic: the clip multiply
and the compact decay mask folded into AdamW reproduce grad.mul_(scale) +
kf_adamw with the fp32 mask, and the residual add folded into the norm
backward reproduces kf_rmsnorm_bwd + a torch bf16 add. The gradient norm only
changes its summation order and is held to a derived bound instead.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from kubeflow_amd import ops
from kubeflow_amd.ops import _backend
from kubeflow_amd.ops import testing as T

DEV = torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_native():
    _backend.require()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ---------------------------------------------------------- kf_grad_sumsq

# one grid pass of stage one: 2048 blocks x 256 threads x 8 elements
_PASS = 2048 * 256 * 8

SUMSQ_SIZES = [
    4,                       # scalar tail only, one block
    1028 + 3,                # 128 vectors + a 7-element scalar tail
    (1 << 21) + 1028,        # many blocks, below the grid cap
    2 * _PASS + _PASS // 2 + 3,   # capped grid, single-vector loop runs 2-3x
    4 * _PASS + 8 * 1000 + 5,     # four-loads-in-flight loop, then remainder
]

# About log2(n) ~ 33 fp32 roundings of 2^-24 lie along the reduction tree
# (pairwise within a vector, a short chain per thread, wave and block
# reduce), over positive terms, and the final stage is exact in fp64:
# 33 * 2^-24 ~ 2e-6.
SUMSQ_BOUND = 2e-6


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_grad_sumsq_matches_float64(n):
    g = torch.randn(n, generator=_gen(n % 1000)).bfloat16()
    ref = math.sqrt(float(g.double().pow(2).sum()))
    gd = g.to(DEV)
    got = ops.grad_norm(gd)
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    again = ops.grad_norm(gd)
    err = abs(float(got) - ref) / ref
    print(f"SUMSQ n={n} got={float(got):.9g} ref={ref:.9g} rel_err={err:.3e} "
          f"bound={SUMSQ_BOUND}")
    assert err < SUMSQ_BOUND
    assert torch.equal(got, again)  # no atomics: same bits every time


def test_grad_sumsq_past_int32():
    """n = 2^32 + 4096: the last 4096 elements lie past every 32-bit index."""
    n = (1 << 32) + 4096
    g = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    g[-4096:] = 1.0
    got = float(ops.grad_norm(g))
    del g
    print(f"SUMSQ n=2^32+4096 got={got}")
    assert got == 64.0


def test_grad_sumsq_rejects_misaligned():
    g = torch.zeros(64, dtype=torch.bfloat16, device=DEV)[1:]
    lib = _backend.require()
    out = torch.zeros(1, device=DEV)
    parts = torch.zeros(int(lib.kf_grad_sumsq_nparts(63)), device=DEV)
    assert lib.kf_grad_sumsq(ops._fp(out), ops._fp(parts), ops._p(g), 63,
                             ops._stream()) != 0
    # the wrapper routes such a buffer to torch instead
    assert float(ops.grad_norm(g)) == 0.0


# ---------------------------------------------------------- kf_adamw_clip

N_ADAMW = (1 << 21) + 1028
_NODECAY = ((1 << 20), (1 << 20) + 4096)   # the one undecayed range
HYPER = (1e-2, 0.9, 0.95, 1e-8, 0.1, 3)     # lr, b1, b2, eps, wd, step


def _adamw_state():
    g = _gen(7)
    p32 = torch.randn(N_ADAMW, generator=g)
    grad = (torch.randn(N_ADAMW, generator=g) * 0.5).bfloat16()
    m = torch.randn(N_ADAMW, generator=g) * 0.1
    v = torch.rand(N_ADAMW, generator=g) * 0.01
    return [t.to(DEV) for t in (p32.bfloat16(), p32, grad, m, v)]


def _masks():
    lo, hi = _NODECAY
    mask = torch.ones(N_ADAMW, device=DEV)
    mask[lo:hi] = 0.0
    groups = torch.ones(-(-N_ADAMW // ops.WD_GROUP), dtype=torch.uint8,
                        device=DEV)
    groups[lo // ops.WD_GROUP:hi // ops.WD_GROUP] = 0
    return mask, groups


def _assert_same(a, b, what):
    for name, x, y in zip(("p16", "p32", "grad", "m", "v"), a, b):
        assert torch.equal(x, y), f"{what}: {name} differs"


@pytest.mark.parametrize("scale", [0.37, 1.0])
def test_adamw_clip_bit_equal_to_mul_then_adamw(scale):
    mask, groups = _masks()
    scale_bf16 = torch.tensor(scale, device=DEV).to(torch.bfloat16)
    old, new = _adamw_state(), _adamw_state()
    g_before = new[2].clone()

    old[2].mul_(scale_bf16)
    ops.fused_adamw(*old, mask, *HYPER)
    ops.fused_adamw(*new, None, *HYPER, wd_groups=groups,
                    gscale=scale_bf16.float().reshape(1))
    _assert_same(old, new, f"scale={scale}")
    if scale == 1.0:
        assert torch.equal(new[2], g_before)   # neither scaled nor rewritten
    else:
        assert not torch.equal(new[2], g_before)
    # the undecayed range really is undecayed: against a run that decays all
    lo, hi = _NODECAY
    alld = _adamw_state()
    alld[2].mul_(scale_bf16)
    ops.fused_adamw(*alld, None, *HYPER)
    assert not torch.equal(alld[1][lo:hi], new[1][lo:hi])
    assert torch.equal(alld[1][hi:], new[1][hi:])


def test_adamw_clip_null_scale_null_mask_and_fp32_mask():
    mask, groups = _masks()
    scale_bf16 = torch.tensor(0.37, device=DEV).to(torch.bfloat16)
    gscale = scale_bf16.float().reshape(1)

    old, new = _adamw_state(), _adamw_state()       # gscale null
    ops.fused_adamw(*old, mask, *HYPER)
    ops.fused_adamw(*new, None, *HYPER, wd_groups=groups)
    _assert_same(old, new, "gscale null")

    old, new = _adamw_state(), _adamw_state()       # mask null
    old[2].mul_(scale_bf16)
    ops.fused_adamw(*old, None, *HYPER)
    ops.fused_adamw(*new, None, *HYPER, gscale=gscale)
    _assert_same(old, new, "mask null")

    old, new = _adamw_state(), _adamw_state()       # fp32 mask kept (ZeRO)
    old[2].mul_(scale_bf16)
    ops.fused_adamw(*old, mask, *HYPER)
    ops.fused_adamw(*new, mask, *HYPER, gscale=gscale)
    _assert_same(old, new, "fp32 mask")


def test_adamw_clip_rejects_bad_arguments():
    n = 4096 + 2
    p32 = torch.zeros(n, device=DEV)
    st = [p32.bfloat16(), p32, p32.bfloat16(), p32.clone(), p32.clone()]
    one = torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError, match="adamw_clip"):   # n % 4 != 0
        ops.fused_adamw(*st, None, *HYPER, gscale=one)
    with pytest.raises(RuntimeError, match="adamw"):        # as before
        ops.fused_adamw(*st, None, *HYPER)
    st = [t[:4096] for t in st]
    groups = torch.ones(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="not both"):
        ops.fused_adamw(*st, torch.ones(4096, device=DEV), *HYPER,
                        wd_groups=groups)
    with pytest.raises(ValueError, match="wd_groups"):      # too few groups
        ops.fused_adamw(*st, None, *HYPER, wd_groups=groups[:63])
    lib = _backend.require()   # the entry point itself refuses both masks
    assert lib.kf_adamw_clip(
        ops._p(st[0]), ops._fp(st[1]), ops._p(st[2]), ops._fp(st[3]),
        ops._fp(st[4]), ops._fp(torch.ones(4096, device=DEV)),
        ops._p(groups), ops._fp(None), 4096, *HYPER, ops._stream()) != 0


# ------------------------------------------------------ kf_rmsnorm_bwd_res

def _norm_bwd(lib_fn, name, dy, x, w, rstd, dres=None):
    rows, cols = x.shape
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    acc = torch.zeros(cols, dtype=torch.float32, device=DEV)
    args = [ops._p(dx), ops._p(dw), ops._fp(acc), ops._p(dy), ops._p(x),
            ops._p(w), ops._fp(rstd)]
    if name == "rmsnorm_bwd_res":
        args.append(ops._p(dres))
    _backend.check(lib_fn(*args, rows, cols, ops._stream()), name)
    return dx, dw


# rows: one block / a few / past the 1024-block cap (the row loop iterates).
# cols 256 and 4096 take the register kernel (one slot partly filled, two
# full slots); 8192 is past it and takes the LDS-accumulator kernel.
@pytest.mark.parametrize("cols", [256, 4096, 8192])
@pytest.mark.parametrize("rows", [1, 5, 2100])
def test_rmsnorm_bwd_res_bit_equal_to_bwd_then_add(rows, cols):
    g = _gen(rows + cols)
    x, dy, dres = (torch.randn(rows, cols, generator=g).bfloat16()
                   for _ in range(3))
    w = torch.randn(cols, generator=g).bfloat16()
    xd, dyd, dresd, wd = (t.to(DEV) for t in (x, dy, dres, w))
    lib = _backend.require()
    y = torch.empty_like(xd)
    rstd = torch.empty(rows, dtype=torch.float32, device=DEV)
    _backend.check(lib.kf_rmsnorm_fwd(ops._p(y), ops._fp(rstd), ops._p(xd),
                                      ops._p(wd), rows, cols, 1e-5,
                                      ops._stream()), "rmsnorm_fwd")
    dx0, _ = _norm_bwd(lib.kf_rmsnorm_bwd, "rmsnorm_bwd", dyd, xd, wd, rstd)
    dx1, dw1 = _norm_bwd(lib.kf_rmsnorm_bwd_res, "rmsnorm_bwd_res", dyd, xd,
                         wd, rstd, dresd)
    assert torch.equal(dx1, dx0 + dresd)
    dx2, dw2 = _norm_bwd(lib.kf_rmsnorm_bwd_res, "rmsnorm_bwd_res", dyd, xd,
                         wd, rstd, None)
    assert torch.equal(dx2, dx0)
    # dw goes through fp32 atomics (not bit-reproducible on any path):
    # test_rmsnorm_bwd's whole-tensor bound, and per column under the same
    _, _, dwr = T.rms_norm_oracle(x, w, dy)
    for dw in (dw1, dw2):
        whole, col = T.rel_err(dw, dwr), T.col_err(dw, dwr)
        print(f"PARITY rmsnorm_bwd_res dw rows={rows} cols={cols} "
              f"whole={whole:.5f} col_err={col:.5f} bound=0.03")
        assert whole < 3e-2 and col < 3e-2


_REGS_OFF_CHILD = r"""
import torch
from kubeflow_amd import ops
from kubeflow_amd.ops import _backend
lib = _backend.require()
dev = torch.device("cuda", 0)
for rows, cols in ((5, 256), (2100, 4096)):
    g = torch.Generator(device="cpu").manual_seed(rows)
    x, dy, dres = (torch.randn(rows, cols, generator=g).bfloat16().to(dev)
                   for _ in range(3))
    w = torch.randn(cols, generator=g).bfloat16().to(dev)
    rstd = torch.rsqrt(x.float().pow(2).mean(1) + 1e-5)
    out = []
    for fn, extra in ((lib.kf_rmsnorm_bwd, []),
                      (lib.kf_rmsnorm_bwd_res, [ops._p(dres)])):
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        acc = torch.zeros(cols, device=dev)
        err = fn(ops._p(dx), ops._p(dw), ops._fp(acc), ops._p(dy), ops._p(x),
                 ops._p(w), ops._fp(rstd), *extra, rows, cols, ops._stream())
        assert err == 0, err
        out.append((dx, dw))
    assert torch.equal(out[1][0], out[0][0] + dres), (rows, cols)
    rel = (out[1][1].float() - out[0][1].float()).norm() \
        / out[0][1].float().norm()
    assert float(rel) < 3e-2, float(rel)
print("REGS_OFF_OK")
"""


def test_rmsnorm_bwd_res_regs_switch_child_process():
    """KF_RMSNORM_BWD_REGS=0 (read once per process): the LDS-accumulator
    kernel with the residual add at widths the register kernel otherwise
    takes; same dx."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KF_RMSNORM_BWD_REGS="0")
    r = subprocess.run([sys.executable, "-c", _REGS_OFF_CHILD], cwd=repo,
                       env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0 and "REGS_OFF_OK" in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_rmsnorm_bwd_res_rejects_cols_not_multiple_of_8():
    x = torch.zeros(4, 12, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(12, device=DEV, dtype=torch.bfloat16)
    rstd = torch.ones(4, device=DEV)
    lib = _backend.require()
    with pytest.raises(RuntimeError, match="rmsnorm_bwd_res"):
        _norm_bwd(lib.kf_rmsnorm_bwd_res, "rmsnorm_bwd_res", x, x, w, rstd, x)


def test_rms_norm_residual_noncontiguous_grad_falls_back():
    """A non-contiguous residual gradient takes kf_rmsnorm_bwd + add; the
    result is the fused one's."""
    g = _gen(3)
    x = torch.randn(6, 256, generator=g).bfloat16().to(DEV)
    w = torch.randn(256, generator=g).bfloat16().to(DEV)
    dy = torch.randn(6, 256, generator=g).bfloat16().to(DEV)
    dr = torch.randn(256, 6, generator=g).bfloat16().to(DEV)
    grads = []
    for dres in (dr.t(), dr.t().contiguous()):
        xg = x.clone().requires_grad_(True)
        y, xr = ops.rms_norm_residual(xg, w)
        torch.autograd.backward([y, xr], [dy, dres])
        grads.append(xg.grad)
    assert torch.equal(grads[0], grads[1])


# ------------------------------------------------------------ model wiring

def _tiny_grads(monkeypatch, norm_res):
    from kubeflow_amd.models import build_model
    if norm_res is None:
        monkeypatch.delenv("KF_NORM_RES", raising=False)
    else:
        monkeypatch.setenv("KF_NORM_RES", norm_res)
    torch.manual_seed(0)
    model = build_model("llama-tiny", device=DEV)
    acts = {}

    def keep(name):
        def hook(_mod, _inp, out):
            out.retain_grad()
            acts[name] = out
        return hook

    model.embed.register_forward_hook(keep("embed"))
    for i, layer in enumerate(model.layers):
        layer.register_forward_hook(keep(f"layer{i}"))
    g = _gen(1)
    tokens = torch.randint(0, model.cfg.vocab_size, (2, 128), generator=g)
    targets = torch.randint(0, model.cfg.vocab_size, (2, 128), generator=g)
    loss = model(tokens.to(DEV), targets.to(DEV))
    loss.backward()
    out = {k: a.grad for k, a in acts.items()}
    # matrix gradients come from GEMMs over those activations; norm weights
    # and the loss value (fp32 atomics: kf_rmsnorm_bwd*'s dw, kf_ce_fwd's
    # row sum) and the embedding scatter are not bit-reproducible
    out.update({n: p.grad for n, p in model.named_parameters()
                if p.dim() == 2 and not n.startswith("embed")})
    loose = {n: p.grad for n, p in model.named_parameters() if p.dim() == 1}
    return out, loose, float(loss.detach())


def test_llama_tiny_grads_equal_with_and_without_norm_res(monkeypatch):
    new, new_loose, new_loss = _tiny_grads(monkeypatch, None)
    old, old_loose, old_loss = _tiny_grads(monkeypatch, "0")
    assert set(new) == set(old) and len(new) > 10
    for k in new:
        assert new[k] is not None and torch.equal(new[k], old[k]), k
    for k in new_loose:   # atomics: test_rmsnorm_bwd's bound
        assert T.rel_err(new_loose[k], old_loose[k]) < 3e-2, k
    # the forward is the same code on both routes; its loss is an atomic
    # fp32 sum over T = 256 rows, at worst T roundings of 2^-24 apart
    assert abs(new_loss - old_loss) <= 256 * 2.0 ** -24 * old_loss


def test_trainer_step_equal_with_and_without_step_tail(monkeypatch):
    """Two llama-tiny trainer steps, KF_STEP_TAIL=0 against the default:
    same clipped gradients and parameters, grad norm within the bound."""
    from kubeflow_amd.models import build_model
    from kubeflow_amd.runtime import Trainer, TrainConfig
    monkeypatch.setenv("KF_NORM_RES", "0")   # identical backward on both
    runs = []
    for tail in ("0", "1"):
        monkeypatch.setenv("KF_STEP_TAIL", tail)
        torch.manual_seed(0)
        model = build_model("llama-tiny", device=DEV)
        tr = Trainer(model, TrainConfig(warmup_steps=1))
        g = _gen(2)
        tok = torch.randint(0, model.cfg.vocab_size, (2, 128), generator=g)
        tok = tok.to(DEV)
        loss = tr.step(tok, tok)
        assert float(loss) > 0
        runs.append(tr)
    a, b = runs
    assert a.last_grad_norm.dim() == 0 == b.last_grad_norm.dim()
    assert b.last_grad_norm.dtype == torch.float32 and b.last_grad_norm.is_cuda
    # norm-weight gradients come from fp32 atomics and differ from run to
    # run, so the compared tail starts from one state and one gradient
    b.flat.data.copy_(a.flat.data)
    b.p32.copy_(a.p32)
    b.m.copy_(a.m)
    b.v.copy_(a.v)
    gnew = torch.randn(a.flat.numel, generator=_gen(5)).bfloat16().to(DEV)
    gnew = gnew * (a.p32 != 0)   # padding keeps g = 0
    a.flat.grad.copy_(gnew); b.flat.grad.copy_(gnew)
    monkeypatch.setenv("KF_STEP_TAIL", "0")
    a._clip_and_update()
    monkeypatch.setenv("KF_STEP_TAIL", "1")
    b._clip_and_update()
    rel = abs(float(a.last_grad_norm) - float(b.last_grad_norm)) \
        / float(a.last_grad_norm)
    print(f"TAIL grad_norm old={float(a.last_grad_norm):.9g} "
          f"new={float(b.last_grad_norm):.9g} rel={rel:.3e}")
    assert rel < SUMSQ_BOUND
    scale_a = (1.0 / (a.last_grad_norm + 1e-6)).clamp(max=1.0).bfloat16()
    scale_b = (1.0 / (b.last_grad_norm + 1e-6)).clamp(max=1.0).bfloat16()
    assert float(scale_a) < 1.0           # the clip is active
    if torch.equal(scale_a, scale_b):     # else: a flipped bf16 rounding
        for name in ("data", "grad"):
            assert torch.equal(getattr(a.flat, name), getattr(b.flat, name))
        assert torch.equal(a.p32, b.p32) and torch.equal(a.m, b.m)
        assert torch.equal(a.v, b.v)
    else:
        pytest.fail(f"clip scale rounded differently: {float(scale_a)} vs "
                    f"{float(scale_b)} (norms {float(a.last_grad_norm)} / "
                    f"{float(b.last_grad_norm)})")
