"""CPU counterpart of test_step_tail_gpu.py: the compact decay mask, the
reference compositions behind the new ops, and the model wiring of
rms_norm_residual. On the CPU every route is the reference composition, so
everything is equal bit for bit.
"""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.models import MnistMLP, build_model
from kubeflow_amd.parallel import FlatParamSpace
from kubeflow_amd.parallel.flat import ALIGN
from kubeflow_amd.runtime import Trainer, TrainConfig


def test_wd_groups_expand_to_wd_mask():
    """One byte per ALIGN elements; expanded, it is build_wd_mask except on
    the zero padding behind a decayed slice."""
    assert ops.WD_GROUP == ALIGN
    model = build_model("llama-tiny", dtype=torch.float32)
    flat = FlatParamSpace(model)
    mask, groups = flat.build_wd_mask(), flat.build_wd_groups()
    assert groups.dtype == torch.uint8
    assert groups.numel() * ALIGN == flat.numel
    assert groups.numel() * 256 <= mask.numel() * mask.element_size()
    expanded = groups.float().repeat_interleave(ALIGN)
    real = torch.zeros(flat.numel, dtype=torch.bool)
    kinds = set()
    for (off, n), p in zip(flat.slices, flat.params):
        assert off % ALIGN == 0
        real[off:off + n] = True
        kinds.add(p.dim() >= 2)
        assert (groups[off // ALIGN:-(-(off + n) // ALIGN)]
                == int(p.dim() >= 2)).all()
    assert kinds == {True, False}
    assert torch.equal(expanded[real], mask[real])
    assert (flat.data[~real] == 0).all() and (flat.grad[~real] == 0).all()

    # a model whose slices are not ALIGN multiples: padding shares the group
    flat = FlatParamSpace(MnistMLP(in_dim=5, hidden=3, n_classes=7),
                          dtype=torch.float32)
    expanded = flat.build_wd_groups().float().repeat_interleave(ALIGN)
    mask = flat.build_wd_mask()
    for off, n in flat.slices:
        assert torch.equal(expanded[off:off + n], mask[off:off + n])


def _state(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    p32 = torch.randn(n, generator=g)
    return [p32.bfloat16(), p32, (torch.randn(n, generator=g) * 0.5).bfloat16(),
            torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01]


HYPER = (1e-2, 0.9, 0.95, 1e-8, 0.1, 3)


@pytest.mark.parametrize("scale", [0.37, 1.0])
def test_fused_adamw_reference_with_groups_and_gscale(scale):
    n = 4096 + 128 + 4
    mask = torch.ones(n)
    mask[1024:1024 + 128] = 0.0
    groups = torch.ones(-(-n // ALIGN), dtype=torch.uint8)
    groups[1024 // ALIGN:(1024 + 128) // ALIGN] = 0
    s16 = torch.tensor(scale).bfloat16()
    old, new = _state(n), _state(n)
    old[2].mul_(s16)
    ops.fused_adamw(*old, mask, *HYPER)
    ops.fused_adamw(*new, None, *HYPER, wd_groups=groups,
                    gscale=s16.float().reshape(1))
    for a, b in zip(old, new):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="not both"):
        ops.fused_adamw(*new, mask, *HYPER, wd_groups=groups)


def test_grad_norm_cpu_is_vector_norm():
    g = torch.randn(1031).bfloat16()
    got = ops.grad_norm(g)
    assert got.dtype == torch.float32 and got.dim() == 0
    assert torch.equal(got, torch.linalg.vector_norm(g, dtype=torch.float32))


def test_rms_norm_residual_sums_both_gradients():
    """The returned x carries the residual branch: x.grad is the norm's dx
    plus whatever flows into the second output — against the two-consumer
    graph it replaces, in fp64, and by gradcheck."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 16, generator=g, dtype=torch.float64)
    w = torch.randn(16, generator=g, dtype=torch.float64)
    dy = torch.randn(3, 5, 16, generator=g, dtype=torch.float64)
    dres = torch.randn(3, 5, 16, generator=g, dtype=torch.float64)

    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y, xr = ops.rms_norm_residual(xa, wa, 1e-5)
    assert torch.equal(xr, xa)
    torch.autograd.backward([y, xr], [dy, dres])

    xb, wb = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ops.rms_norm(xb, wb, 1e-5).backward(dy)
    assert torch.equal(y, ops.rms_norm(xb, wb, 1e-5))
    assert torch.allclose(xa.grad, xb.grad + dres, rtol=1e-12, atol=1e-12)
    assert torch.equal(wa.grad, wb.grad)

    def both(xi, wi):
        yi, ri = ops.rms_norm_residual(xi, wi, 1e-5)
        return yi + 3.0 * ri   # both outputs reach the loss
    # reference.rms_norm computes in fp32 whatever the input type: central
    # differences at eps = 1e-3 carry ~1e-7 / 1e-3 = 1e-4 of rounding noise
    # and O(eps^2) of truncation, against entries of order 1
    assert torch.autograd.gradcheck(
        both, (x[0].clone().requires_grad_(True),
               w.clone().requires_grad_(True)),
        eps=1e-3, atol=2e-3, rtol=1e-3)


def _tiny_grads(monkeypatch, norm_res):
    if norm_res is None:
        monkeypatch.delenv("KF_NORM_RES", raising=False)
    else:
        monkeypatch.setenv("KF_NORM_RES", norm_res)
    torch.manual_seed(0)
    model = build_model("llama-tiny", dtype=torch.float32)
    acts = {}

    def keep(name):
        def hook(_mod, _inp, out):
            out.retain_grad()
            acts[name] = out
        return hook

    model.embed.register_forward_hook(keep("embed"))
    for i, layer in enumerate(model.layers):
        layer.register_forward_hook(keep(f"layer{i}"))
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, model.cfg.vocab_size, (2, 32), generator=g)
    targets = torch.randint(0, model.cfg.vocab_size, (2, 32), generator=g)
    loss = model(tokens, targets)
    loss.backward()
    out = {"loss": loss.detach()}
    out.update({k: a.grad for k, a in acts.items()})
    out.update({n: p.grad for n, p in model.named_parameters()})
    return out


def test_llama_tiny_grads_equal_with_and_without_norm_res(monkeypatch):
    new = _tiny_grads(monkeypatch, None)
    old = _tiny_grads(monkeypatch, "0")
    assert set(new) == set(old) and len(new) > 10
    for k in new:
        assert new[k] is not None and torch.equal(new[k], old[k]), k


def test_trainer_step_tail_switch_is_inert_on_cpu(monkeypatch):
    """CPU tensors keep the reference tail whatever KF_STEP_TAIL says."""
    results = []
    for tail in ("0", "1"):
        monkeypatch.setenv("KF_STEP_TAIL", tail)
        torch.manual_seed(0)
        tr = Trainer(build_model("llama-tiny", dtype=torch.float32),
                     TrainConfig(lr=1e-3, warmup_steps=1))
        assert not tr._fused_tail(tr.flat.grad)
        tok = torch.randint(0, 512, (2, 32),
                            generator=torch.Generator().manual_seed(3))
        tr.step(tok, tok)
        tr.step(tok, tok)
        results.append((tr.flat.data.clone(), tr.flat.grad.clone(),
                        tr.last_grad_norm.clone()))
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert results[0][2].dim() == 0
