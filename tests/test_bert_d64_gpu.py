"""The real BERT configs (12 or 2 heads x 64) on the GPU: a training step
with the padded-length mask, and classify serving through InferenceEngine,
both with every attention call on the head-dim-64 kernels."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_BOUND = 4e-2  # test_attention_bwd's bound
LOSS_BOUND = 1e-2


def _relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _train_step(model, tokens, targets, kv_len):
    model.zero_grad(set_to_none=True)
    loss = model(tokens, targets, kv_len=kv_len)
    loss.backward()
    torch.cuda.synchronize()
    return (float(loss.detach()),
            {n: p.grad.detach().clone() for n, p in model.named_parameters()})


def test_bert_tiny_train_step_matches_reference_route(monkeypatch):
    """bert-tiny (2 layers, 2 heads x 64), B = 2, S = 128, kv_len = 50:
    loss and every parameter gradient on the native kernels against the
    KF_ATTN_D64=0 reference route on the same weights."""
    from kubeflow_amd.models import build_model
    torch.manual_seed(3)
    dev = torch.device("cuda", 0)
    model = build_model("bert-tiny", device=dev)
    with torch.no_grad():  # zero-init biases: make every path carry signal
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.02 * torch.randn_like(p))
    g = torch.Generator(device="cpu").manual_seed(4)
    tokens = torch.randint(0, model.cfg.vocab_size, (2, 128),
                           generator=g).to(dev)
    targets = torch.randint(0, model.cfg.n_classes, (2,), generator=g).to(dev)

    loss_n, grads_n = _train_step(model, tokens, targets, 50)
    monkeypatch.setenv("KF_ATTN_D64", "0")
    loss_r, grads_r = _train_step(model, tokens, targets, 50)

    print("loss native/reference", loss_n, loss_r)
    assert abs(loss_n - loss_r) < LOSS_BOUND, (loss_n, loss_r)
    errs = {n: _relerr(grads_n[n], grads_r[n]) for n in grads_r}
    print(errs)
    assert any(g.abs().max() > 0 for g in grads_r.values())
    bad = {n: e for n, e in errs.items() if not e < GRAD_BOUND}
    assert not bad, bad


def test_bert_base_classify_engine():
    """bert-base through the whole InferenceEngine at prompt lengths 51
    (padded, masked path) and 128 (unpadded path): class probabilities
    within test_classifier_engine_gpu_matches_forward's bound of a CPU fp32
    clone of the same weights."""
    from kubeflow_amd.runtime.serving import InferenceEngine

    torch.manual_seed(10)
    dev = torch.device("cuda", 0)
    eng = InferenceEngine("bert-base", device=dev, max_batch=4)
    eng.start()
    try:
        cpu = copy.deepcopy(eng.model).float().cpu()
        for n in (51, 128):
            prompt = list(range(2, 2 + n))
            r = eng.generate(prompt, timeout=120)
            assert not r.error, r.error
            with torch.no_grad():
                want = torch.softmax(cpu(torch.tensor([prompt]))[0].float(),
                                     dim=-1)
            got = torch.tensor(r.scores)
            assert torch.allclose(got, want, atol=0.05), (n, got, want)
    finally:
        eng.stop()
