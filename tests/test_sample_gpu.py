"""kf_sample (ops.sample on bf16 GPU logits) against reference.sample in
float64: exact tokens.

u is never random. For a target token j, u is the centre of j's interval of
the float64 CDF over the kept set in index order, and j's kept probability is
asserted >= 1e-4, so u sits >= 5e-5 of the mass from either edge. The
kernel's error is far inside that: weights are fp32 exp2 results (relative
error ~1e-6 near the maximum, where the mass is) truncated to 2^-40, and all
sums are exact integers. A symbolic top_p is the midpoint between two
consecutive prefix masses in rank order, their gap asserted >= 1e-4 likewise.
"""
import functools

import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import reference
from kubeflow_amd.runtime.serving import InferenceEngine

pytestmark = pytest.mark.gpu
NINF = float("-inf")
VOCABS = (512, 1000, 1003, 128256)


@functools.lru_cache(maxsize=None)
def _logits(V, variant="randn"):
    """[5, V] bf16 on the CPU: 3 * randn (ties heavily at V = 128256)."""
    g = torch.Generator().manual_seed(V)
    x = (3 * torch.randn(5, V, generator=g)).bfloat16()
    if variant == "plateau":      # 40 entries tied at the maximum
        idx = torch.randperm(V, generator=g)[:40]
        x[:, idx] = x.max() + 1
    elif variant == "ninf":       # 10% of the entries -inf
        x[torch.rand(5, V, generator=g) < 0.1] = NINF
    return x


def _plan(x, T, k, p):
    """One row in float64: (top_p as a number, kept weights in index order)."""
    x = x.double()
    xs, order = torch.sort(x, descending=True, stable=True)
    w = torch.exp((xs - xs[0]) / T)
    w[xs == NINF] = 0
    if 0 < k < x.numel():
        w[k:] = 0
    cum = w.cumsum(0)
    total = cum[-1]
    if p == "mid0.9":   # between the prefix masses on either side of 0.9
        i = int((cum >= 0.9 * total).nonzero()[0])
        lo = cum[i - 1] if i else cum[i] * 0
        assert (cum[i] - lo) / total >= 1e-4
        p = float((lo + cum[i]) / 2 / total)
    elif p == "below_top":  # half the top token's mass: it alone is kept
        assert w[0] / total >= 1e-4
        p = float(w[0] / total / 2)
    if p < 1:
        w = w * ((cum - w) < p * total)
    wi = torch.zeros_like(w)
    wi[order] = w
    return p, wi


def _inputs(x, rows, which):
    """rows: one (temperature, top_k, top_p) per row of x -> the four
    parameter tensors (CPU) and each sampled row's target: its first, middle
    or last kept index (which = 0, 1, 2), None for a greedy row."""
    temp, top_k, top_p, u, aim = [], [], [], [], []
    for r, (T, k, p) in enumerate(rows):
        temp.append(T)
        top_k.append(k)
        if T <= 0:
            top_p.append(1.0)
            u.append(0.5)
            aim.append(None)
            continue
        p, wi = _plan(x[r], T, k, p)
        prob = wi / wi.sum()
        ok = (prob >= 1e-4).nonzero().flatten()
        assert ok.numel() > 0
        j = int(ok[(0, ok.numel() // 2, -1)[which]])
        assert prob[j] >= 1e-4
        top_p.append(p)
        u.append(float(prob[:j + 1].sum() - prob[j] / 2))
        aim.append(j)
    return (torch.tensor(temp, dtype=torch.float32),
            torch.tensor(top_k, dtype=torch.int32),
            torch.tensor(top_p, dtype=torch.float32),
            torch.tensor(u, dtype=torch.float32)), aim


def _check(x, rows, x_dev=None):
    """Three launches: every sampled row aims at its first, middle and last
    kept index."""
    x_dev = x.cuda() if x_dev is None else x_dev
    for which in range(3):
        args, aim = _inputs(x, rows, which)
        want = reference.sample(x, *args, dtype=torch.float64)
        for r, j in enumerate(aim):
            assert j is None or int(want[r]) == j
        got = ops.sample(x_dev, *(t.cuda() for t in args))
        assert got.dtype == torch.int32 and got.shape == (x.shape[0],)
        assert torch.equal(got.cpu(), want), (which, got.cpu(), want)


PARAMS = {
    "greedy": (0.0, 0, 1.0),
    "temp0.7": (0.7, 0, 1.0),
    "temp1.5": (1.5, 0, 1.0),
    "k1": (1.0, 1, 1.0),
    "k2": (1.0, 2, 1.0),
    "k50": (1.0, 50, 1.0),
    "kV": (1.0, "V", 1.0),
    "p0.9": (0.3, 0, "mid0.9"),
    "p_single": (0.3, 0, "below_top"),
    "k50_p0.9": (0.5, 50, "mid0.9"),
}
MIXED = ("greedy", "k50_p0.9", "temp1.5", "p0.9", "k2")


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize(
    "name,N", [(n, N) for n in PARAMS for N in (1, 5)] + [("mixed", 5)])
def test_matches_float64_reference(name, N, V):
    # mixed: one launch with a different parameter set in each of its 5 rows
    rows = ([PARAMS[n] for n in MIXED] if name == "mixed"
            else [PARAMS[name]] * N)
    rows = [(T, V if k == "V" else k, p) for T, k, p in rows]
    _check(_logits(V)[:N], rows)


@pytest.mark.parametrize("V", (1000, 128256))
@pytest.mark.parametrize("variant,row", [
    ("plateau", (1.0, 17, 1.0)),     # k = 17 cuts the 40-entry plateau
    ("plateau", (1.0, 0, "mid0.9")),
    ("ninf", (0.7, 0, 1.0)),
    ("ninf", (0.3, 50, "mid0.9")),
])
def test_plateau_and_ninf_rows(variant, row, V):
    _check(_logits(V, variant), [row] * 5)


@pytest.mark.parametrize("pad", (8, 3))  # 16-byte aligned rows, and not
@pytest.mark.parametrize("V", (1000, 128256))
def test_row_stride(V, pad):
    x = _logits(V)
    wide = torch.full((5, V + pad), 50.0, dtype=torch.bfloat16).cuda()
    wide[:, :V] = x.cuda()
    assert not wide[:, :V].is_contiguous()
    _check(x, [PARAMS[n] for n in MIXED], x_dev=wide[:, :V])


def test_any_input_gives_a_token_in_range():
    V = 1000
    x = _logits(V).clone()
    x[0, ::7] = float("nan")
    x[1, 5] = float("inf")
    x[2] = float("nan")
    x[3] = NINF
    x[4, 1::2] = NINF
    inf, nan = float("inf"), float("nan")
    for temp, k, p, u in (
            ([nan, 1.0, 1.0, 1.0, 1e-30], [-5, 2 ** 31 - 1, -2 ** 31, 3, V],
             [-1.0, nan, 0.0, 2.0, -inf], [nan, 2.0, -1.0, inf, 1.0]),
            ([inf, inf, 1e30, 1e-38, 0.5], [1, 0, 7, -1, 999],
             [0.0, 1e-30, 0.5, nan, 0.999999], [1.0, -0.0, nan, 0.5, 7.0])):
        got = ops.sample(x.cuda(), torch.tensor(temp).cuda(),
                         torch.tensor(k, dtype=torch.int32).cuda(),
                         torch.tensor(p).cuda(), torch.tensor(u).cuda()).cpu()
        assert bool(((got >= 0) & (got < V)).all()), got


def test_capture_follows_the_static_tensors():
    V = 1000
    x = _logits(V)
    x_dev = x.cuda()
    sets = [[t.cuda() for t in _inputs(x, [PARAMS[n] for n in names], w)[0]]
            for names, w in ((("k50", "temp0.7", "greedy", "p0.9", "k2"), 0),
                             (MIXED, 2))]
    eager = [ops.sample(x_dev, *s).clone() for s in sets]
    assert not torch.equal(eager[0], eager[1])
    static = [t.clone() for t in sets[0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.sample(x_dev, *static)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sample(x_dev, *static)
    for i in (0, 1, 1, 0, 1):
        for dst, src in zip(static, sets[i]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), i


def _generate(monkeypatch, graphs, **kw):
    monkeypatch.setenv("KF_SERVE_GRAPH", graphs)
    torch.manual_seed(0)
    eng = InferenceEngine("llama-tiny", max_slots=4, smax=256,
                          max_batch=2).start(precapture=False)
    try:
        r = eng.generate([1, 2, 3, 4], max_new_tokens=8, **kw)
        assert r.error == "" and len(r.generated) == 8
        return r.generated
    finally:
        eng.stop()


def test_engine_seeded_request_with_and_without_graphs(monkeypatch):
    kw = dict(temperature=1.2, top_k=40, top_p=0.9, seed=5)
    with_graphs = _generate(monkeypatch, "1", **kw)
    assert with_graphs == _generate(monkeypatch, "0", **kw)
    assert with_graphs != _generate(monkeypatch, "1", **{**kw, "seed": 6})


def test_engine_top_k_1_is_greedy(monkeypatch):
    greedy = _generate(monkeypatch, "1")
    assert greedy == _generate(monkeypatch, "1", temperature=1.0, top_k=1,
                               seed=3)
