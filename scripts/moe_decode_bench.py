"""MoE decode benchmark (GPU), scripts/moe_dispatch_bench.py protocol: warm-up,
device events, enough replays for a >= 0.5 s window, three repeats with the
competitors alternated inside each repeat, min..max shown.

One MoE block at llama-moe-3b layer dims (h = f = 2048, E = 8, k = 2), inside
a captured graph, at T = 1, 4, 16, 32 decode tokens:

  dense        MoEMLP.decode_dense: every expert on every token (the path the
               serving engine takes by default)
  routed       MoEMLP.decode_routed: ops.moe_experts_decode, the grouped
               skinny GEMM over device offsets
  routed_fp8   the same with per-row e4m3 expert banks

with the router's own seeded random logits ("random") and with a gate that
sends every token to experts {0, 1} ("two").

The two banks of one block are 201 MB in bf16, less than the 256 MB Infinity
Cache, so a graph of one block would replay out of cache. The graph therefore
holds --layers independent blocks (default 4, 805 MB of banks), as a decode
step does, and the time is per block.

Weight bytes are counted from `offsets`: an expert with rows streams its w13
and w2 once, an expert without rows nothing; dense streams all E. GB/s is
those bytes over the time of the whole block (router, sort, swiglu and combine
included), not a kernel's rate.

Usage: python scripts/moe_decode_bench.py [--window 0.5] [--repeats 3]
                                          [--layers 4] [--tokens 1,4,16,32]
Prints one table per logits pattern and one JSON line per row.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F
from kubeflow_amd import ops
from kubeflow_amd.models import llama
from kubeflow_amd.runtime.serving import quantize_moe_banks

E, K, H, FF = 8, 2, 2048, 2048


def _ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def _iters_for(fn, window):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = _ms(fn, 3)
    return max(5, math.ceil(window * 1e3 / max(t, 1e-3)))


def _med(xs):
    return sorted(xs)[len(xs) // 2]


def _alternate(fns, window, repeats):
    iters = {n: _iters_for(fn, window) for n, fn in fns.items()}
    times = {n: [] for n in fns}
    for _ in range(repeats):
        for n, fn in fns.items():
            times[n].append(_ms(fn, iters[n]))
    return times


def _modules(dev, layers, pattern):
    cfg = llama.LlamaConfig(name="moe-layer", hidden_size=H, ffn_dim=FF,
                            n_experts=E, top_k=K)
    g = torch.Generator(device="cpu").manual_seed(0)
    mods = []
    for _ in range(layers):
        moe = llama.MoEMLP(cfg)
        with torch.no_grad():
            for p in moe.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            if pattern == "two":
                # column 0 of x is held at 8: logits 80 for experts {0, 1}
                moe.gate.weight[:, 0] = 0.0
                moe.gate.weight[:2, 0] = 10.0
        mods.append(moe.to(device=dev, dtype=torch.bfloat16))
    return mods


def _capture(fn):
    """The capture pattern of InferenceEngine._graph_for."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@torch.no_grad()
def _rows(dev, pattern, tokens, layers, window, repeats):
    mods = _modules(dev, layers, pattern)
    q8s = [quantize_moe_banks(m) for m in mods]
    per_expert = 3 * H * FF            # w13 + w2 elements of one expert
    print(f"\nlogits: {pattern}; E{E} k{K} h{H} f{FF}, {layers} blocks per "
          "graph, times per block")
    print("| T | path | us median (min..max) | experts hit | weight MB | "
          "GB/s | vs dense |")
    print("|---|---|---|---|---|---|---|")
    for T in tokens:
        g = torch.Generator(device="cpu").manual_seed(T)
        x = torch.randn(T, 1, H, generator=g)
        x[:, :, 0] = 8.0
        x = x.to(dev, torch.bfloat16)
        for m in mods:
            if not m.routed_decode_ok(x) or not m.routed_decode_ok(x, True):
                raise RuntimeError("routed decode does not apply; the "
                                   "comparison would be dense against dense")
        hit = []
        for m in mods:
            lg = F.linear(x.reshape(T, H), m.gate.weight)
            off = ops.moe_route(lg, K, sync=False).offsets
            hit.append(int((off.diff() > 0).sum()))
        hit_mean = sum(hit) / len(hit)
        paths = {
            "dense": lambda: [m.decode_dense(x) for m in mods],
            "routed": lambda: [m.decode_routed(x) for m in mods],
            "routed_fp8": lambda: [m.decode_routed(x, q8=q)
                                   for m, q in zip(mods, q8s)],
        }
        graphs, outs = {}, {}
        for n, fn in paths.items():
            graphs[n], outs[n] = _capture(fn)
            graphs[n].replay()
        torch.cuda.synchronize()
        agree = {n: max(_rel(a, b) for a, b in zip(outs[n], outs["dense"]))
                 for n in ("routed", "routed_fp8")}
        times = _alternate({n: gr.replay for n, gr in graphs.items()}, window,
                           repeats)
        dense_med = _med(times["dense"]) / layers
        for n, t in times.items():
            t = [v / layers for v in t]
            experts = E if n == "dense" else hit_mean
            nbytes = experts * per_expert * (1 if n == "routed_fp8" else 2)
            if n == "routed_fp8":
                nbytes += experts * (2 * FF + H) * 4  # fp32 row scales
            s = sorted(t)
            gbs = nbytes / (_med(t) * 1e-3) / 1e9
            print(f"| {T} | {n} | {_med(t) * 1e3:.1f} ({s[0] * 1e3:.1f}.."
                  f"{s[-1] * 1e3:.1f}) | {experts:g} | {nbytes / 1e6:.1f} | "
                  f"{gbs:.0f} | {_med(t) / dense_med:.2f}x |")
            print(json.dumps({
                "row": "moe_decode", "logits": pattern, "T": T, "path": n,
                "us_per_block": [v * 1e3 for v in t], "experts_hit": experts,
                "weight_bytes": nbytes, "gbs": gbs,
                "over_dense": _med(t) / dense_med,
                "rel_err_vs_dense": agree.get(n, 0.0)}), flush=True)
        del graphs, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--tokens", default="1,4,16,32")
    ap.add_argument("--logits", default="random,two")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    tokens = [int(t) for t in args.tokens.split(",")]
    for pattern in args.logits.split(","):
        _rows(dev, pattern, tokens, args.layers, args.window, args.repeats)


if __name__ == "__main__":
    main()
