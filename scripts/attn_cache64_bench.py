#!/usr/bin/env python
"""D = 64 cache attention (kf_attn64_cache) at the Llama-3.2-1B heads (Hq 32,
Hkv 8, D 64) against the D = 128 kernels on the same cache bytes (Hq 16,
Hkv 4, D 128: kv-heads halved, head dim doubled, g kept) and against torch
SDPA on the sliced cache.

Rows: decode (N sequences, one token each), verify (T tokens each) and prefill
(one sequence of C new tokens) behind `context` cached tokens, every kernel
through its ops wrapper as the engine calls it. SDPA gets the slot slab
[N, context + C] as a strided view, a prebuilt boolean mask where C > 1 and
enable_gqa. Each measurement walks a ring of slot groups of more than 512 MB
of K and V (twice the Infinity Cache), the ring pass captured into one graph.
Device events, windows of --window seconds, --repeats rounds alternating the
three.

  python scripts/attn_cache64_bench.py [--window S] [--repeats N]
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kubeflow_amd import ops  # noqa: E402

RING_BYTES = 512 << 20
SHAPES = {"d64": (32, 8, 64), "d128": (16, 4, 128)}   # Hq, Hkv, D
# (kind, N sequences, C tokens each, context)
ROWS = ([("decode", n, 1, ctx) for ctx in (1024, 4096) for n in (1, 4, 16)] +
        [("verify", 4, t, ctx) for ctx in (1024, 4096) for t in (4, 8)] +
        [("prefill", 1, c, ctx) for ctx in (1024, 4096)
         for c in (17, 256, 1024)])


def _ms(graph, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def _alternate(graphs, window, repeats):
    iters = {}
    for n, g in graphs.items():
        g.replay()
        torch.cuda.synchronize()
        iters[n] = max(3, math.ceil(window * 1e3 / max(_ms(g, 3), 1e-3)))
    times = {n: [] for n in graphs}
    for _ in range(repeats):
        for n, g in graphs.items():
            times[n].append(_ms(g, iters[n]))
    return times


def _native(dev, shape, kind, N, C, ctx, smax, ring, gen):
    """The ring pass of one kernel family at one head shape."""
    Hq, Hkv, D = SHAPES[shape]
    kc = torch.randn(ring * N, smax, Hkv, D, generator=gen).to(
        dev, torch.bfloat16)
    vc = kc.flip(0).contiguous()
    q = torch.randn(N * C, Hq, D, generator=gen).to(dev, torch.bfloat16)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    lens = i32([ctx + 1] * N)
    starts = i32([C * i for i in range(N + 1)])
    slots = [i32(list(range(i * N, (i + 1) * N))) for i in range(ring)]
    q4 = q.view(N, C, Hq, D)

    def run():
        for s in slots:
            if kind == "decode":
                ops.attention_decode(q, kc, vc, s, lens)
            elif kind == "verify":
                ops.attention_verify(q4, kc, vc, s, lens)
            else:
                ops.attention_prefill(q, kc, vc, s, starts, lens, C)
    return run, (kc, vc, q4)


def _sdpa(tensors, N, C, ctx, ring):
    kc, vc, q4 = tensors
    L = ctx + C
    qt = q4.transpose(1, 2)                                    # [N,Hq,C,D]
    mask = None
    if C > 1:   # token i sees keys [0, ctx + 1 + i)
        mask = (torch.arange(L, device=kc.device)[None, :]
                <= ctx + torch.arange(C, device=kc.device)[:, None])

    def run():
        for i in range(ring):
            k = kc[i * N:(i + 1) * N, :L].transpose(1, 2)      # [N,Hkv,L,D]
            v = vc[i * N:(i + 1) * N, :L].transpose(1, 2)
            F.scaled_dot_product_attention(qt, k, v, attn_mask=mask,
                                           enable_gqa=True)
    return run


@torch.no_grad()
def row(dev, kind, N, C, ctx, window, repeats):
    smax = (ctx + C + 127) // 128 * 128
    ring = max(4, math.ceil(RING_BYTES / (N * smax * 8 * 64 * 4)))
    gen = torch.Generator(device="cpu").manual_seed(smax + N)
    d64, t64 = _native(dev, "d64", kind, N, C, ctx, smax, ring, gen)
    d128, _ = _native(dev, "d128", kind, N, C, ctx, smax, ring, gen)
    times = _alternate({"d64": _capture(d64), "d128": _capture(d128),
                        "sdpa": _capture(_sdpa(t64, N, C, ctx, ring))},
                       window, repeats)
    us = {n: sorted(v * 1e3 / ring for v in ts) for n, ts in times.items()}
    med = {n: v[len(v) // 2] for n, v in us.items()}
    cell = lambda n: f"{med[n]:.1f} ({us[n][0]:.1f}..{us[n][-1]:.1f})"
    print(f"| {kind} | {N} | {C} | {ctx} | {cell('d64')} | {cell('d128')} | "
          f"{cell('sdpa')} | {med['d128'] / med['d64']:.2f} | "
          f"{med['sdpa'] / med['d64']:.2f} |")
    print(json.dumps({"row": "attn_cache64", "kind": kind, "N": N, "C": C,
                      "context": ctx, "us": us}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    print("| kind | N | tokens each | context | kf_attn64_cache us median "
          "(min..max) | D = 128 kernel, same bytes | torch SDPA, D = 64 | "
          "d128 / d64 | sdpa / d64 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for kind, N, C, ctx in ROWS:
        row(dev, kind, N, C, ctx, args.window, args.repeats)


if __name__ == "__main__":
    main()
