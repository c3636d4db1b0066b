#!/usr/bin/env python
"""Ragged prefill attention: ops.attention_prefill (kf_attn_prefill) against
ops.flash_attention_rect (kf_attn_fwd4_rect) on the same tensors.

Rows (llama3-8b heads: Hq 32, Hkv 8, g = 4), both through their wrappers as
the engine calls them, rect on the zero-copy slab view of one slot with its
256-row query pad: one sequence of C new tokens behind `context` cached ones,
and one mixed batch in a single ragged call against the sum of the
per-sequence rect calls. Each measurement walks a ring of slot groups of more
than 512 MB of K and V, the ring pass captured into one graph. Device events,
windows of --window seconds, --repeats rounds alternating the two.

  python scripts/prefill_bench.py [--window S] [--repeats N]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kubeflow_amd import ops  # noqa: E402

HQ, HKV, D = 32, 8, 128
RING_BYTES = 512 << 20
SINGLE = [(C, ctx) for ctx in (1024, 4096) for C in (17, 256, 1024)]
# (C, context) per sequence: a prefix-cache tail, two fresh prompts of unlike
# length and a chunk in the middle of a long prompt
MIXED = [(17, 1024), (100, 0), (700, 0), (207, 512)]


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


@torch.no_grad()
def row(dev, name, seqs, window, repeats):
    N = len(seqs)
    smax = (max(c + ctx for c, ctx in seqs) + 127) // 128 * 128
    ring = max(4, math.ceil(RING_BYTES / (N * smax * HKV * D * 4)))
    gen = torch.Generator(device="cpu").manual_seed(smax + N)
    kc = torch.randn(ring * N, smax, HKV, D, generator=gen).to(
        dev, torch.bfloat16)
    vc = kc.flip(0).contiguous()
    counts = [c for c, _ in seqs]
    q = torch.randn(sum(counts), HQ, D, generator=gen).to(dev, torch.bfloat16)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    starts = i32([0] + counts).cumsum(0).int()
    lens = i32([ctx + 1 for _, ctx in seqs])
    slots = [i32(list(range(i * N, (i + 1) * N))) for i in range(ring)]
    qs = q.split(counts)

    def ragged():
        for s in slots:
            ops.attention_prefill(q, kc, vc, s, starts, lens, max(counts))

    def rect():
        for i in range(ring):
            for n, (c, ctx) in enumerate(seqs):
                s = i * N + n
                ops.flash_attention_rect(qs[n][None], kc[s:s + 1, :ctx + c],
                                         vc[s:s + 1, :ctx + c], q_offset=ctx)

    times = _alternate({"ragged": _capture(ragged), "rect": _capture(rect)},
                       window, repeats)
    us = {n: sorted(v * 1e3 / ring for v in ts) for n, ts in times.items()}
    med = {n: v[len(v) // 2] for n, v in us.items()}
    print(f"| {name} | {med['ragged']:.1f} ({us['ragged'][0]:.1f}.."
          f"{us['ragged'][-1]:.1f}) | {med['rect']:.1f} ({us['rect'][0]:.1f}"
          f"..{us['rect'][-1]:.1f}) | {med['rect'] / med['ragged']:.2f} |")
    print(json.dumps({"row": "attn_prefill", "seqs": seqs, "us": us}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    print("| sequences (C new @ context) | kf_attn_prefill us median "
          "(min..max) | flash_attention_rect us, summed | ratio |")
    print("|---|---|---|---|")
    for c, ctx in SINGLE:
        row(dev, f"{c} @ {ctx}", [(c, ctx)], args.window, args.repeats)
    row(dev, "mixed: " + ", ".join(f"{c} @ {x}" for c, x in MIXED), MIXED,
        args.window, args.repeats)


if __name__ == "__main__":
    main()
