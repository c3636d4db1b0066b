#!/usr/bin/env python
"""Speculative decoding: kf_attn_verify against T successive kf_attn_decode
calls, and the captured verify step against the captured one-token step.

Kernel rows (llama3-8b heads: Hq 32, Hkv 8, g = 4): both kernels through their
C entry points on the same bf16 cache, one call (or T decode calls) per slot
group of a ring of more than 512 MB of K and V, the ring pass captured into
one graph. Device events, windows of --window seconds, --repeats rounds
alternating the two. --baseline-lib: a libkfops.so of another commit, whose
kf_attn_decode the decode rows then run.

Graph rows: the engine's captured step at `batch` sequences of context 1024,
one token against T tokens per sequence, per KF_SERVE_QUANT; the ratio minus
one is the number of accepted draft tokens per step at which speculation
breaks even. The weights are random, so nothing here says how many drafts a
real model accepts.

  python scripts/spec_decode_bench.py [--baseline-lib PATH] [--graph MODEL]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kubeflow_amd import ops  # noqa: E402
from kubeflow_amd.ops import _backend  # noqa: E402

HQ, HKV, D = 32, 8, 128
RING_BYTES = 512 << 20


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
def kernel_rows(dev, base, window, repeats):
    lib = _backend.require()
    print("| N | context | T | kf_attn_verify us | T x kf_attn_decode us | "
          "ratio |")
    print("|---|---|---|---|---|---|")
    for ctx in (1024, 4096):
        smax = ctx + 8
        for N in (1, 4):
            ring = max(4, math.ceil(RING_BYTES / (N * smax * HKV * D * 4)))
            g = torch.Generator(device="cpu").manual_seed(ctx + N)
            kc = torch.randn(ring * N, smax, HKV, D, generator=g).to(
                dev, torch.bfloat16)
            vc = kc.flip(0).contiguous()
            slots = [torch.arange(i * N, (i + 1) * N, dtype=torch.int32,
                                  device=dev) for i in range(ring)]
            splits = min(8, max(1, 512 // (N * HKV)))
            for Tn in (1, 2, 4, 8):
                q = torch.randn(N, Tn, HQ, D, generator=g).to(
                    dev, torch.bfloat16)
                qt = [q[:, t].contiguous() for t in range(Tn)]
                lens = [torch.full((N,), ctx + t, dtype=torch.int32,
                                   device=dev) for t in range(Tn)]
                out = torch.empty_like(q)
                po = torch.empty(N, Tn * HQ, splits, D, device=dev)
                pm = torch.empty(N, Tn * HQ, splits, 2, device=dev)
                p, st = ops._p, ops._stream

                def verify():
                    for s in slots:
                        _backend.check(lib.kf_attn_verify(
                            p(out), p(po), p(pm), p(q), p(kc), p(vc),
                            ops._i32p(s), ops._i32p(lens[0]), N, Tn, smax, HQ,
                            HKV, D, splits, D ** -0.5, st()), "verify")

                def decode():
                    for s in slots:
                        for t in range(Tn):
                            _backend.check(base.kf_attn_decode(
                                p(out[:, 0]), p(po), p(pm), p(qt[t]), p(kc),
                                p(vc), ops._i32p(s), ops._i32p(lens[t]), N,
                                smax, HQ, HKV, D, splits, D ** -0.5, st()),
                                "decode")

                times = _alternate({"verify": _capture(verify),
                                    "decode": _capture(decode)}, window,
                                   repeats)
                us = {n: sorted(v * 1e3 / ring for v in ts)
                      for n, ts in times.items()}
                med = {n: v[len(v) // 2] for n, v in us.items()}
                print(f"| {N} | {ctx} | {Tn} | {med['verify']:.1f} "
                      f"({us['verify'][0]:.1f}..{us['verify'][-1]:.1f}) | "
                      f"{med['decode']:.1f} ({us['decode'][0]:.1f}.."
                      f"{us['decode'][-1]:.1f}) | "
                      f"{med['decode'] / med['verify']:.2f} |")
                print(json.dumps({"row": "attn_verify", "N": N, "ctx": ctx,
                                  "T": Tn, "splits": splits, "us": us}),
                      flush=True)
            del kc, vc
            torch.cuda.empty_cache()


@torch.no_grad()
def graph_rows(dev, model, window, repeats):
    from kubeflow_amd.runtime.serving import InferenceEngine

    ctx = 1024
    for quant in ("off", "fp8"):
        torch.manual_seed(0)
        eng = InferenceEngine(model, device=dev, max_slots=6, smax=2048,
                              max_batch=4, quant=quant)
        graphs = {}
        for batch in (1, 4):
            for Tn in (1, 2, 4, 8):
                graph, static = eng._graph_for(batch, Tn)
                seq = torch.arange(batch, dtype=torch.int32, device=dev) + 1
                static["slots"].copy_(seq.repeat_interleave(Tn))
                if Tn > 1:
                    static["seq_slots"].copy_(seq)
                static["lens"].fill_(ctx)
                static["positions"].copy_(
                    ctx - 1 + torch.arange(Tn, device=dev).repeat(batch))
                graphs[(batch, Tn)] = graph
        times = _alternate(graphs, window, repeats)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for (batch, Tn), ts in times.items():
            s = sorted(ts)
            ratio = med[(batch, Tn)] / med[(batch, 1)]
            print(f"| {model} | {quant} | {batch} | {Tn} | "
                  f"{med[(batch, Tn)]:.3f} ({s[0]:.3f}..{s[-1]:.3f}) | "
                  f"{ratio:.3f} | {ratio - 1:.3f} |")
            print(json.dumps({"row": "verify_graph", "model": model,
                              "quant": quant, "batch": batch, "T": Tn,
                              "ms": s}), flush=True)
        del eng, graphs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--graph", default="",
                    help="comma-separated model names for the graph rows")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    base = _backend.require()
    if args.baseline_lib:
        base = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        base.kf_attn_decode.restype = ctypes.c_int
        base.kf_attn_decode.argtypes = _backend.SIGNATURES["kf_attn_decode"]
        print(f"kf_attn_decode from {args.baseline_lib}")
    if not args.no_kernels:
        kernel_rows(dev, base, args.window, args.repeats)
    if args.graph:
        print("\n| model | KF_SERVE_QUANT | sequences | T | graph replay ms "
              "median (min..max) | vs T=1 | break-even accepted/step |")
        print("|---|---|---|---|---|---|---|")
    for model in filter(None, args.graph.split(",")):
        graph_rows(dev, model, args.window, args.repeats)


if __name__ == "__main__":
    main()
