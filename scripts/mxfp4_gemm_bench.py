#!/usr/bin/env python
"""Decode GEMMs in bf16, fp8 and MXFP4 at the llama3-8b shapes, and the
captured decode step of a model under each KF_SERVE_QUANT.

Kernel rows: kf_skinny_gemm / _q8 / _q4 called through their C entry points,
one call per weight copy of a ring larger than the 256 MB of MALL (so every
call streams its weights from HBM), the ring pass captured into one graph so
the host's launch cost stays out. Device events, windows of --window seconds,
--repeats rounds alternating the three formats. GB/s counts the weight bytes
a call must read (scales included), nothing else.

--baseline-lib: a libkfops.so built from another commit; the bf16 and fp8
rows then run that library's kernels, so the new format is compared with what
the tree computed before it.

  python scripts/mxfp4_gemm_bench.py [--baseline-lib PATH] [--graph MODEL,...]
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

SHAPES = [("qkv", 6144, 4096), ("wo", 4096, 4096), ("w13", 28672, 4096),
          ("w2", 4096, 14336)]
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


def _ring(tensors, nbytes):
    """Copies of a weight (tuple of tensors) until the ring passes RING_BYTES;
    at least 4."""
    n = max(4, math.ceil(RING_BYTES / nbytes))
    return [tuple(t.clone() for t in tensors) for _ in range(n)]


@torch.no_grad()
def kernel_rows(dev, base, window, repeats):
    lib = _backend.require()
    print("| shape | M | format | us median (min..max) | weight MB | GB/s |")
    print("|---|---|---|---|---|---|")
    for name, N, K in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(N + K)
        w = (torch.randn(N, K, generator=g) * 0.02).to(dev, torch.bfloat16)
        w8, s8 = ops.quantize_fp8_rows(w)
        w4, s4 = ops.quantize_mxfp4_rows(w)
        fmts = {
            "bf16": ((w,), N * K * 2),
            "fp8": ((w8, s8), N * K + N * 4),
            "mxfp4": ((w4, s4), N * K // 2 + N * K // 32),
        }
        rings = {n: _ring(t, b) for n, (t, b) in fmts.items()}
        del w, w8, s8, w4, s4
        for M in (1, 16, 32):
            x = (torch.randn(M, K, generator=g) * 0.5).to(dev, torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            st = ops._stream

            def run(fmt):
                for t in rings[fmt]:
                    if fmt == "bf16":
                        err = base.kf_skinny_gemm(
                            ops._p(y), ops._p(x), ops._p(t[0]), None, M, N, K,
                            K, 0, 0, st())
                    elif fmt == "fp8":
                        err = base.kf_skinny_gemm_q8(
                            ops._p(y), ops._p(x), ops._p(t[0]), ops._fp(t[1]),
                            None, M, N, K, K, 0, 0, st())
                    else:
                        err = lib.kf_skinny_gemm_q4(
                            ops._p(y), ops._p(x), ops._p(t[0]), ops._p(t[1]),
                            None, M, N, K, K, 0, 0, st())
                    _backend.check(err, fmt)

            graphs = {f: _capture(lambda f=f: run(f)) for f in fmts}
            times = _alternate(graphs, window, repeats)
            for f, ts in times.items():
                us = sorted(v * 1e3 / len(rings[f]) for v in ts)
                med = us[len(us) // 2]
                gbs = fmts[f][1] / (med * 1e-6) / 1e9
                print(f"| {name} {N}x{K} | {M} | {f} | {med:.1f} "
                      f"({us[0]:.1f}..{us[-1]:.1f}) | {fmts[f][1] / 1e6:.1f} "
                      f"| {gbs:.0f} |")
                print(json.dumps({"row": "skinny_gemm", "shape": name, "N": N,
                                  "K": K, "M": M, "format": f, "us": us,
                                  "weight_bytes": fmts[f][1], "gbs": gbs}),
                      flush=True)
            del graphs
        del rings
        torch.cuda.empty_cache()


@torch.no_grad()
def graph_rows(dev, model, batch, window, repeats):
    """The engine's captured decode step at one batch bucket, per format. The
    engines are built one after the other and only their graphs kept."""
    from kubeflow_amd.runtime.serving import InferenceEngine

    graphs, keep = {}, []
    for quant in ("off", "fp8", "mxfp4"):
        torch.manual_seed(0)
        eng = InferenceEngine(model, device=dev, max_slots=batch + 1,
                              smax=1024, max_batch=batch, quant=quant)
        if (quant != "off") != bool(eng.quant):
            print(f"{model}: quant={quant} is not active, row skipped")
            continue
        graph, static = eng._graph_for(batch)
        static["lens"].fill_(512)
        static["positions"].fill_(511)
        graphs[quant] = graph
        keep.append(eng)
    times = _alternate(graphs, window, repeats)
    for q, ts in times.items():
        s = sorted(ts)
        print(f"| {model} | {batch} | {q} | {s[len(s) // 2]:.3f} "
              f"({s[0]:.3f}..{s[-1]:.3f}) |")
        print(json.dumps({"row": "decode_graph", "model": model,
                          "batch": batch, "quant": q, "ms": s}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--graph", default="",
                    help="comma-separated model names for the graph rows")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    base = _backend.require()
    if args.baseline_lib:
        base = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        for fn in ("kf_skinny_gemm", "kf_skinny_gemm_q8"):
            getattr(base, fn).restype = ctypes.c_int
            getattr(base, fn).argtypes = _backend.SIGNATURES[fn]
        print(f"bf16 and fp8 rows from {args.baseline_lib}")
    if not args.no_kernels:
        kernel_rows(dev, base, args.window, args.repeats)
    if args.graph:
        print("\n| model | batch | KF_SERVE_QUANT | graph replay ms median "
              "(min..max) |")
        print("|---|---|---|---|")
    for model in filter(None, args.graph.split(",")):
        graph_rows(dev, model, args.batch, args.window, args.repeats)


if __name__ == "__main__":
    main()
