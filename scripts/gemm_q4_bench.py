"""kf_gemm_q4 benchmark (GPU), scripts/moe_decode_bench.py protocol: warm-up
per shape, device events, enough calls for a >= 0.5 s window, three repeats
with the competitors alternated inside each repeat, min..max shown.

llama3-8b's four linears (wqkv 6144x4096, wo 4096x4096, w13 28672x4096, w2
4096x14336) at M = 64 / 256 / 1024 / 4096 rows, every competitor fed the same
bf16 activations and computing the product on the same dequantized values:

  gemm_q4   ops.linear_q4 -> kf_gemm_q4 on the MXFP4 pair
  bf16      F.linear on the dequantized bf16 weight (hipBLASLt: the rate
            yardstick; it reads 4x the weight bytes and converts nothing)
  dequant   today's path for such a call: dequantize_mxfp4_rows + F.linear

TFLOP/s is 2*M*N*K over the call time, whatever the call does inside.

--engine adds the serving side on llama3-8b, quant="mxfp4" with quant_prefill
off and on: torch.cuda.memory_allocated() and engine.weight_bytes after
construction, and the time to the first token of one 1024-token prompt
(median of 3 after one warm-up, host clock around a synchronized prefill).

Usage: python scripts/gemm_q4_bench.py [--window 0.5] [--repeats 3]
                                       [--rows 64,256,1024,4096] [--engine]
Prints one table and one JSON line per row.
"""
import argparse
import gc
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F
from kubeflow_amd import ops

SHAPES = (("wqkv", 6144, 4096), ("wo", 4096, 4096), ("w13", 28672, 4096),
          ("w2", 4096, 14336))


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


@torch.no_grad()
def _gemm_rows(dev, rows, window, repeats):
    print("| linear NxK | M | path | us median (min..max) | TFLOP/s | "
          "x bf16 time | x dequant time |")
    print("|---|---|---|---|---|---|---|")
    for name, N, K in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(N + K)
        w = (torch.randn(N, K, generator=g) * 0.02).to(dev)
        w4, sc = ops.quantize_mxfp4_rows(w)
        wb = ops.dequantize_mxfp4_rows(w4, sc)
        del w
        for M in rows:
            x = (torch.randn(M, K, generator=g) * 0.5).to(dev, torch.bfloat16)
            fns = {
                "gemm_q4": lambda: ops.linear_q4(x, w4, sc),
                "bf16": lambda: F.linear(x, wb),
                "dequant": lambda: F.linear(
                    x, ops.dequantize_mxfp4_rows(w4, sc, x.dtype)),
            }
            if not ops._gemm_q4_shape_ok(M, N, K) or M <= 32:
                raise RuntimeError("kf_gemm_q4 does not take this call; the "
                                   "row would time another path")
            ref = fns["bf16"]().float()
            rel = ((fns["gemm_q4"]().float() - ref).norm() / ref.norm()).item()
            times = _alternate(fns, window, repeats)
            for n, t in times.items():
                s = sorted(t)
                print(f"| {name} {N}x{K} | {M} | {n} | {_med(t) * 1e3:.1f} "
                      f"({s[0] * 1e3:.1f}..{s[-1] * 1e3:.1f}) | "
                      f"{2 * M * N * K / (_med(t) * 1e-3) / 1e12:.0f} | "
                      f"{_med(t) / _med(times['bf16']):.2f} | "
                      f"{_med(t) / _med(times['dequant']):.2f} |")
                print(json.dumps({
                    "row": "gemm_q4", "linear": name, "N": N, "K": K, "M": M,
                    "path": n, "us": [v * 1e3 for v in t],
                    "over_bf16": _med(t) / _med(times["bf16"]),
                    "over_dequant": _med(t) / _med(times["dequant"]),
                    "rel_err_vs_bf16": rel}), flush=True)
        del w4, sc, wb


def _engine_rows(dev):
    from kubeflow_amd.runtime.serving import InferenceEngine, Request

    print("\n| llama3-8b, quant=mxfp4 | memory_allocated GB | weight_bytes GB "
          "| first token of a 1024-token prompt, ms (3 runs) |")
    print("|---|---|---|---|")
    prompt = torch.randint(
        0, 32000, (1024,),
        generator=torch.Generator().manual_seed(0)).tolist()
    for knob in (False, True):
        gc.collect()
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        eng = InferenceEngine("llama3-8b", device=dev, max_slots=2, smax=2048,
                              max_batch=1, quant="mxfp4", quant_prefill=knob)
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        alloc = torch.cuda.memory_allocated()
        ttft = []
        for _ in range(4):
            req = Request(rid="r", prompt=prompt, max_new_tokens=2)
            req.slot = eng.cache.alloc()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng._prefill(req)
            torch.cuda.synchronize()
            ttft.append((time.perf_counter() - t0) * 1e3)
            eng.cache.free(req.slot)
        ttft = ttft[1:]
        print(f"| quant_prefill={knob} | {alloc / 1e9:.2f} | "
              f"{eng.weight_bytes / 1e9:.2f} | {_med(ttft):.1f} "
              f"({min(ttft):.1f}..{max(ttft):.1f}) |")
        print(json.dumps({"row": "engine", "quant_prefill": knob,
                          "memory_allocated": alloc,
                          "weight_bytes": eng.weight_bytes,
                          "ttft_ms": ttft}), flush=True)
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", default="64,256,1024,4096")
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--no-gemm", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if not args.no_gemm:
        _gemm_rows(dev, [int(m) for m in args.rows.split(",")], args.window,
                   args.repeats)
    if args.engine:
        _engine_rows(dev)


if __name__ == "__main__":
    main()
