"""kf_gemm_q4_grouped benchmark (GPU), scripts/gemm_q4_bench.py protocol (its
helpers): warm-up per row, device events, enough calls for a >= 0.5 s window,
three repeats with the competitors alternated inside each repeat, min..max.

llama-moe-3b layer shapes (h = f = 2048, E = 8, k = 2) at T = 64 / 256 / 1024
/ 4096 tokens, router logits random or all on two experts. One MoE block,
every path fed the same x and logits, banks holding the same dequantized
values:

  q4          ops.moe_experts_q4: route, grouped w13 GEMM through routing.src
              with the SwiGLU epilogue, grouped w2 GEMM, combine; no host sync
  bf16        ops.moe_experts on bf16 banks, the path MoE prefill takes without
              quant_prefill: one host sync, gather, a hipBLASLt mm per expert,
              swiglu over [M, 2f], mm per expert, combine
  dequant     dequantize both banks, then the bf16 path
  q4-unfused  q4 with swiglu=False and ops.swiglu over [M, 2f]
  q4-gather   q4 with ops.moe_gather in front of the w13 GEMM instead of rows=

--sanity: every row on one expert against kf_gemm_q4 at the same M (w13 bank,
no swiglu): what the prologue and the dead blocks of the grid cost.
--verify: MoEMLP.decode_routed(q4=) at 64 and 256 rows against decode_dense.
--engine: llama-moe-3b, quant="mxfp4", quant_prefill off and on: weight_bytes,
memory_allocated() and the first token of a 1024-token prompt (median of 3).

Usage: python scripts/gemm_q4_grouped_bench.py [--window 0.5] [--repeats 3]
           [--tokens 64,256,1024,4096] [--sanity] [--verify] [--engine]
Prints tables and one JSON line per row.
"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from gemm_q4_bench import _alternate, _med
from kubeflow_amd import ops

H = F = 2048
E, TOPK = 8, 2


def _report(row, key, times, base):
    for n, t in times.items():
        s = sorted(t)
        print(f"| {key} | {n} | {_med(t) * 1e3:.1f} ({s[0] * 1e3:.1f}.."
              f"{s[-1] * 1e3:.1f}) | {_med(t) / _med(times[base]):.2f} |")
        print(json.dumps({"row": row, "case": key, "path": n,
                          "us": [v * 1e3 for v in t],
                          "over_" + base: _med(t) / _med(times[base])}),
              flush=True)


def _banks(dev):
    g = torch.Generator().manual_seed(0)
    q4, bf = [], []
    for n, k in ((2 * F, H), (H, F)):
        w = (torch.randn(E * n, k, generator=g) * 0.02).to(dev)
        q4.append(ops.quantize_mxfp4_rows(w))
        bf.append(ops.dequantize_mxfp4_rows(*q4[-1]).view(E, n, k))
    return tuple(q4), bf


def _inputs(dev, T, two):
    g = torch.Generator().manual_seed(T)
    x = (torch.randn(T, H, generator=g) * 0.5).to(dev, torch.bfloat16)
    logits = torch.randn(T, E, generator=g)
    if two:
        logits[:, :2] += 100.0
    return x, logits.to(dev, torch.bfloat16)


@torch.no_grad()
def _block_rows(dev, tokens, window, repeats):
    q4, (w13, w2) = _banks(dev)
    (w13_4, s13), (w2_4, s2) = q4
    print("| T, routing | path | us per block median (min..max) | x bf16 |")
    print("|---|---|---|---|")
    for T in tokens:
        for two in (False, True):
            x, logits = _inputs(dev, T, two)

            def unfused():
                r = ops.moe_route(logits, TOPK, sync=False)
                a = ops.swiglu(ops.grouped_linear_q4(x, w13_4, s13, r.offsets,
                                                     r.src))
                return ops.moe_combine(
                    ops.grouped_linear_q4(a, w2_4, s2, r.offsets), r)

            def gathered():
                r = ops.moe_route(logits, TOPK, sync=False)
                a = ops.grouped_linear_q4(ops.moe_gather(x, r), w13_4, s13,
                                          r.offsets, swiglu=True)
                return ops.moe_combine(
                    ops.grouped_linear_q4(a, w2_4, s2, r.offsets), r)

            fns = {
                "q4": lambda: ops.moe_experts_q4(x, logits, q4, TOPK),
                "bf16": lambda: ops.moe_experts(x, logits, w13, w2, TOPK),
                "dequant": lambda: ops.moe_experts(
                    x, logits,
                    ops.dequantize_mxfp4_rows(w13_4, s13).view_as(w13),
                    ops.dequantize_mxfp4_rows(w2_4, s2).view_as(w2), TOPK),
                "q4-unfused": unfused, "q4-gather": gathered,
            }
            ref = fns["bf16"]().float()
            for n in ("q4", "q4-unfused", "q4-gather"):
                rel = ((fns[n]().float() - ref).norm() / ref.norm()).item()
                assert rel < 2e-2, (n, rel)
            _report("block", f"{T}, {'two experts' if two else 'random'}",
                    _alternate(fns, window, repeats), "bf16")


@torch.no_grad()
def _sanity_rows(dev, tokens, window, repeats):
    (w13_4, s13), _ = _banks(dev)[0]
    print("\n| M on one expert | path | us median (min..max) | x gemm_q4 |")
    print("|---|---|---|---|")
    for T in tokens:
        M = T * TOPK
        x = (torch.randn(M, H) * 0.5).to(dev, torch.bfloat16)
        off = torch.tensor([0, 0, 0] + [M] * (E - 2), dtype=torch.int32,
                           device=dev)       # everything on expert 2
        w4e, se = w13_4[2 * 2 * F:3 * 2 * F], s13[2 * 2 * F:3 * 2 * F]
        fns = {"grouped": lambda: ops.grouped_linear_q4(x, w13_4, s13, off),
               "gemm_q4": lambda: ops.linear_q4(x, w4e, se)}
        assert torch.equal(fns["grouped"](), fns["gemm_q4"]())
        _report("sanity", str(M), _alternate(fns, window, repeats), "gemm_q4")


@torch.no_grad()
def _verify_rows(dev, window, repeats):
    from kubeflow_amd.models import build_model
    from kubeflow_amd.runtime.serving import quantize_moe_banks

    moe = build_model("llama-moe-3b", device=dev,
                      dtype=torch.bfloat16).layers[0].moe
    q4 = quantize_moe_banks(moe, "mxfp4")
    print("\n| verify-step rows | path | us median (min..max) | x dense |")
    print("|---|---|---|---|")
    for rows in (64, 256):
        x = (torch.randn(rows, 1, moe.cfg.hidden_size) * 0.5).to(
            dev, torch.bfloat16)
        fns = {"routed q4": lambda: moe.decode_routed(x, q4=q4),
               "dense": lambda: moe.decode_dense(x)}
        _report("verify", str(rows), _alternate(fns, window, repeats),
                "dense")


def _engine_rows(dev):
    from kubeflow_amd.runtime.serving import InferenceEngine, Request

    print("\n| llama-moe-3b, quant=mxfp4 | memory_allocated GB | weight_bytes "
          "GB | first token of a 1024-token prompt, ms (3 runs) |")
    print("|---|---|---|---|")
    prompt = torch.randint(
        0, 32000, (1024,),
        generator=torch.Generator().manual_seed(0)).tolist()
    for knob in (False, True):
        gc.collect()
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        eng = InferenceEngine("llama-moe-3b", device=dev, max_slots=2,
                              smax=2048, max_batch=1, quant="mxfp4",
                              quant_prefill=knob)
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
    ap.add_argument("--tokens", default="64,256,1024,4096")
    ap.add_argument("--no-block", action="store_true")
    ap.add_argument("--sanity", action="store_true")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--engine", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tokens = [int(t) for t in args.tokens.split(",")]
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if not args.no_block:
        _block_rows(dev, tokens, args.window, args.repeats)
    if args.sanity:
        _sanity_rows(dev, tokens, args.window, args.repeats)
    if args.verify:
        _verify_rows(dev, args.window, args.repeats)
    if args.engine:
        _engine_rows(dev)


if __name__ == "__main__":
    main()
