"""MoE dispatch benchmark (GPU), scripts/attn_d64_bench.py protocol: warm-up,
device events, enough iterations for a >= 0.5 s window, three repeats with the
competitors alternated inside each repeat, spread reported.

Shape: T = 16384 tokens, E = 8, k = 2, h = 2048, f = 2048 (one llama-moe-3b
layer at micro-batch 4 x seq 4096).

  block    one MoEMLP forward (no_grad) and forward + backward with
           KF_MOE_NATIVE=1 (moe.hip path) and KF_MOE_NATIVE=0 (the per-expert
           Python loop), on the same module and input
  kernels  each moe.hip entry point alone, through the C ABI, with the
           achieved GB/s against the bytes it must move (every input read
           once, every output written once)

Usage: python scripts/moe_dispatch_bench.py [--window 0.5] [--repeats 3]
                                            [--only all|block|kernels]
Prints tables and one JSON line per row.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from kubeflow_amd import ops
from kubeflow_amd.models import llama
from kubeflow_amd.ops import _backend

T, E, K, H, F = 16384, 8, 2, 2048, 2048


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


def _spread(xs):
    return (max(xs) - min(xs)) / _med(xs)


def _alternate(fns, window, repeats):
    """{name: [ms per repeat]}, the competitors alternated in each repeat."""
    iters = {n: _iters_for(fn, window) for n, fn in fns.items()}
    times = {n: [] for n in fns}
    for _ in range(repeats):
        for n, fn in fns.items():
            times[n].append(_ms(fn, iters[n]))
    return times


def _block_rows(dev, window, repeats):
    cfg = llama.LlamaConfig(name="moe-layer", hidden_size=H, ffn_dim=F,
                            n_experts=E, top_k=K)
    g = torch.Generator(device="cpu").manual_seed(0)
    moe = llama.MoEMLP(cfg)
    with torch.no_grad():
        for p in moe.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    moe = moe.to(device=dev, dtype=torch.bfloat16)
    x = (torch.randn(4, T // 4, H, generator=g)
         .to(dev, torch.bfloat16).requires_grad_(True))
    do = torch.randn(4, T // 4, H, generator=g).to(dev, torch.bfloat16)

    def run(native, backward):
        def fn():
            os.environ["KF_MOE_NATIVE"] = native
            try:
                if backward:
                    moe(x).backward(do)
                    x.grad = None
                    moe.zero_grad(set_to_none=True)
                else:
                    with torch.no_grad():
                        moe(x)
            finally:
                os.environ.pop("KF_MOE_NATIVE", None)
        return fn

    fns = {f"{kind}_native{n}": run(n, kind == "fwdbwd")
           for kind in ("fwd", "fwdbwd") for n in ("1", "0")}
    times = _alternate(fns, window, repeats)
    print(f"\nblock: T{T} E{E} k{K} h{H} f{F}")
    print("| pass | KF_MOE_NATIVE | ms median (min..max) | spread |")
    print("|---|---|---|---|")
    for name, t in times.items():
        kind, native = name.split("_native")
        s = sorted(t)
        print(f"| {kind} | {native} | {_med(t):.3f} ({s[0]:.3f}..{s[-1]:.3f})"
              f" | {_spread(t) * 100:.1f}% |")
        print(json.dumps({"row": "block", "pass": kind, "native": native,
                          "ms": t, "spread": _spread(t)}), flush=True)
    for kind in ("fwd", "fwdbwd"):
        a, b = times[f"{kind}_native1"], times[f"{kind}_native0"]
        print(json.dumps({"row": "block_ratio", "pass": kind,
                          "native1_over_native0": _med(a) / _med(b)}),
              flush=True)


def _kernel_rows(dev, window, repeats):
    lib = _backend.require()
    p, fp, st = ops._p, ops._fp, ops._stream
    g = torch.Generator(device="cpu").manual_seed(0)
    bf = dict(device=dev, dtype=torch.bfloat16)
    logits = torch.randn(T, E, generator=g).to(**bf)
    r = ops.moe_route(logits, K)
    M = r.rows
    x = torch.randn(T, H, generator=g).to(**bf)
    y = torch.randn(M, H, generator=g).to(**bf)
    dout = torch.randn(T, H, generator=g).to(**bf)
    dwup = torch.randn(T, K, generator=g).to(**bf)
    xp, dy = torch.empty_like(y), torch.empty_like(y)
    out = torch.empty_like(x)
    dw = torch.empty_like(r.topw)
    dlogits = torch.empty_like(logits)
    topi, pos = torch.empty_like(r.topi), torch.empty_like(r.pos)
    src, offsets = torch.empty_like(r.src), torch.empty_like(r.offsets)
    probs, topw = torch.empty_like(r.probs), torch.empty_like(r.topw)
    work = torch.empty(int(lib.kf_moe_sort_nwork(T, K, E)),
                       dtype=torch.int32, device=dev)
    row = M * H * 2          # bytes of one pass over the permuted buffer
    tok = T * H * 2
    P = T * K
    # (launcher, bytes that must move)
    kernels = {
        "kf_moe_route": (lambda: lib.kf_moe_route(
            p(topi), fp(probs), p(topw), p(logits), T, E, K, st()),
            T * E * 2 + P * 10),
        "kf_moe_sort": (lambda: lib.kf_moe_sort(
            p(pos), p(src), p(offsets), p(work), p(r.topi), T, K, 0, E, st()),
            P * 4 + P * 4 + M * 4),
        "kf_moe_gather": (lambda: lib.kf_moe_gather(
            p(xp), p(x), p(r.src), M, T, H, st()), 2 * row + M * 4),
        "kf_moe_gather_bwd": (lambda: lib.kf_moe_gather_bwd(
            p(out), p(y), p(r.pos), T, K, H, M, st()), row + tok + P * 4),
        "kf_moe_combine": (lambda: lib.kf_moe_combine(
            p(out), p(y), p(r.topw), p(r.pos), T, K, H, M, st()),
            row + tok + P * 6),
        "kf_moe_combine_bwd": (lambda: lib.kf_moe_combine_bwd(
            p(dy), p(dw), p(dout), p(y), p(r.topw), p(r.pos), T, K, H, M,
            st()), 2 * row + tok + P * 8),
        "kf_moe_route_bwd": (lambda: lib.kf_moe_route_bwd(
            p(dlogits), p(dwup), fp(r.probs), p(r.topi), T, E, K, st()),
            P * 10 + T * E * 2),
    }
    times = _alternate({n: k[0] for n, k in kernels.items()}, window, repeats)
    print(f"\nkernels: T{T} E{E} k{K} h{H}, M = {M}")
    print("| kernel | us median (min..max) | MB | GB/s |")
    print("|---|---|---|---|")
    for name, t in times.items():
        nbytes = kernels[name][1]
        s = sorted(t)
        gbs = nbytes / (_med(t) * 1e-3) / 1e9
        print(f"| {name} | {_med(t) * 1e3:.1f} ({s[0] * 1e3:.1f}.."
              f"{s[-1] * 1e3:.1f}) | {nbytes / 1e6:.2f} | {gbs:.0f} |")
        print(json.dumps({"row": "kernel", "kernel": name, "ms": t,
                          "bytes": nbytes, "gbs": gbs,
                          "spread": _spread(t)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("all", "block", "kernels"),
                    default="all")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if args.only in ("all", "kernels"):
        _kernel_rows(dev, args.window, args.repeats)
    if args.only in ("all", "block"):
        _block_rows(dev, args.window, args.repeats)


if __name__ == "__main__":
    main()
