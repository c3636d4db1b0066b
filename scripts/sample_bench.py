"""Sampling benchmark (GPU), scripts/moe_dispatch_bench.py protocol: warm-up,
device events, enough calls for a >= 0.5 s window, three repeats with the
competitors alternated inside each repeat, min..max shown.

[N, V] bf16 logits at the Llama-3 vocabulary (V = 128256), N = 1, 16, 32
rows, three parameter mixes:

  greedy     every row temperature 0
  temp       every row temperature 0.8
  topk_topp  temperature 0.8, top_k 50, top_p 0.9

and two ways to turn them into tokens:

  native   ops.sample (kf_sample, one launch)
  torch    the sequence the engine ran before kf_sample existed and still
           runs under KF_SAMPLE=0 (InferenceEngine._sample_batch): argmax for
           an all-greedy batch, else two small host-to-device tensors, a float
           copy and divide, softmax, multinomial, argmax and where. It has no
           top-k or top-p, so the third mix is native only.

Two times per cell. "device" is the event time per call with the parameter
tensors already on the device and no read-back. "wall" is the host clock per
call for what a decode step pays outside the graph: building the per-step
host-to-device tensors (native: u, unless every row is greedy; torch: its
two), the call, and .tolist().

The logits (at most 8 MB) stay in cache between calls, as they do in a decode
step, where the LM head has just written them.

Usage: python scripts/sample_bench.py [--window 0.5] [--repeats 3]
                                      [--rows 1,16,32] [--out FILE.md]
Prints a markdown table (also written to --out) and one JSON line per row.
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from kubeflow_amd import ops
from kubeflow_amd.runtime.serving import InferenceEngine

V = 128256
MIXES = {"greedy": (0.0, 0, 1.0), "temp": (0.8, 0, 1.0),
         "topk_topp": (0.8, 50, 0.9)}


def _device_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def _wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()          # ends in .tolist(): synchronises
    return (time.perf_counter() - t0) * 1e3 / iters


def _iters_for(fn, timer, window):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return max(5, math.ceil(window * 1e3 / max(timer(fn, 3), 1e-3)))


def _alternate(fns, timer, window, repeats):
    iters = {n: _iters_for(fn, timer, window) for n, fn in fns.items()}
    times = {n: [] for n in fns}
    for _ in range(repeats):
        for n, fn in fns.items():
            times[n].append(timer(fn, iters[n]))
    return times


def _torch_device(logits, temps):
    """InferenceEngine._sample_batch without its .tolist()."""
    if all(t <= 0 for t in temps):
        return logits.argmax(-1)
    t = torch.tensor([max(tt, 1e-6) if tt > 0 else 1.0 for tt in temps],
                     device=logits.device).unsqueeze(1)
    probs = torch.softmax(logits.float() / t, dim=-1)
    sampled = torch.multinomial(probs, 1).squeeze(1)
    greedy = logits.argmax(-1)
    pick = torch.tensor([tt > 0 for tt in temps], device=logits.device)
    return torch.where(pick, sampled, greedy)


class _Req:
    def __init__(self, temperature):
        self.temperature = temperature


def _fmt(xs):
    xs = [1e3 * x for x in xs]  # microseconds
    return f"{sorted(xs)[len(xs) // 2]:.1f} ({min(xs):.1f}..{max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", default="1,16,32")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    lines = ["| N | mix | native device µs | torch device µs | "
             "native wall µs | torch wall µs |", "|---|---|---|---|---|---|"]
    for N in [int(n) for n in args.rows.split(",")]:
        logits = (3 * torch.randn(N, V, generator=g)).bfloat16().to(dev)
        for mix, (temp, k, p) in MIXES.items():
            temps = [temp] * N
            reqs = [_Req(temp) for _ in range(N)]
            t_d = torch.full((N,), temp, device=dev)
            k_d = torch.full((N,), k, dtype=torch.int32, device=dev)
            p_d = torch.full((N,), p, device=dev)
            u_h = torch.rand(N, generator=g)
            u_d = u_h.to(dev)
            u_list = u_h.tolist()

            def native_wall():
                # as the engine: no draws are sent for an all-greedy batch
                u = (torch.tensor(u_list, dtype=torch.float32, device=dev)
                     if temp > 0 else u_d)
                return ops.sample(logits, t_d, k_d, p_d, u).tolist()

            device = {"native": lambda: ops.sample(logits, t_d, k_d, p_d, u_d)}
            wall = {"native": native_wall}
            if mix != "topk_topp":
                device["torch"] = lambda: _torch_device(logits, temps)
                wall["torch"] = lambda: InferenceEngine._sample_batch(logits,
                                                                      reqs)
            dt = _alternate(device, _device_ms, args.window, args.repeats)
            wt = _alternate(wall, _wall_ms, args.window, args.repeats)
            lines.append(
                f"| {N} | {mix} | {_fmt(dt['native'])} | "
                f"{_fmt(dt['torch']) if 'torch' in dt else '-'} | "
                f"{_fmt(wt['native'])} | "
                f"{_fmt(wt['torch']) if 'torch' in wt else '-'} |")
            print(lines[-1], flush=True)
            print(json.dumps({"N": N, "mix": mix, "device_ms": dt,
                              "wall_ms": wt}), flush=True)
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
