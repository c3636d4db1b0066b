"""Head-dim-64 attention kernel benchmark (GPU), tests/attn_bench.py protocol:
warm-up, device events, enough iterations for a >= 0.5 s window, three
repeats with the competitors alternated inside each repeat.

Shapes: fine-tune (B64, S512, H12, D64) non-causal, and classify
(B64, S128, H12, D64) with kv_len 100. Competitors:
  a  ops.flash_attention on the attention_d64.hip kernels
  b  torch.nn.functional.scaled_dot_product_attention on the same tensors
     (k/v sliced to kv_len)
  c  KF_ATTN_D64=0, the torch reference math masked_attention used before
  d  the project's D = 128 kernels at half the heads (identical FLOPs;
     unmasked shape only — flash_attention has no kv_len at D = 128)
Each is timed forward alone (no_grad) and forward + backward. TF counts
4*B*H*S*kv_len*D for the forward and 2.5x that for the backward.

Per-sequence lengths (B64, S512, H12, one fixed seeded length mix), on the
same tensors:
  a  ops.flash_attention(seq_lens=...) on the kf_attn64_*_varlen kernels
  b  ops.flash_attention(kv_len=max(len)), the only native option before
  c  torch SDPA with a boolean key-padding mask
and a uniform row, seq_lens all 512 against the scalar path with no mask,
which shows what the varlen instantiation costs when there is nothing to
skip. Printed with the ratios a/b next to the ideal
sum(len^2) / (B * S * max(len)), and uniform a/b next to each side's own
repeat-to-repeat spread.

Usage: python scripts/attn_d64_bench.py [--window 0.5] [--repeats 3]
                                        [--only all|scalar|varlen]
Prints a table and one JSON line per (shape, competitor).
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

SHAPES = {
    "finetune": dict(B=64, S=512, H=12, kv_len=None),
    "classify": dict(B=64, S=128, H=12, kv_len=100),
}


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


def _competitors(B, S, H, kv_len, dev):
    g = torch.Generator(device="cpu").manual_seed(0)

    def mk(h, d):
        return (torch.randn(B, S, h, d, generator=g)
                .to(dev, torch.bfloat16).requires_grad_(True))

    q, k, v = mk(H, 64), mk(H, 64), mk(H, 64)
    do = torch.randn(B, S, H, 64, generator=g).to(dev, torch.bfloat16)
    q2, k2, v2 = mk(H // 2, 128), mk(H // 2, 128), mk(H // 2, 128)
    do2 = torch.randn(B, S, H // 2, 128, generator=g).to(dev, torch.bfloat16)

    def native():
        return ops.flash_attention(q, k, v, causal=False, kv_len=kv_len)

    def sdpa():
        kk, vv = (k, v) if kv_len is None else (k[:, :kv_len], v[:, :kv_len])
        return F.scaled_dot_product_attention(
            q.transpose(1, 2), kk.transpose(1, 2),
            vv.transpose(1, 2)).transpose(1, 2)

    def ref():
        os.environ["KF_ATTN_D64"] = "0"
        try:
            return ops.flash_attention(q, k, v, causal=False, kv_len=kv_len)
        finally:
            os.environ["KF_ATTN_D64"] = "1"

    def d128():
        return ops.flash_attention(q2, k2, v2, causal=False)

    comps = {"a_native_d64": (native, (q, k, v), do),
             "b_torch_sdpa": (sdpa, (q, k, v), do),
             "c_reference": (ref, (q, k, v), do)}
    if kv_len is None:
        comps["d_native_d128"] = (d128, (q2, k2, v2), do2)
    return comps


def _measure(comps, window, repeats, label=""):
    """{name: {"fwd": [ms per repeat], "fwdbwd": [...]}}, the competitors
    alternated inside each repeat."""
    runs = {}
    for name, (fn, leaves, do) in comps.items():
        def fwd(fn=fn):
            with torch.no_grad():
                fn()

        def fwdbwd(fn=fn, leaves=leaves, do=do):
            fn().backward(do)
            for t in leaves:
                t.grad = None

        try:
            runs[name] = (fwd, _iters_for(fwd, window), fwdbwd,
                          _iters_for(fwdbwd, window))
        except Exception as e:  # a competitor missing on this build
            print(f"{label} {name}: unavailable ({e})", flush=True)
    times = {n: {"fwd": [], "fwdbwd": []} for n in runs}
    for _ in range(repeats):
        for name, (fwd, nf, fwdbwd, nb) in runs.items():
            times[name]["fwd"].append(_ms(fwd, nf))
            times[name]["fwdbwd"].append(_ms(fwdbwd, nb))
    return times


def _med(xs):
    return sorted(xs)[len(xs) // 2]


def _spread(xs):
    return (max(xs) - min(xs)) / _med(xs)


def _varlen_rows(dev, window, repeats):
    B, S, H = 64, 512, 12
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(B, S, H, 64, generator=g)
               .to(dev, torch.bfloat16).requires_grad_(True)
               for _ in range(3))
    do = torch.randn(B, S, H, 64, generator=g).to(dev, torch.bfloat16)
    lens = torch.randint(16, S + 1, (B,), generator=g)
    sl = lens.to(dev, torch.int32)
    max_len = int(lens.max())
    ideal = float((lens.double() ** 2).sum()) / (B * S * max_len)
    keep = (torch.arange(S)[None, :] < lens[:, None]).to(dev)[:, None, None]

    def sdpa_mask():
        return F.scaled_dot_product_attention(
            q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
            attn_mask=keep).transpose(1, 2)

    full = torch.full((B,), S, dtype=torch.int32, device=dev)
    rows = {
        "mixed": {
            "a_varlen": lambda: ops.flash_attention(
                q, k, v, causal=False, seq_lens=sl),
            "b_scalar_maxlen": lambda: ops.flash_attention(
                q, k, v, causal=False, kv_len=max_len),
            "c_torch_sdpa_mask": sdpa_mask},
        "uniform": {
            "a_varlen": lambda: ops.flash_attention(
                q, k, v, causal=False, seq_lens=full),
            "b_scalar": lambda: ops.flash_attention(q, k, v, causal=False)},
    }
    print(f"\nvarlen: B{B} S{S} H{H} D64, lengths seed 0: min "
          f"{int(lens.min())} mean {float(lens.float().mean()):.1f} max "
          f"{max_len}; ideal sum(len^2)/(B*S*max) = {ideal:.3f}")
    for rname, fns in rows.items():
        comps = {n: (fn, (q, k, v), do) for n, fn in fns.items()}
        times = _measure(comps, window, repeats, f"varlen {rname}")
        print(f"\nvarlen {rname}:")
        print("| competitor | fwd ms (min..max) | fwd+bwd ms (min..max) |")
        print("|---|---|---|")
        for name, t in times.items():
            f, fb = sorted(t["fwd"]), sorted(t["fwdbwd"])
            print(f"| {name} | {_med(f):.3f} ({f[0]:.3f}..{f[-1]:.3f}) | "
                  f"{_med(fb):.3f} ({fb[0]:.3f}..{fb[-1]:.3f}) |")
            print(json.dumps({"shape": f"varlen_{rname}", "competitor": name,
                              "fwd_ms": t["fwd"],
                              "fwdbwd_ms": t["fwdbwd"]}), flush=True)
        a = times["a_varlen"]
        b = times["b_scalar_maxlen" if rname == "mixed" else "b_scalar"]
        out = {"shape": f"varlen_{rname}", "ratio_a_over_b": {
            kind: _med(a[kind]) / _med(b[kind]) for kind in a}}
        if rname == "mixed":
            out["ideal"] = ideal
        else:
            out["spread"] = {kind: {"a": _spread(a[kind]),
                                    "b": _spread(b[kind])} for kind in a}
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("all", "scalar", "varlen"),
                    default="all")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if args.only == "varlen":
        return _varlen_rows(dev, args.window, args.repeats)

    for sname, sh in SHAPES.items():
        B, S, H, kv_len = sh["B"], sh["S"], sh["H"], sh["kv_len"]
        fwd_flops = 4.0 * B * H * S * (kv_len or S) * 64
        comps = _competitors(B, S, H, kv_len, dev)
        times = _measure(comps, args.window, args.repeats, sname)
        print(f"\n{sname}: B{B} S{S} H{H} D64 kv_len={kv_len or S} "
              f"(d: H{H // 2} D128)")
        print("| competitor | fwd ms (min..max) | fwd TF | fwd+bwd ms "
              "(min..max) | bwd TF |")
        print("|---|---|---|---|---|")
        for name, t in times.items():
            f, fb = sorted(t["fwd"]), sorted(t["fwdbwd"])
            fmed, fbmed = f[len(f) // 2], fb[len(fb) // 2]
            bwd = max(fbmed - fmed, 1e-6)
            print(f"| {name} | {fmed:.3f} ({f[0]:.3f}..{f[-1]:.3f}) | "
                  f"{fwd_flops / fmed / 1e9:.1f} | {fbmed:.3f} "
                  f"({fb[0]:.3f}..{fb[-1]:.3f}) | "
                  f"{2.5 * fwd_flops / bwd / 1e9:.1f} |")
            print(json.dumps({"shape": sname, "competitor": name,
                              "fwd_ms": t["fwd"], "fwdbwd_ms": t["fwdbwd"],
                              "fwd_tf": fwd_flops / fmed / 1e9,
                              "bwd_tf": 2.5 * fwd_flops / bwd / 1e9}),
                  flush=True)
    if args.only == "all":
        _varlen_rows(dev, args.window, args.repeats)


if __name__ == "__main__":
    main()
