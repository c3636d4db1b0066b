"""Classifier-serving throughput (GPU): N concurrent clients issue
fixed-length classify requests against one InferenceEngine for a fixed
window. Prints one JSON line: requests/s and latency p50.

Usage: python scripts/classify_bench.py --model bert-base
           [--concurrency 64] [--prompt-len 128] [--seconds 5]
"""
import argparse
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from kubeflow_amd.runtime.serving import InferenceEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--concurrency", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=5.0)
    args = ap.parse_args()

    eng = InferenceEngine(args.model, device=torch.device("cuda", 0),
                          max_batch=args.concurrency)
    eng.start()
    prompt = [2 + i % 1000 for i in range(args.prompt_len)]
    lat, errors = [], []
    lock = threading.Lock()
    try:
        for _ in range(3):  # warm-up: allocator, kernel load
            r = eng.generate(prompt, timeout=120)
            assert not r.error, r.error
        stop_at = time.time() + args.seconds

        def client():
            mine = []
            while time.time() < stop_at:
                t0 = time.time()
                r = eng.generate(prompt, timeout=120)
                if r.error:
                    errors.append(r.error)
                    return
                mine.append(time.time() - t0)
            with lock:
                lat.extend(mine)

        threads = [threading.Thread(target=client)
                   for _ in range(args.concurrency)]
        t0 = time.time()
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        wall = time.time() - t0
    finally:
        eng.stop()
    assert not errors, errors[:3]
    lat.sort()
    print(json.dumps({
        "metric": "classify_requests_per_s",
        "value": round(len(lat) / wall, 1),
        "model": args.model,
        "concurrency": args.concurrency,
        "prompt_len": args.prompt_len,
        "latency_p50_ms": round(lat[len(lat) // 2] * 1e3, 2),
        "requests": len(lat),
        "wall_s": round(wall, 2),
    }), flush=True)


if __name__ == "__main__":
    main()
