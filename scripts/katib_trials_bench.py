"""Measured Katib trial throughput (VERDICT round-1 item 8): N concurrent
BERT fine-tune trials sharing the available GPUs via gpu_shared
co-scheduling. Prints one JSON line with measured trials/hour.

usage: katib_trials_bench.py [parallel] [total] [steps] [--model NAME]
(--model defaults to bert-base-hd128, the config behind the published
number; bert-base is the real 12 x 64 config)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kubeflow_amd.api import new_object
from kubeflow_amd.api.objects import has_condition
from kubeflow_amd.platform import Platform

PARAMS = [
    {"name": "lr", "parameterType": "double",
     "feasibleSpace": {"min": "1e-5", "max": "1e-3"}},
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parallel", nargs="?", type=int, default=2)
    ap.add_argument("total", nargs="?", type=int, default=6)
    ap.add_argument("steps", nargs="?", type=int, default=50)
    ap.add_argument("--model", default="bert-base-hd128")
    args = ap.parse_args()
    parallel, total, steps = args.parallel, args.total, args.steps
    root = os.path.join("/tmp", f"katib-bench-{int(time.time())}")
    with Platform(root_dir=root) as plat:
        exp = new_object("Experiment", "bert-hpo", "default", spec={
            "objective": {"type": "minimize",
                          "objectiveMetricName": "loss"},
            "algorithm": {"algorithmName": "random"},
            "parallelTrialCount": parallel,
            "maxTrialCount": total,
            "maxFailedTrialCount": 2,
            "parameters": PARAMS,
            "trialTemplate": {"model": args.model, "steps": steps,
                              "micro_batch": 32, "seq_len": 512,
                              "gpus_per_replica": 1, "gpu_shared": True,
                              "gpu_memory": "48Gi", "status_every": 10,
                              "save_final": False, "replicas": 1},
        })
        t0 = time.time()
        plat.store.create(exp)
        deadline = time.time() + 3600
        while time.time() < deadline:
            obj = plat.store.get("Experiment", "bert-hpo", "default")
            if has_condition(obj, "Succeeded") or has_condition(obj, "Failed"):
                break
            time.sleep(1)
        wall = time.time() - t0
        st = obj["status"]
        done = st.get("trialsSucceeded", st.get("trials", 0))
        print(json.dumps({
            "metric": "katib_trials_per_hour",
            "value": round(done * 3600 / wall, 1),
            "trials_succeeded": done,
            "parallel": parallel,
            "wall_s": round(wall, 1),
            "steps_per_trial": steps,
            "model": args.model,
            "gpus": plat.scheduler.inv.n_gpus,
            "measured": True,
        }), flush=True)


if __name__ == "__main__":
    main()
