#!/usr/bin/env python3
"""Host cost per call of the five observation-batch fronts (strategic_features, ObservationMemory.update,
valid_actions_mask_from_observation, double_q_target, categorical_target) at 4 rows of 5x5, where the Python front and the C
argument checks, not the kernel, are what a call costs.

usage: scripts/bench_obs_front.py [--calls K] [--warmup W] [--label NAME] [--out file.json]

Every call is timed on the host (perf_counter around the call: checks, result tensors, struct, launch); nothing synchronises
with the device until after the last call of an entry point.  Prints one JSON line with the median (and the 10th and 90th
percentile) in microseconds per entry point; --out appends that object to the JSON list in the file, so that runs of several
builds (profiles/obs_batch_host_cost.json: parent, result, parent again) end up side by side."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import generalsreinforcementlearning_amd as g
    dev = torch.device("cuda", 0)
    rows, H, W, N = 4, 5, 5, 51
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    obs = (torch.rand(rows, 9, H, W, device=dev, generator=gen) < 0.5).float()
    q = torch.randn(rows, 5 * H * W, device=dev, generator=gen)
    logits = torch.randn(rows, 5 * H * W, N, device=dev, generator=gen)
    reward, done = torch.randn(rows, device=dev, generator=gen), torch.zeros(rows, dtype=torch.bool, device=dev)
    mem = g.ObservationMemory((rows,), H, W)
    entries = {"strategic_features": lambda: g.strategic_features(obs),
               "ObservationMemory.update": lambda: mem.update(obs),
               "valid_actions_mask_from_observation": lambda: g.valid_actions_mask_from_observation(obs),
               "double_q_target": lambda: g.double_q_target(obs, q, reward, 0.99, done, q_select=q),
               "categorical_target": lambda: g.categorical_target(obs, logits, reward, 0.99, done, -10.0, 10.0, logits_select=logits)}
    result = {"label": args.label, "rows": rows, "board": f"{W}x{H}", "calls": args.calls, "device": torch.cuda.get_device_name(0),
              "median_us": {}, "p10_us": {}, "p90_us": {}}
    clock = time.perf_counter
    for name, call in entries.items():
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        took = [0.0] * args.calls
        for i in range(args.calls):
            t0 = clock()
            call()
            took[i] = clock() - t0
        torch.cuda.synchronize()
        took.sort()
        for key, at in (("median_us", 0.5), ("p10_us", 0.1), ("p90_us", 0.9)):
            result[key][name] = round(1e6 * took[int(at * (args.calls - 1))], 3)
    print(json.dumps(result))
    if args.out:
        runs = json.load(open(args.out)) if os.path.exists(args.out) else []
        runs.append(result)
        with open(args.out, "w") as f:
            json.dump(runs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
