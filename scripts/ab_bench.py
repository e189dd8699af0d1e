#!/usr/bin/env python3
"""Interleaved A/B timing of two builds of libgvec_hip.so in ONE process on ONE device
(cdna_hip_programming.md 5.4 rule 24).   usage: scripts/ab_bench.py [--dup] [--json=OUT.json] libA.so libB.so [libC.so ...] [rounds] [steps]
--json=OUT.json also writes every round's raw per-turn and fused times (us) per build."""
import statistics as st
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from generalsreinforcementlearning_amd import _lib
from generalsreinforcementlearning_amd.vec_engine import VecEngine

json_out = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--json=")), None)
sys.argv = [a for a in sys.argv if not a.startswith("--json=")]
paths = [a for a in sys.argv[1:] if a.endswith(".so")]
if "--dup" in sys.argv:  # every build twice, interleaved: shows how much of a difference is buffer placement / order
    sys.argv.remove("--dup")
    paths = paths + paths
nums = [int(a) for a in sys.argv[1:] if not a.endswith(".so")]
rounds = nums[0] if len(nums) > 0 else 7
steps = nums[1] if len(nums) > 1 else 100
B, W, H, P = 262144, 20, 20, 4
engs = []
for p in paths:
    L = _lib.load_from(os.path.abspath(p))
    e = VecEngine(B, W, H, P, auto_reset=True, lib=L, stream=torch.cuda.current_stream().cuda_stream)
    e.reset_generated(1000003)
    e.build_board_pool(4096, 7919)
    e.rollout(20, 1, 0, fused=False, want_stats=False)
    engs.append(e)
torch.cuda.synchronize()
res = [[] for _ in engs]
fres = [[] for _ in engs]
for r in range(rounds):
    for i, e in enumerate(engs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.rollout(steps, 1, 0, fused=False, want_stats=False)
        b.record()
        torch.cuda.synchronize()
        res[i].append(a.elapsed_time(b) / steps)
        a.record()
        e.rollout(32, 2, 0, fused=True, want_stats=False)
        b.record()
        torch.cuda.synchronize()
        fres[i].append(a.elapsed_time(b) / 32)
for i, p in enumerate(paths):
    m, f = st.median(res[i]), st.median(fres[i])
    print(f"{p}: per-turn median {m*1e3:.1f} us/step (min {min(res[i])*1e3:.1f}, max-min {(max(res[i])-min(res[i]))*1e3:.1f}) -> {B/m/1e3:.1f} M steps/s | "
          f"fused {f*1e3:.1f} us/turn (max-min {(max(fres[i])-min(fres[i]))*1e3:.1f}) -> {B/f/1e3:.1f} M steps/s")
if json_out:
    import json
    us = lambda v: [round(x * 1e3, 2) for x in v]
    json.dump({"boards": [B, W, H, P], "rounds": rounds, "steps_per_round": steps, "order": "interleaved, one process, one device",
               "builds": [{"lib": p, "per_turn_us": us(res[i]), "per_turn_median_us": round(st.median(res[i]) * 1e3, 2),
                           "per_turn_max_minus_min_us": round((max(res[i]) - min(res[i])) * 1e3, 2),
                           "fused_us_per_turn": us(fres[i]), "fused_median_us": round(st.median(fres[i]) * 1e3, 2)} for i, p in enumerate(paths)]},
              open(json_out, "w"), indent=1)
