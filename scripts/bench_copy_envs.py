#!/usr/bin/env python3
"""gvec_copy_envs (on-device clone / save / restore of env states) against the route that existed before it, per
configuration, in one process:
  disjoint   full-batch copy of half the envs onto the other half (n = B/2 pairs, one handle)
  fanout     1 -> 64 fan-out: B/128 roots, each copied to 64 destinations (n = B/2 pairs, one handle)
  save       every env into a second handle of the same config (n = B pairs)
  route      what a user had before, for the disjoint pairs: gvec_export_records of the batch -> torch gather of the three
             slab segments by source -> gvec_import_records of the destination run
  branch     the search primitive on GeneralsVecEnv: copy_envs(check=False) of the fan-out pairs (incl. its observe pass)
             + one step (gvec_gym_step over the batch); reported as branch evaluations/s = n / time
Times are wall-clock per call (every copy synchronises its stream: the range check), median of the repeats.  Bytes per
pair are computed from the resident layout below (read = written).  Kernel times: run it under rocprofv3 --kernel-trace
--stats and divide the bytes by copy_envs_kernel's average duration.
usage: scripts/bench_copy_envs.py [--calls K] [--repeats R] [--configs B:WxH:P,...] [--out file.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import generalsreinforcementlearning_amd as g
from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--configs", default="262144:20x20:4,65536:15x15:2")
ap.add_argument("--out", default=None)
args = ap.parse_args()


def pair_bytes(e, gym=False):
    """Bytes one pair moves each way, from the layout (gvec_api.hip set_geometry): header 96, planes row_dw dwords
    ((3*MAXP + 13) planes of fd dwords, padded to 4), narrow armies NSLOT*128 (wide envs: twice that), and in a gym
    handle the reward-baseline row of 3*MAXP int32."""
    lay = e.experience_record_layout()
    mp, fd, ns = lay["mp"], lay["fd"], lay["ns"]
    row_dw = ((3 * mp + 13) * fd + 3) // 4 * 4
    return {"header": 96, "planes": 4 * row_dw, "army": ns * 128, "gym_prev": 12 * mp if gym else 0,
            "total": 96 + 4 * row_dw + ns * 128 + (12 * mp if gym else 0)}


def timed(fn, calls, repeats):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        best.append((time.perf_counter() - t0) / calls)
    best.sort()
    return best[len(best) // 2]


def run(B, w, h, P):
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    e = g.VecEngine(B, w, h, P, auto_reset=True, stream=stream)
    e.reset_generated(1)
    e.rollout(8, seed=2, fused=False, want_stats=False)
    half = B // 2
    dst = torch.arange(half, B, device=dev, dtype=torch.int32)
    src = torch.arange(0, half, device=dev, dtype=torch.int32)
    roots = torch.arange(0, half, 64, device=dev, dtype=torch.int32)      # B/128 roots in the first half
    fan = roots.repeat_interleave(64)
    other = g.VecEngine(B, w, h, P, auto_reset=True, stream=stream)
    other.reset_generated(3)
    nb = e.state_bytes_per_env()
    slab = torch.empty(B * nb, dtype=torch.uint8, device=dev)
    lay = e.experience_record_layout()
    seg = [96, nb - 96 - lay["ns"] * 256, lay["ns"] * 256]                 # record slab: headers | planes | int32 armies
    src64 = src.long()

    def route():
        e.export_records(slab.data_ptr())
        parts, off = [], 0
        for size in seg:
            parts.append(slab[off: off + B * size].view(B, size)[src64].reshape(-1))
            off += B * size
        e.import_records(torch.cat(parts).data_ptr(), half, half)

    pb = pair_bytes(e)
    res = {"envs": B, "board": f"{w}x{h}", "players": P, "bytes_per_pair": pb}
    for name, fn, n in (("disjoint", lambda: e.copy_envs(dst, src), half), ("fanout", lambda: e.copy_envs(dst, fan), half),
                        ("save", lambda: other.copy_envs(src=e), B), ("route", route, half)):
        t = timed(fn, args.calls, args.repeats)
        res[name] = {"pairs": n, "ms": round(t * 1e3, 4), "pairs_per_s": round(n / t), "GB_per_s_each_way": round(n * pb["total"] / t / 1e9, 1)}
    res["route_over_disjoint"] = round(res["route"]["ms"] / res["disjoint"]["ms"], 2)
    del e, other, slab
    torch.cuda.empty_cache()
    # the search primitive on the gym env: fan-out + one step of the whole batch
    env = GeneralsVecEnv(B, w, h, P, max_turns=10 ** 6, seed=4, device_outputs=True)
    obs, info = env.reset()
    acts = torch.argmax(info["valid_actions_mask"].to(torch.uint8), dim=1).contiguous()
    d64, f64 = dst.long(), fan.long()

    def branch():
        env.copy_envs(d64, f64, check=False)
        env.step(acts)

    t = timed(branch, args.calls, args.repeats)
    t_step = timed(lambda: env.step(acts), args.calls, args.repeats)
    res["branch"] = {"pairs": half, "ms": round(t * 1e3, 4), "branch_evals_per_s": round(half / t), "step_alone_ms": round(t_step * 1e3, 4),
                     "bytes_per_pair_gym": pair_bytes(env.engine, gym=True)["total"]}
    env.close()
    return res


out = {"bench": "copy_envs", "device": torch.cuda.get_device_name(0), "results": []}
for c in args.configs.split(","):
    b, wh, p = c.split(":")
    w, h = wh.split("x")
    out["results"].append(run(int(b), int(w), int(h), int(p)))
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
