#!/usr/bin/env python3
"""The scripted opponent (gvec_bot_actions, bot_kernel) at the engine's batch sizes, in one process:
  bot_all / bot_one   gvec_bot_actions into device memory for every seat / for seat 1 only, on mid-game boards (after
                      `--age` random-agent turns), against step_kernel (one per-turn gvec_rollout call) on the same batch
  env_bot / env_rand  GeneralsVecEnv(device_outputs=True).step with opponent="bot" against the default random opponent
                      (one gvec_gym_step launch), learner actions drawn from the mask on the device
Times are wall-clock per call (median of the repeats, every call enqueued, one synchronisation per repeat).  Bytes: what
query_kernel reads (header, mutable and constant planes, narrow armies) plus 8 B per written slot; kernel times come from
a separate rocprofv3 --kernel-trace --stats run of this script.
usage: scripts/bench_bot.py [--calls K] [--repeats R] [--age T] [--skip-env] [--out file.json]"""
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
ap.add_argument("--age", type=int, default=100)
ap.add_argument("--engine-config", default="262144:20x20:4")
ap.add_argument("--env-configs", default="4096:15x15:2,65536:15x15:2")
ap.add_argument("--skip-env", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()


def timed(fn, calls, repeats):
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / calls)
    runs.sort()
    return runs[len(runs) // 2]


def parse(c):
    b, wh, p = c.split(":")
    w, h = wh.split("x")
    return int(b), int(w), int(h), int(p)


def engine_bench(B, w, h, P):
    stream = torch.cuda.current_stream().cuda_stream
    e = g.VecEngine(B, w, h, P, stream=stream)
    e.reset_generated(1)
    e.rollout(args.age, 7, 0, fused=False, want_stats=False)
    st = e.game_state(fields=("done", "alive"))
    tr = e.step_traffic_bytes()
    acts = torch.zeros((B, P, 8), dtype=torch.uint8, device="cuda")
    full = (1 << P) - 1
    t_all = timed(lambda: e.bot_actions_device(full, 0, 0, acts.data_ptr()), args.calls, args.repeats)
    t_one = timed(lambda: e.bot_actions_device(0b10, 0, 0, acts.data_ptr()), args.calls, args.repeats)
    t_mix = timed(lambda: e.bot_actions_device(full, 0, 100, acts.data_ptr()), args.calls, args.repeats)
    # the step kernel on a copy of the same boards would need a second batch; a per-turn rollout call on this one moves
    # the games on by `calls * repeats` turns, so it is timed last
    t_step = timed(lambda: e.rollout_range(0, B, 1, 9), args.calls, args.repeats)
    read = tr["read"]
    res = {"config": f"{B}:{w}x{h}:{P}", "age_turns": args.age, "done_envs": int(st["done"].sum()),
           "alive_seats": int(st["alive"].sum()), "read_bytes_per_env": read,
           "bot_all_ms": t_all * 1e3, "bot_one_ms": t_one * 1e3, "bot_all_permille100_ms": t_mix * 1e3, "step_rollout_ms": t_step * 1e3,
           "bot_all_over_step": t_all / t_step,
           "bot_all_bytes": B * (read + 8 * P), "bot_one_bytes": B * (read + 8),
           "bot_all_wall_tbs": B * (read + 8 * P) / t_all / 1e12}
    e.close()
    return res


def env_bench(B, w, h, P):
    out = {"config": f"{B}:{w}x{h}:{P}"}
    for opp in ("random", "bot"):
        env = GeneralsVecEnv(B, w, h, P, device_outputs=True, opponent=opp, seed=3)
        _, info = env.reset()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)
        state = {"mask": info["valid_actions_mask"]}

        def step():
            m = state["mask"].reshape(B, -1).float() + 1e-6
            a = torch.multinomial(m, 1, generator=gen).reshape(-1)
            r = env.step(a)
            state["mask"] = r[4]["valid_actions_mask"]

        for _ in range(50):
            step()
        out[f"env_{opp}_ms"] = timed(step, args.calls, args.repeats) * 1e3
        out[f"env_{opp}_steps_per_s"] = B / out[f"env_{opp}_ms"] * 1e3
        env.close()
    # the learner-action draw (torch.multinomial) is in both numbers
    out["bot_over_random"] = out["env_bot_ms"] / out["env_random_ms"]
    return out


res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats,
       "engine": engine_bench(*parse(args.engine_config))}
if not args.skip_env:
    res["env"] = [env_bench(*parse(c)) for c in args.env_configs.split(",")]
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
