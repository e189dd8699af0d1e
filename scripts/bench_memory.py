#!/usr/bin/env python3
"""The fog-of-war memory planes (gvec_obs_memory_update, obs_memory_kernel) on observations of games in progress, against a
torch formulation of the same definition, in one process:
  hip     ObservationMemory.update(obs, reset) in place on [N, 9, H, W] observations taken from a GeneralsSelfPlayVecEnv after
          `--age` turns of random legal actions (both learners' views of every board), the memory carried through those turns
  torch   the same definition as torch elementwise ops (where / clamp / compares) on the same inputs, writing into the same
          kind of preallocated state
The two results are compared bit for bit before anything is timed.  Times are wall-clock per call (median of the repeats, every
call enqueued, one synchronisation per repeat); the kernel's own time comes from a separate rocprofv3 --kernel-trace --stats
run of this script per shape with --skip-torch --skip-rollout; `--merge wall.json --kernel-stats
config=kernel_stats.csv,...` folds those into the result file afterwards (no GPU needed).
Bytes: by construction a row reads three observation planes and four planes of its state and writes four,
11 * H * W * 4 B; the floor is that over the copy rate bench.py reports (--copy-tbs).
  rollout ms per SelfPlayRolloutBuffer.step with and without memory=, alternating (next_rollout's slot copies every `horizon`
          steps included), next to the step time the parent commit's profiles/rollout_bench.json recorded for the same config
usage: scripts/bench_memory.py [--calls K] [--repeats R] [--age T] [--skip-torch] [--skip-rollout] [--configs ...] [--out file.json]
       scripts/bench_memory.py --merge wall.json --kernel-stats 8192:20x20:2=a.csv,4096:15x15:2=b.csv --out profiles/memory_bench.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--age", type=int, default=100)
ap.add_argument("--cap", type=int, default=64)
ap.add_argument("--configs", default="8192:20x20:2,4096:15x15:2", help="envs:WxH:players - envs * players rows each")
ap.add_argument("--rollout-config", default="4096:15x15:2:32", help="envs:WxH:players:horizon, a config of profiles/rollout_bench.json")
ap.add_argument("--rollout-steps", type=int, default=64)
ap.add_argument("--copy-tbs", type=float, default=6.29)
ap.add_argument("--skip-torch", action="store_true")
ap.add_argument("--skip-rollout", action="store_true")
ap.add_argument("--merge", default=None, help="a result file of this script to add kernel times to")
ap.add_argument("--kernel-stats", default=None, help="config=rocprofv3 kernel_stats.csv of a --skip-torch run of that config alone, ...")
ap.add_argument("--out", default=None)
args = ap.parse_args()


def kernel_us(path):
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "obs_memory_kernel" in row.get("Name", ""):
                return {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                        "max_us": float(row["MaxNs"]) / 1e3}
    return None


def finish(res):
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if args.merge:
    res = json.load(open(args.merge))
    stats = dict(item.split("=", 1) for item in args.kernel_stats.split(","))
    for row in res["shapes"]:
        k = kernel_us(stats[row["config"]]) if row["config"] in stats else None
        if k:
            row["kernel"] = k
            row["kernel_floor_fraction"] = row["floor_us"] / k["avg_us"]
            row["kernel_tbs"] = row["bytes"] / (k["avg_us"] * 1e-6) / 1e12
            if "torch_wall_us" in row:
                row["torch_wall_over_kernel"] = row["torch_wall_us"] / k["avg_us"]
    finish(res)
    sys.exit(0)

import torch  # noqa: E402

from generalsreinforcementlearning_amd.memory import ObservationMemory  # noqa: E402
from generalsreinforcementlearning_amd.rollout import SelfPlayRolloutBuffer  # noqa: E402
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv  # noqa: E402


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


def random_legal(mask, gen):
    m = mask.reshape(-1, mask.shape[-1]).float() + 1e-6
    return torch.multinomial(m, 1, generator=gen).reshape(mask.shape[:-1])


def game_in_progress(B, w, h, P):
    """(observation [B, P, 9, h, w] after --age turns, the memory of those turns [B, P, 4, h, w], the last step's reset flags)"""
    env = GeneralsSelfPlayVecEnv(B, w, h, max_players=P, device_outputs=True, seed=5)
    mem = ObservationMemory((B, P), h, w, cap=args.cap)
    obs, info = env.reset()
    mem.update(obs)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for k in range(args.age):
        if k == args.age - 1:
            before = mem.planes.clone()
        obs, _, _, _, info = env.step(random_legal(info["valid_actions_mask"], gen))
        mem.update(obs, info["reset"])
    out = obs.clone(), before, info["reset"].clone()
    env.close()
    return out


def torch_update(prev, obs, reset, cap, out):
    """the definition as torch elementwise ops: prev / out [B, P, 4, h, w], obs [B, P, 9, h, w], reset [B]"""
    fresh = reset.bool()[:, None, None, None]
    zero, one = torch.zeros((), device=obs.device), torch.ones((), device=obs.device)
    vis = obs[:, :, 0] != 0
    seen = torch.where(fresh, zero, prev[:, :, 0])
    age = torch.where(fresh, one, prev[:, :, 3])
    older = torch.clamp(age * cap + 1.0, max=float(cap)) / cap
    torch.where(vis, one, seen, out=out[:, :, 0])
    out[:, :, 1] = torch.where(vis, obs[:, :, 1], torch.where(fresh, zero, prev[:, :, 1]))
    out[:, :, 2] = torch.where(vis, obs[:, :, 2], torch.where(fresh, zero, prev[:, :, 2]))
    out[:, :, 3] = torch.where(vis, zero, torch.where(seen != 0, older, one))
    return out


res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "age_turns": args.age, "cap": args.cap,
       "copy_tbs": args.copy_tbs, "shapes": []}
for c in args.configs.split(","):
    b, wh, p = c.split(":")
    w, h = (int(v) for v in wh.split("x"))
    B, P = int(b), int(p)
    obs, prev, reset = game_in_progress(B, w, h, P)
    N = B * P
    row = {"config": c, "rows": N, "bytes_per_row": 11 * h * w * 4, "bytes": N * 11 * h * w * 4}
    row["floor_us"] = row["bytes"] / (args.copy_tbs * 1e12) * 1e6
    mem = ObservationMemory((B, P), h, w, cap=args.cap)
    want = mem.update(obs, reset, out=torch.empty_like(prev)).clone()       # prev is blank here: the first update's path
    mem.load_state_dict({"planes": prev, "cap": args.cap, "rows_shape": (B, P), "height": h, "width": w})
    got = mem.update(obs, reset, out=torch.empty_like(prev)).clone()
    row["seen_share"] = float(got[:, :, 0].mean())
    row["aging_share"] = float(((got[:, :, 3] > 0) & (got[:, :, 3] < 1)).float().mean())
    row["reset_flags_set"] = int(reset.sum())
    # timed in place from the state after `age` turns: ages keep growing, which changes no cost
    t_hip = timed(lambda: mem.update(obs, reset), args.calls, args.repeats)
    row["hip_wall_us"] = t_hip * 1e6
    row["hip_wall_floor_fraction"] = row["floor_us"] / row["hip_wall_us"]
    if not args.skip_torch:
        ref = torch_update(prev, obs, reset, args.cap, torch.empty_like(prev))
        row["equal_to_torch"] = bool(torch.equal(ref.view(torch.int32), got.view(torch.int32)))
        blank = torch.zeros_like(prev)
        blank[:, :, 3] = 1.0
        row["equal_to_torch_from_blank"] = bool(torch.equal(torch_update(blank, obs, reset, args.cap, torch.empty_like(prev)).view(torch.int32),
                                                            want.view(torch.int32)))
        state = prev.clone()
        t_torch = timed(lambda: torch_update(state, obs, reset, args.cap, state), args.calls, args.repeats)
        row["torch_wall_us"] = t_torch * 1e6
        row["torch_over_hip"] = t_torch / t_hip
    res["shapes"].append(row)

if not args.skip_rollout:
    b, wh, p, T = args.rollout_config.split(":")
    w, h = (int(v) for v in wh.split("x"))
    B, P, T = int(b), int(p), int(T)
    zeros = torch.zeros(B, P, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)

    def stepper(with_memory):
        env = GeneralsSelfPlayVecEnv(B, w, h, max_players=P, device_outputs=True, seed=5)
        buf = SelfPlayRolloutBuffer(env, horizon=T, memory=ObservationMemory((B, P), h, w, cap=args.cap) if with_memory else None)
        buf.begin(*env.reset())
        actions = torch.zeros(B, P, dtype=torch.int64, device="cuda")

        def step():
            if buf.full:
                buf._finished = True                                        # the slot copies of next_rollout, without the GAE
                buf.next_rollout()
            buf.step(actions, zeros, zeros)
        return step

    fns = {"buffer_step": stepper(False), "buffer_step_memory": stepper(True)}
    for f in fns.values():
        for _ in range(3):
            f()
    times = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.rollout_steps):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.rollout_steps * 1e3)
    ro = {"config": args.rollout_config, "steps": args.rollout_steps}
    for k, v in times.items():
        ro[k] = {"ms": round(sorted(v)[len(v) // 2], 5), "ms_all": [round(x, 5) for x in v]}
    ro["memory_over_plain_ms"] = round(ro["buffer_step_memory"]["ms"] - ro["buffer_step"]["ms"], 5)
    try:
        for r in json.load(open(os.path.join(ROOT, "profiles", "rollout_bench.json")))["rows"]:
            if (r["envs"], r["board"], r["players"], r["horizon"]) == (B, wh, P, T):
                ro["parent_buffer_step_ms"] = r["step"]["buffer_step"]["ms"]   # recorded by scripts/bench_rollout.py on the parent commit
    except (OSError, KeyError, ValueError):
        pass
    res["rollout"] = ro
finish(res)
