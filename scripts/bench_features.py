#!/usr/bin/env python3
"""The strategic feature planes (gvec_obs_features, obs_features_kernel) on observations of games in progress, against a
torch formulation of the same definition, in one process:
  hip     features.strategic_features on [N, 9, H, W] observations taken from a GeneralsSelfPlayVecEnv after `--age` turns of
          random legal actions (both learners' views of every board)
  torch   the definition as iterated masked dilation on the device: per level four shifted ORs and a mask for the four
          searches at once, to the fixpoint of the batch (one host read per level: the loop has to know when to stop)
The two results are compared bit for bit before anything is timed.  Times are wall-clock per call (median of the repeats, every
call enqueued, one synchronisation per repeat); the kernel's own time comes from a separate rocprofv3 --kernel-trace --stats
run of this script per shape with --skip-torch; `--merge wall.json --kernel-stats config=kernel_stats.csv,...`
folds those into the result file afterwards (no GPU needed).
Bytes: by construction a row reads five planes and writes five, 2 * 5 * H * W * 4 B; the floor is that over the copy rate
bench.py reports (--copy-tbs).
usage: scripts/bench_features.py [--calls K] [--repeats R] [--age T] [--skip-torch] [--configs ...] [--out file.json]
       scripts/bench_features.py --merge wall.json --kernel-stats 8192:20x20:2=a.csv,4096:15x15:2=b.csv --out profiles/features_bench.json"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--age", type=int, default=100)
ap.add_argument("--cap", type=int, default=64)
ap.add_argument("--configs", default="8192:20x20:2,4096:15x15:2", help="envs:WxH:players - envs * players observations each")
ap.add_argument("--copy-tbs", type=float, default=6.29)
ap.add_argument("--skip-torch", action="store_true")
ap.add_argument("--merge", default=None, help="a result file of this script to add kernel times to")
ap.add_argument("--kernel-stats", default=None, help="config=rocprofv3 kernel_stats.csv of a --skip-torch run of that config alone, ...")
ap.add_argument("--out", default=None)
args = ap.parse_args()


def kernel_us(path):
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "obs_features_kernel" in row.get("Name", ""):
                return {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                        "max_us": float(row["MaxNs"]) / 1e3}
    return None


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
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

from generalsreinforcementlearning_amd.features import strategic_features  # noqa: E402
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


def observations(B, w, h, P):
    env = GeneralsSelfPlayVecEnv(B, w, h, max_players=P, device_outputs=True, seed=5)
    obs, info = env.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for _ in range(args.age):
        m = info["valid_actions_mask"].reshape(B * P, -1).float() + 1e-6
        obs, _, _, _, info = env.step(torch.multinomial(m, 1, generator=gen).reshape(B, P))
    out = obs.reshape(B * P, 9, h, w).clone()
    env.close()
    return out


def torch_features(obs, cap):
    """-> (features [N, 5, H, W], uncapped distances int32 [N, 4, H, W] with -1 = no path, levels walked)"""
    vis, mine, enemy = obs[:, 0] != 0, obs[:, 1] == 0.5, obs[:, 1] == 1.0
    passable, city, gen = obs[:, 4] == 0, obs[:, 5] != 0, obs[:, 6] != 0

    def around(m):
        r = torch.zeros_like(m)
        r[..., 1:, :] |= m[..., :-1, :]
        r[..., :-1, :] |= m[..., 1:, :]
        r[..., :, 1:] |= m[..., :, :-1]
        r[..., :, :-1] |= m[..., :, 1:]
        return r

    free = passable[:, None].expand(-1, 4, -1, -1)
    frontier = torch.stack([gen & mine, enemy, city & ~mine, ~vis], dim=1) & free
    dist = torch.where(frontier, 0, -1).to(torch.int32)
    level = 0
    while bool(frontier.any()):
        level += 1
        frontier = around(frontier) & free & (dist < 0)
        dist = torch.where(frontier, level, dist)
    f = torch.empty((obs.shape[0], 5) + tuple(obs.shape[2:]), dtype=torch.float32, device=obs.device)
    f[:, :4] = torch.where(dist < 0, 1.0, dist.clamp(max=cap).float() / cap)
    f[:, 4] = (mine & around(enemy)).float()
    return f, dist, level


res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "age_turns": args.age, "cap": args.cap,
       "copy_tbs": args.copy_tbs, "shapes": []}
for c in args.configs.split(","):
    b, wh, p = c.split(":")
    w, h = (int(v) for v in wh.split("x"))
    B, P = int(b), int(p)
    obs = observations(B, w, h, P)
    N = obs.shape[0]
    out = torch.empty((N, 5, h, w), dtype=torch.float32, device="cuda")
    row = {"config": c, "observations": N, "bytes_per_row": 2 * 5 * h * w * 4, "bytes": N * 2 * 5 * h * w * 4}
    row["floor_us"] = row["bytes"] / (args.copy_tbs * 1e12) * 1e6
    t_hip = timed(lambda: strategic_features(obs, cap=args.cap, out=out), args.calls, args.repeats)
    row["hip_wall_us"] = t_hip * 1e6
    row["hip_wall_floor_fraction"] = row["floor_us"] / row["hip_wall_us"]
    if not args.skip_torch:
        ref, dist, levels = torch_features(obs, args.cap)
        row["equal_to_torch"] = bool(torch.equal(ref, strategic_features(obs, cap=args.cap)))
        deepest = dist.reshape(N, 4, -1).max(dim=2).values.clamp(min=0).float()       # levels a search of one row runs
        row["levels_batch_fixpoint"] = levels
        row["levels_per_bfs_mean"] = float(deepest.mean())
        row["levels_per_bfs_by_plane"] = [float(v) for v in deepest.mean(dim=0)]
        row["levels_per_row_mean"] = float(deepest.max(dim=1).values.mean())           # the kernel's loop: the deepest of a row's four
        row["levels_per_row_max"] = int(deepest.max())
        row["share_below_one"] = float((ref[:, :4] < 1.0).float().mean())
        t_torch = timed(lambda: torch_features(obs, args.cap), max(1, args.calls // 4), args.repeats)
        row["torch_wall_us"] = t_torch * 1e6
        row["torch_over_hip"] = t_torch / t_hip
    res["shapes"].append(row)
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
