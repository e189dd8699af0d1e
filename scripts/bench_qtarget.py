#!/usr/bin/env python3
"""The masked Q targets (gvec_obs_valid_mask, gvec_q_target, gvec_categorical_target) on next observations of games in
progress, against the same definitions written in torch, in one process:
  hip     valid_actions_mask_from_observation / double_q_target / categorical_target (q_targets.py) on [rows, 9, H, W]
          observations taken from a GeneralsSelfPlayVecEnv after `--age` turns of random legal actions (every learner's view
          of every board: what a replay ring of that game holds as next_state), Double targets: a selection and an
          evaluation network's output, random values at every action
  torch   the mask built from the observation by torch ops (compares, shifted slices), then masked_fill + argmax + gather
          for the scalar target, and softmax over all [rows, A, N] logits, expected values, masked argmax and the usual
          floor / ceil scatter_add projection for the categorical one
The results are compared before anything is timed.  Times are wall-clock per call (median of the repeats, every call
enqueued, one synchronisation per repeat).  Bytes are what each formulation has to move by construction: the kernels read
three observation planes, the values of the legal actions only and write their outputs; the torch formulation reads every
value of every action at least once.
usage: scripts/bench_qtarget.py [--calls K] [--repeats R] [--age T] [--atoms N] [--configs envs:WxH:players,...] [--out file.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--age", type=int, default=100)
ap.add_argument("--atoms", type=int, default=51)
ap.add_argument("--v-min", type=float, default=-10.0)
ap.add_argument("--v-max", type=float, default=10.0)
ap.add_argument("--gamma", type=float, default=0.99)
ap.add_argument("--configs", default="512:15x15:2,8192:15x15:2,512:20x20:2,8192:20x20:2", help="envs:WxH:players - envs * players rows each")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from generalsreinforcementlearning_amd.q_targets import (categorical_target, double_q_target,  # noqa: E402
                                                         valid_actions_mask_from_observation)
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
    """every learner's observation [B * P, 9, h, w] after --age turns, and the env's own masks for them"""
    env = GeneralsSelfPlayVecEnv(B, w, h, max_players=P, device_outputs=True, seed=5)
    obs, info = env.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for _ in range(args.age):
        obs, _, _, _, info = env.step(random_legal(info["valid_actions_mask"], gen))
    out = obs.reshape(B * P, 9, h, w).clone(), info["valid_actions_mask"].reshape(B * P, -1).bool().clone()
    env.close()
    return out


def torch_mask(ns):
    src = (ns[:, 1] == 0.5) & (ns[:, 2] > 0.09)
    ok = ns[:, 4] == 0
    up, right = F.pad(ok[:, :-1], (0, 0, 1, 0)), F.pad(ok[:, :, 1:], (0, 1))
    down, left = F.pad(ok[:, 1:], (0, 0, 0, 1)), F.pad(ok[:, :, :-1], (1, 0))
    moves = torch.stack([up, right, down, left], -1) & src[..., None]
    return torch.cat([moves, moves.any(-1, keepdim=True)], -1).reshape(ns.shape[0], -1)


def torch_q_target(ns, q_eval, q_sel, r, gamma, d):
    mask = torch_mask(ns)
    a = q_sel.masked_fill(~mask, float("-inf")).argmax(1)
    boot = mask.any(1) & ~d
    nv = q_eval.gather(1, a[:, None]).squeeze(1) * boot
    return r + gamma * nv, torch.where(mask.any(1), a, -1)


def torch_categorical(ns, lg_eval, lg_sel, r, gamma, d, v_min, v_max):
    rows, A, N = lg_eval.shape
    mask = torch_mask(ns)
    z = torch.linspace(v_min, v_max, N, device=ns.device)
    delta = (v_max - v_min) / (N - 1)
    a = (torch.softmax(lg_sel, -1) * z).sum(-1).masked_fill(~mask, float("-inf")).argmax(1)
    boot = mask.any(1) & ~d
    p = torch.softmax(lg_eval[torch.arange(rows, device=ns.device), a], -1)
    tz = (r[:, None] + gamma * boot[:, None] * z[None, :]).clamp(v_min, v_max)
    b = (tz - v_min) / delta
    lo, hi = b.floor().long(), b.ceil().long()
    lo[(hi > 0) & (lo == hi)] -= 1
    hi[(lo < N - 1) & (lo == hi)] += 1
    m = torch.zeros(rows, N, device=ns.device)
    m.scatter_add_(1, lo, p * (hi.float() - b))
    m.scatter_add_(1, hi, p * (b - lo.float()))
    return m, torch.where(boot, a, -1)


res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "age_turns": args.age, "atoms": args.atoms,
       "v_min": args.v_min, "v_max": args.v_max, "shapes": []}
gen = torch.Generator(device="cuda")
gen.manual_seed(1)
for c in args.configs.split(","):
    b, wh, p = c.split(":")
    w, h = (int(v) for v in wh.split("x"))
    B, P, N = int(b), int(p), args.atoms
    ns, env_mask = game_in_progress(B, w, h, P)
    rows, A = B * P, 5 * w * h
    legal = int(env_mask.sum())
    row = {"config": c, "rows": rows, "actions": A, "legal_per_row": legal / rows, "legal_share": legal / (rows * A)}
    r = torch.randn(rows, device="cuda", generator=gen)
    d = torch.rand(rows, device="cuda", generator=gen) < 0.05
    q_eval, q_sel = (torch.randn(rows, A, device="cuda", generator=gen) for _ in range(2))
    obs_bytes, per_row = rows * 3 * w * h * 4, rows * (4 + 1 + 4 + 8)
    # ---- mask ----
    got = valid_actions_mask_from_observation(ns)
    row["mask_equals_env"] = bool(torch.equal(got, env_mask))
    row["mask_equals_torch"] = bool(torch.equal(got, torch_mask(ns)))
    out = torch.empty_like(got)
    e = {"hip_bytes": obs_bytes + rows * A, "hip_us": timed(lambda: valid_actions_mask_from_observation(ns, out=out), args.calls, args.repeats) * 1e6,
         "torch_us": timed(lambda: torch_mask(ns), args.calls, args.repeats) * 1e6}
    row["mask"] = e
    # ---- scalar Double DQN target ----
    t_hip, a_hip = double_q_target(ns, q_eval, r, args.gamma, d, q_select=q_sel)
    t_ref, a_ref = torch_q_target(ns, q_eval, q_sel, r, args.gamma, d)
    row["q_action_equal"], row["q_target_max_diff"] = bool(torch.equal(a_hip, a_ref)), float((t_hip - t_ref).abs().max())
    e = {"hip_bytes": obs_bytes + 2 * legal * 4 + per_row, "torch_bytes": obs_bytes + 2 * rows * A * 4,
         "hip_us": timed(lambda: double_q_target(ns, q_eval, r, args.gamma, d, q_select=q_sel), args.calls, args.repeats) * 1e6,
         "torch_us": timed(lambda: torch_q_target(ns, q_eval, q_sel, r, args.gamma, d), args.calls, args.repeats) * 1e6}
    row["q_target"] = e
    del q_eval, q_sel
    # ---- categorical ----
    lg_eval, lg_sel = (2 * torch.randn(rows, A, N, device="cuda", generator=gen) for _ in range(2))
    m_hip, a_hip = categorical_target(ns, lg_eval, r, args.gamma, d, args.v_min, args.v_max, logits_select=lg_sel)
    m_ref, a_ref = torch_categorical(ns, lg_eval, lg_sel, r, args.gamma, d, args.v_min, args.v_max)
    same = a_hip == a_ref
    row["categorical_action_equal_share"] = float(same.float().mean())
    row["categorical_m_max_diff"] = float((m_hip - m_ref)[same].abs().max())
    e = {"hip_bytes": obs_bytes + legal * N * 4 + 2 * rows * N * 4 + per_row, "torch_bytes": obs_bytes + rows * A * N * 4 + 2 * rows * N * 4,
         "logits_bytes_each": rows * A * N * 4,
         "hip_us": timed(lambda: categorical_target(ns, lg_eval, r, args.gamma, d, args.v_min, args.v_max, logits_select=lg_sel), args.calls,
                         args.repeats) * 1e6,
         "torch_us": timed(lambda: torch_categorical(ns, lg_eval, lg_sel, r, args.gamma, d, args.v_min, args.v_max), args.calls,
                           args.repeats) * 1e6}
    row["categorical"] = e
    del lg_eval, lg_sel, m_ref
    for k in ("mask", "q_target", "categorical"):
        e = row[k]
        e["torch_over_hip"] = e["torch_us"] / e["hip_us"]
        e["hip_gbs"] = e["hip_bytes"] / (e["hip_us"] * 1e-6) / 1e9
    res["shapes"].append(row)
    torch.cuda.empty_cache()
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
