#!/usr/bin/env python3
"""Self-play step (gvec_gym_step_players, every player a learner) against what the existing calls offer, in one process,
alternating and repeated:
  players   gvec_gym_step_players: one launch, every learner's observation / mask / reward
  single    (a) gvec_gym_step for ONE learner (the opponents are the on-device agent)
  composed  (b) the cheapest composition of existing calls yielding every learner's observation: gvec_gym_actions per
            learner -> gvec_step -> gvec_gym_observe per learner (its rewards are wrong - every learner after the first is
            measured against stats the previous call refreshed - but it writes the same bytes)
Prints one JSON line: per configuration ms per step (median of the repeats), env-steps/s, learner-steps/s and the output
bytes by construction, L x (9*4 + 5) x tile_stride per env.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
usage: scripts/bench_selfplay.py [--steps K] [--repeats R] [--configs B:WxH:P,...]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import generalsreinforcementlearning_amd as g
from generalsreinforcementlearning_amd._lib import check

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--configs", default="4096:15x15:2,65536:15x15:2,4096:20x20:4,65536:20x20:4")
args = ap.parse_args()


def run(B, w, h, P):
    dev = torch.device("cuda")
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    n, L, max_turns = w * h, P, 10 ** 6
    bits = (1 << P) - 1
    e = g.VecEngine(B, w, h, P, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream)
    e.reset_generated(1)
    e.build_board_pool(1024, 2)
    stride = e.stride
    turn, zeros8 = z(B, torch.int64), z(B, torch.uint8)
    # players: [B][L] outputs
    obs, mask = z((B, L, 9, stride), torch.float32), z((B, L, stride * 5), torch.uint8)
    rew, inv, err, alive = z((B, L), torch.float64), z((B, L), torch.uint8), z((B, L), torch.uint8), z((B, L), torch.uint8)
    f8 = {k: z(B, torch.uint8) for k in ("term", "trunc", "nr")}
    win, tout = z(B, torch.int8), z(B, torch.int64)
    # (b): one [B] buffer set per learner; (a) uses learner 0's
    lobs, lmask = z((L, B, 9, stride), torch.float32), z((L, B, stride * 5), torch.uint8)
    lrew, lplayed, linv, lerr = z((L, B), torch.float64), z((L, B), torch.uint8), z((L, B), torch.uint8), z((L, B), torch.uint8)
    acts = z((B, P, 8), torch.uint8)
    check(e.L.gvec_gym_observe_players(e.h, bits, turn.data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(), rew.data_ptr(), None, None))
    for p in range(L):
        check(e.L.gvec_gym_observe(e.h, p, turn.data_ptr(), max_turns, lobs[p].data_ptr(), lmask[p].data_ptr(), None, None, None))
    # fixed actions: each learner's first valid index at the start (most stay valid for a while, the rest are refused)
    a_pl = torch.argmax(mask, dim=2).contiguous()                       # [B, L]
    a_l = [a_pl[:, p].contiguous() for p in range(L)]
    seed = [0]

    def players():
        seed[0] += 1
        check(e.L.gvec_gym_step_players(e.h, bits, seed[0], a_pl.data_ptr(), zeros8.data_ptr(), turn.data_ptr(), max_turns, obs.data_ptr(),
                                        mask.data_ptr(), rew.data_ptr(), f8["term"].data_ptr(), f8["trunc"].data_ptr(), win.data_ptr(),
                                        f8["nr"].data_ptr(), tout.data_ptr(), inv.data_ptr(), err.data_ptr(), alive.data_ptr()))

    def single():
        seed[0] += 1
        check(e.L.gvec_gym_step(e.h, 0, seed[0], a_l[0].data_ptr(), zeros8.data_ptr(), turn.data_ptr(), max_turns, lobs[0].data_ptr(),
                                lmask[0].data_ptr(), lrew[0].data_ptr(), f8["term"].data_ptr(), f8["trunc"].data_ptr(), win.data_ptr(),
                                f8["nr"].data_ptr(), tout.data_ptr(), lplayed[0].data_ptr(), linv[0].data_ptr(), lerr[0].data_ptr()))

    def composed():
        for p in range(L):
            check(e.L.gvec_gym_actions(e.h, p, a_l[p].data_ptr(), lmask[p].data_ptr(), zeros8.data_ptr(), acts.data_ptr(), lplayed[p].data_ptr(),
                                       linv[p].data_ptr(), lerr[p].data_ptr()))
        e.step_device(acts.data_ptr())
        for p in range(L):
            check(e.L.gvec_gym_observe(e.h, p, turn.data_ptr(), max_turns, lobs[p].data_ptr(), lmask[p].data_ptr(), lrew[p].data_ptr(), None, None))

    fns = {"players": players, "single": single, "composed": composed}
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out_b = L * (9 * 4 + 5) * stride
    row = {"envs": B, "board": f"{w}x{h}", "players": P, "learners": L, "out_bytes_per_env": out_b,
           "out_GB_per_step": B * out_b / 1e9}
    for k, ms in med.items():
        ln = L if k != "single" else 1
        row[k] = {"ms": round(ms, 4), "ms_all": [round(t, 4) for t in times[k]], "M_env_steps_s": round(B / ms / 1e3, 2),
                  "M_learner_steps_s": round(B * ln / ms / 1e3, 2),
                  "out_TBps": round(B * (ln * (9 * 4 + 5) * stride) / ms / 1e9, 3)}
    row["players_vs_composed"] = round(med["composed"] / med["players"], 3)
    e.close()
    return row


rows = []
for c in args.configs.split(","):
    b, wh, p = c.split(":")
    w, h = (int(x) for x in wh.split("x"))
    rows.append(run(int(b), w, h, int(p)))
    torch.cuda.empty_cache()
print(json.dumps({"bench": "selfplay", "steps": args.steps, "repeats": args.repeats, "rows": rows}))
