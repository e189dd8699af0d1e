#!/usr/bin/env python3
"""gvec_gym_step and gvec_gym_step_players of two builds of the library in one process, alternating, against the noise of
the comparison itself: BASE is loaded twice (from two files, BASE_COPY being a copy of BASE - one path loads once), and the
gap between the two loads of one build is the noise band the other build is judged by.
  gym_step     one learner, scripts/bench_gym_sizes.py's sizes at 65,536 envs
  players      every player a learner, scripts/bench_selfplay.py's 65,536-env configs
Per size: median of --repeats timings of --steps steps per library, `band` = |BASE - BASE_COPY|, `inside` = NEW lies within
BASE +- band.  Prints one JSON line.
usage: scripts/ab_gym_libs.py BASE.so BASE_COPY.so NEW.so [--steps K] [--repeats R] [--envs B]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from generalsreinforcementlearning_amd import _lib
from generalsreinforcementlearning_amd._lib import check
from generalsreinforcementlearning_amd.vec_engine import VecEngine

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--envs", type=int, default=65536)
args = ap.parse_args()
NAMES = ("base", "base_copy", "new")
LIBS = [_lib.load_from(os.path.abspath(p)) for p in args.libs]
GYM_STEP = ((15, 15, 2), (16, 16, 2), (10, 10, 2), (20, 20, 4), (20, 20, 2), (25, 25, 4), (32, 32, 8))
PLAYERS = ((15, 15, 2), (20, 20, 4))


def run(B, w, h, P, players):
    dev = torch.device("cuda")
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    L, max_turns = (P if players else 1), 10 ** 6
    bits = (1 << P) - 1
    engines = []
    for lib in LIBS:
        e = VecEngine(B, w, h, P, auto_reset=True, lib=lib, stream=torch.cuda.current_stream().cuda_stream)
        e.reset_generated(1)
        e.build_board_pool(1024, 2)
        engines.append(e)
    stride = engines[0].stride
    # the libraries share their output buffers; each engine keeps its own state and turn count
    obs, mask = z((B, L, 9, stride), torch.float32), z((B, L, stride * 5), torch.uint8)
    rew, inv, err, alive, played = (z((B, L), torch.float64), z((B, L), torch.uint8), z((B, L), torch.uint8), z((B, L), torch.uint8),
                                    z(B, torch.uint8))
    term, trunc, nr, win, tout, zeros8 = z(B, torch.uint8), z(B, torch.uint8), z(B, torch.uint8), z(B, torch.int8), z(B, torch.int64), z(B, torch.uint8)
    turns = [z(B, torch.int64) for _ in engines]
    e = engines[0]
    if players:
        check(e.L.gvec_gym_observe_players(e.h, bits, turns[0].data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(), rew.data_ptr(), None, None))
    else:
        check(e.L.gvec_gym_observe(e.h, 0, turns[0].data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(), None, None, None))
    # fixed actions: each learner's first valid index at the start (most stay valid for a while, the rest are refused)
    acts = torch.argmax(mask, dim=2).contiguous()
    seed = [0]

    def step(i):
        e, turn = engines[i], turns[i]
        seed[0] += 1
        if players:
            check(e.L.gvec_gym_step_players(e.h, bits, seed[0], acts.data_ptr(), zeros8.data_ptr(), turn.data_ptr(), max_turns, obs.data_ptr(),
                                            mask.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), win.data_ptr(), nr.data_ptr(),
                                            tout.data_ptr(), inv.data_ptr(), err.data_ptr(), alive.data_ptr()))
        else:
            check(e.L.gvec_gym_step(e.h, 0, seed[0], acts.data_ptr(), zeros8.data_ptr(), turn.data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(),
                                    rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), win.data_ptr(), nr.data_ptr(), tout.data_ptr(),
                                    played.data_ptr(), inv.data_ptr(), err.data_ptr()))

    for i in range(len(engines)):
        for _ in range(10):
            step(i)
    torch.cuda.synchronize()
    times = [[] for _ in engines]
    for _ in range(args.repeats):
        for i in range(len(engines)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(i)
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / args.steps)
    med = [statistics.median(t) for t in times]
    band = abs(med[0] - med[1])
    row = {"call": "gvec_gym_step_players" if players else "gvec_gym_step", "envs": B, "board": f"{w}x{h}", "players": P, "learners": L}
    for n, m, t in zip(NAMES, med, times):
        row[n + "_ms"] = round(m, 4)
        row[n + "_ms_all"] = [round(x, 4) for x in t]
    row["band_ms"] = round(band, 4)
    row["new_minus_base_pct"] = round(100.0 * (med[2] - med[0]) / med[0], 2)
    row["inside"] = bool(abs(med[2] - med[0]) <= band)
    for e in engines:
        e.close()
    return row


rows = []
for (w, h, p) in GYM_STEP:
    rows.append(run(args.envs, w, h, p, False))
    torch.cuda.empty_cache()
for (w, h, p) in PLAYERS:
    rows.append(run(args.envs, w, h, p, True))
    torch.cuda.empty_cache()
print(json.dumps({"bench": "ab_gym_libs", "steps": args.steps, "repeats": args.repeats, "rows": rows}))
