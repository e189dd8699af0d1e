#!/usr/bin/env python3
"""The match arena's episode tally (gvec_arena_update, arena_update_kernel) against a torch formulation of the same
definition, and an arena step against a bare env step, in one process:
  hip     EpisodeTally.update on the outputs of a GeneralsSelfPlayVecEnv step taken after `--age` turns of random legal play
  torch   the same definition as batched torch ops on the same inputs and the same kind of state (torch_update below).  Without
          a host sync torch cannot branch on "some env was truncated", so with an observation it counts the land of every column
          on every step; `torch_noobs` is the same without an observation (survivors tie), the bookkeeping alone
Each on an ordinary step (the env's own flags after --age turns) and on a step on which every env is truncated (the same
tensors with truncated set everywhere: the step on which the kernel reads plane 1 of every surviving column).
Both formulations are run over a sequence of such steps (ordinary, truncated, re-dealt, terminated, capped) from zero state and
every state tensor is compared bit for bit before anything is timed.
Times: `wall_us` is wall-clock per call with every call enqueued from Python and one synchronisation per repeat (what a loop
pays when the host is the bottleneck); `graph_us` is per call of a captured graph of --graph-calls calls replayed (the
device's time with no host in the way).  Median of --repeats, the variants alternating inside every repeat.
  arena   ms per step of: `bare` one random policy on all rows (MaskedCategoricalHead.sample on zero logits) + env.step;
          `arena_1` Arena with that one entrant (bare + the tally's launch); `arena_2` Arena with two such entrants (an
          index_select pair and a scatter per entrant on top).  Ordinary steps (max_turns far away).
usage: scripts/bench_arena.py [--calls K] [--repeats R] [--age T] [--configs envs:WxH:players,...] [--out profiles/arena_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--graph-calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--age", type=int, default=60)
ap.add_argument("--arena-steps", type=int, default=100)
ap.add_argument("--configs", default="4096:15x15:4,16384:20x20:2", help="envs:WxH:players")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402

from generalsreinforcementlearning_amd.arena import Arena, EpisodeTally, random_policy  # noqa: E402
from generalsreinforcementlearning_amd.policy_head import MaskedCategoricalHead  # noqa: E402
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv  # noqa: E402

NAMES = ("death", "ep_len", "ep_return", "games", "wins", "eliminated", "len_sum", "ret_sum", "pair2")


def zero_state(B, L):
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    return {"death": z((B, L), torch.int32), "ep_len": z(B, torch.int32), "ep_return": z((B, L), torch.float64), "games": z(B, torch.int32),
            "wins": z((B, L), torch.int32), "eliminated": z((B, L), torch.int32), "len_sum": z(B, torch.int64),
            "ret_sum": z((B, L), torch.float64), "pair2": z((B, L, L), torch.int32)}


def torch_update(s, ids, cap, alive, terminated, truncated, winner, reward, reset, obs):
    """include/generals_vec.h "match arena" as batched torch ops, state updated in place; nothing synchronises"""
    L = alive.shape[1]
    live = ~reset
    ep_len = torch.where(live, s["ep_len"] + 1, 0)
    ret = s["ep_return"] + reward
    death = torch.where((s["death"] == 0) & ~alive, ep_len[:, None], s["death"])
    end = live & (terminated | truncated)
    counted = end & ~(s["games"] == cap) if cap > 0 else end
    key = torch.where(death != 0, death, 1 << 20)
    if obs is not None:
        land = (obs[:, :, 1] == 0.5).flatten(2).sum(-1, dtype=torch.int32)
        key = key + torch.where((death == 0) & (truncated & ~terminated)[:, None], land, 0)
    ki, kj = key[:, :, None], key[:, None, :]
    points = ((ki > kj).to(torch.int32) * 2 + (ki == kj).to(torch.int32)) * ~torch.eye(L, dtype=torch.bool, device=key.device)
    c1, c2 = counted[:, None], counted[:, None, None]
    s["pair2"] += points * c2
    s["games"] += counted
    s["len_sum"] += ep_len * counted
    s["wins"] += (winner[:, None] == ids[None, :]) & c1
    s["eliminated"] += (death != 0) & c1
    s["ret_sum"].copy_(torch.where(c1, s["ret_sum"] + ret, s["ret_sum"]))
    keep = (live & ~end)
    s["death"].copy_(torch.where(keep[:, None], death, 0))
    s["ep_return"].copy_(torch.where(keep[:, None], ret, 0.0))
    s["ep_len"].copy_(torch.where(keep, ep_len, 0))


def alternating(fns, calls, repeats):
    """{name: median seconds per call}: wall-clock, every call enqueued, one synchronisation per repeat and variant"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            runs[k].append((time.perf_counter() - t0) / calls)
    return {k: sorted(v)[len(v) // 2] for k, v in runs.items()}, {k: [round(x * 1e6, 3) for x in v] for k, v in runs.items()}


def graphed(fn, n):
    """fn called n times, captured once: replaying it is the device's time for n calls"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(n):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return g.replay


def step_outputs(B, w, h, P):
    """what a step returned after --age turns of random legal play, cloned: (alive, terminated, truncated, winner, reward, reset, obs)"""
    env = GeneralsSelfPlayVecEnv(B, w, h, max_players=P, max_turns=100000, device_outputs=True, seed=5)
    head = MaskedCategoricalHead()
    obs, info = env.reset()
    zeros = torch.zeros(B, P, 5 * w * h, device="cuda")
    for k in range(args.age):
        actions = head.sample(zeros, info["valid_actions_mask"], seed=k + 1)[0]
        obs, reward, terminated, truncated, info = env.step(actions)
    out = (info["alive"].clone(), terminated.clone(), truncated.clone(), info["winner"].clone(), reward.clone(), info["reset"].clone(), obs.clone())
    ids = list(env.player_ids)
    env.close()
    return out, ids


res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "graph_calls": args.graph_calls, "repeats": args.repeats,
       "age_turns": args.age, "shapes": []}
for c in args.configs.split(","):
    b, wh, p = c.split(":")
    w, h = (int(v) for v in wh.split("x"))
    B, L = int(b), int(p)
    (alive, term, trunc, winner, reward, reset, obs), ids = step_outputs(B, w, h, L)
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    all_trunc, none = torch.ones_like(trunc), torch.zeros_like(trunc)
    ordinary = (alive, term, trunc, winner, reward, reset, obs)
    truncation = (alive, none, all_trunc, winner, reward, none, obs)
    row = {"config": c, "envs": B, "learners": L, "board": wh, "alive_share": float(alive.float().mean()),
           "flags_set": {"terminated": int(term.sum()), "truncated": int(trunc.sum()), "reset": int(reset.sum())},
           "truncation_step_plane_bytes": int((alive & ~none[:, None]).sum()) * w * h * 4}

    # ---- equal before anything is timed: a sequence that meets every branch, with and without observation, capped and not ----
    some = torch.arange(B, device="cuda") % 3 == 0
    won = torch.where(some, torch.tensor(ids[0], dtype=torch.int8, device="cuda"), winner)
    first_dead = alive.clone()
    first_dead[:, 0] &= ~some
    seq = [ordinary, ordinary, truncation, (alive, none, none, winner, reward, all_trunc, obs), ordinary, (first_dead, none, none, winner, reward, none, obs),
           (first_dead, some, all_trunc, won, reward, none, obs), (alive, none, none, winner, reward, some, obs), truncation, ordinary, truncation]
    equal = {}
    for with_obs in (True, False):
        for cap in (0, 2):
            tally, s = EpisodeTally(B, L, ids, games_cap=cap), zero_state(B, L)
            ok = True
            for a_, te, tr, wi, re_, rs, ob_ in seq:
                o = ob_ if with_obs else None
                tally.update(a_, te, tr, wi, re_, reset=rs, obs=o)
                torch_update(s, ids_t, cap, a_, te, tr, wi, re_, rs, o)
                ok = ok and all(torch.equal(tally.state[n], s[n]) for n in NAMES)
            equal[f"obs={with_obs},cap={cap}"] = bool(ok)
            if with_obs and cap == 0:
                row["games_counted_in_check"] = int(tally.games.sum())
    row["equal_to_torch"] = equal
    assert all(equal.values()), equal

    # ---- tally.update against the torch formulation ----
    for kind, inputs in (("ordinary", ordinary), ("truncation", truncation)):
        a_, te, tr, wi, re_, rs, ob_ = inputs
        tally, tally_n = EpisodeTally(B, L, ids), EpisodeTally(B, L, ids)
        s, s_n = zero_state(B, L), zero_state(B, L)
        fns = {"hip": lambda: tally.update(a_, te, tr, wi, re_, reset=rs, obs=ob_),
               "hip_noobs": lambda: tally_n.update(a_, te, tr, wi, re_, reset=rs),
               "torch": lambda: torch_update(s, ids_t, 0, a_, te, tr, wi, re_, rs, ob_),
               "torch_noobs": lambda: torch_update(s_n, ids_t, 0, a_, te, tr, wi, re_, rs, None)}
        wall, wall_all = alternating(fns, args.calls, args.repeats)
        replays = {k: graphed(f, args.graph_calls) for k, f in fns.items()}
        graph, graph_all = alternating(replays, 20, args.repeats)
        row[kind] = {k: {"wall_us": round(wall[k] * 1e6, 3), "graph_us": round(graph[k] * 1e6 / args.graph_calls, 3), "wall_us_all": wall_all[k],
                         "graph_us_all": [round(x / args.graph_calls, 3) for x in graph_all[k]]} for k in fns}
        row[kind]["torch_over_hip_wall"] = round(wall["torch"] / wall["hip"], 2)
        row[kind]["torch_over_hip_graph"] = round(graph["torch"] / graph["hip"], 2)
        row[kind]["torch_noobs_over_hip_noobs_graph"] = round(graph["torch_noobs"] / graph["hip_noobs"], 2)

    # ---- an arena step against a bare env step with the same policy ----
    def bare():
        env = GeneralsSelfPlayVecEnv(B, w, h, max_players=L, max_turns=100000, device_outputs=True, seed=5)
        policy = random_policy(seed=1)
        state = {"obs": None, "mask": None}
        state["obs"], info = env.reset()
        state["mask"] = info["valid_actions_mask"]

        def step():
            actions = policy(state["obs"].view(B * L, 9, h, w), state["mask"].view(B * L, 5 * w * h))
            out = env.step(actions.view(B, L))
            state["obs"], state["mask"] = out[0], out[4]["valid_actions_mask"]
        return step

    def arena(n):
        env = GeneralsSelfPlayVecEnv(B, w, h, max_players=L, max_turns=100000, device_outputs=True, seed=5)
        a = Arena(env, [random_policy(seed=k + 1) for k in range(n)])
        a.reset()
        return a.step

    fns = {"bare": bare(), "arena_1": arena(1), "arena_2": arena(2)}
    for f in fns.values():
        for _ in range(args.age):
            f()
    t, t_all = alternating(fns, args.arena_steps, args.repeats)
    row["arena_step"] = {k: {"ms": round(t[k] * 1e3, 5), "ms_all": [round(x / 1e3, 5) for x in t_all[k]]} for k in fns}
    row["arena_step"]["tally_share_of_arena_1"] = round((t["arena_1"] - t["bare"]) / t["arena_1"], 4)
    res["shapes"].append(row)
    print(json.dumps(row), flush=True)

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
