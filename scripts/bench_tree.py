#!/usr/bin/env python3
"""The tree search below the root (TreeSearch, gvec_search_expand, gvec_tree_select, gvec_tree_backup) in
one process: what keeping a board per playout costs, what the two walks cost, what a whole decision costs against the one-ply
HalvingSearch with the same number of playouts, and how the searcher plays.

  expand    gvec_search_expand (one playout per pair, its board after the first turn kept in a second engine) against the plain
            playout launch of equal shape (gvec_search_playouts: 32 bytes out per playout) and against what a caller had before
            it for the same work: gvec_copy_envs of the parents into a staging engine the size of the frontier, gvec_agent_actions,
            gvec_step, gvec_copy_envs of the result into its place (the read-out) and gvec_rollout(depth - 1).  The comparator
            leaves out the launch that writes the candidate over the seat's slot, in its own favour.  The terms of the first two
            are compared before anything is timed.
  walks     gvec_tree_select and gvec_tree_backup on the tree a real search left behind: device microseconds per wave.
  decision  TreeSearch.search at 16 / 64 and 64 / 256 against HalvingSearch.search at the same playout count on the same roots,
            the tree search's expand launches alone (its share that is not playout kernels) and the wall-clock cost of a
            decision, which holds the one stream synchronisation per wave that gvec_copy_envs' range check costs.
  strength  (--strength) bench_halving.py's three matches, same seeds and settings, for TreeSearch with a uniform prior.
Times: device microseconds per call from an event pair around --calls calls, the median of --repeats repeats, the paths
alternating inside every repeat.  Measurements, not thresholds.
usage: scripts/bench_tree.py [--calls N] [--repeats R] [--strength] [--out profiles/tree_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="4096:15x15:2,1024:20x20:4", help="roots:WxH:players")
ap.add_argument("--searches", default="16:64,64:256", help="candidates:simulations of a decision")
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--age", type=int, default=60)
ap.add_argument("--strength", action="store_true")
ap.add_argument("--strength-searches", default="16:64,64:256")
ap.add_argument("--strength-depths", default="8,16")
ap.add_argument("--strength-envs", type=int, default=1024)
ap.add_argument("--strength-episodes", type=int, default=2)
ap.add_argument("--strength-board", type=int, default=15)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from generalsreinforcementlearning_amd._lib import check  # noqa: E402
from generalsreinforcementlearning_amd.arena import Arena, random_policy  # noqa: E402
from generalsreinforcementlearning_amd.search import HalvingSearch, TreeSearch, playout_policy, search_expand_device  # noqa: E402
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv  # noqa: E402
from generalsreinforcementlearning_amd.vec_engine import MEM_DEVICE, VecEngine  # noqa: E402
from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_tree.py measures on the GPU: no device here")
DEV = torch.device("cuda", 0)


def aged_roots(n, W, H, P, age, seed=7):
    """bench_halving.py's: a self-play env of n boards after `age` turns of uniform random legal play -> (env, mask)"""
    env = GeneralsSelfPlayVecEnv(n, board_width=W, board_height=H, max_players=P, device_outputs=True, seed=seed, max_turns=10 ** 6)
    policy = random_policy(seed=3)
    _, info = env.reset()
    mask = info["valid_actions_mask"]
    for _ in range(age):
        a = policy(None, mask.view(n * P, -1)).view(n, P)
        _, _, _, _, info = env.step(a)
        mask = info["valid_actions_mask"]
    return env, mask.clone()


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(paths, calls=None):
    for f in paths.values():
        for _ in range(2):
            f()
    samples = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, f in paths.items():
            samples[k].append(timed(f, calls or args.calls))
    return {k: {"device_us": float(np.median(v)), "device_us_all": [round(x, 1) for x in v]} for k, v in samples.items()}


def seat_rows(mask, n, P):
    players = (torch.arange(n, device=DEV) % P).to(torch.int32)
    return players, mask[torch.arange(n, device=DEV), players.to(torch.int64)].contiguous()


# ---- expand against its comparators ---------------------------------------------------------------------------------------------
def bench_expand(env, mask, n, P, K, depth):
    e = env.engine
    players, seat_mask = seat_rows(mask, n, P)
    cand, _ = HalvingSearch(env, candidates=K, budget=K, depth=depth).propose(seat_mask, None, seed=1)
    kw = dict(fog_of_war=e.fog_of_war, device=e.device, production=e.production, normal_growth_interval=e.normal_growth_interval)
    dst = VecEngine(n * K, e.max_w, e.max_h, e.max_p, **kw)
    staging = VecEngine(n * K, e.max_w, e.max_h, e.max_p, **kw)
    terms = [torch.empty((n, K, 1, 8), dtype=torch.int32, device=DEV) for _ in range(2)]
    status = torch.empty((n, K), dtype=torch.int32, device=DEV)
    src = torch.arange(n, dtype=torch.int32, device=DEV).repeat_interleave(K).contiguous()
    ids = torch.arange(n * K, dtype=torch.int32, device=DEV)
    acts = torch.zeros((n * K, e.max_p, 8), dtype=torch.uint8, device=DEV)

    def expand():
        search_expand_device(e, n, cand.data_ptr(), players.data_ptr(), terms[0].data_ptr(), K, 1, depth, 11, dst=dst,
                             status_ptr=status.data_ptr())

    def playouts():
        e.search_playouts_device(n, cand.data_ptr(), players.data_ptr(), terms[1].data_ptr(), K, 1, depth, 11)

    def composition():
        staging.copy_envs(ids, src, n=n * K, src=e)
        check(staging.L.gvec_agent_actions(staging.h, 11, 0, C.c_void_p(acts.data_ptr()), MEM_DEVICE), "gvec_agent_actions")
        staging.step_device(acts.data_ptr())
        dst.copy_envs(ids, ids, n=n * K, src=staging)
        staging.rollout(depth - 1, 11, want_stats=False)

    expand()
    playouts()
    torch.cuda.synchronize()
    node_bytes = e.state_bytes_per_env()
    res = {"rows": n, "candidates": K, "depth": depth, "terms_equal": bool(torch.equal(terms[0], terms[1])),
           "boards_stored": int((status & 1).sum()), "bytes_per_stored_board": int(node_bytes)}
    res.update(alternate({"expand": expand, "playouts": playouts, "composition": composition}))
    res["expand_over_playouts"] = res["expand"]["device_us"] / res["playouts"]["device_us"]
    res["composition_over_expand"] = res["composition"]["device_us"] / res["expand"]["device_us"]
    res["us_per_stored_board"] = (res["expand"]["device_us"] - res["playouts"]["device_us"]) / max(1, res["boards_stored"])
    dst.close()
    staging.close()
    return res


# ---- a whole decision, and the walks on the tree it leaves ------------------------------------------------------------------------
def bench_decision(env, mask, n, P, m, sims, depth):
    players, seat_mask = seat_rows(mask, n, P)
    ts = TreeSearch(env, candidates=m, simulations=sims, depth=depth)
    hs = HalvingSearch(env, candidates=m, budget=sims, depth=depth)
    cand0, prior = ts.propose(seat_mask, None, seed=1)

    def tree():
        return ts.search(None, players, cand0, prior, 11)

    def halving():
        return hs.search(None, players, cand0, prior, 11)

    a, b = tree(), tree()
    info, T = a, a["tree"]
    res = {"rows": n, "candidates": m, "simulations": sims, "depth": depth, "schedule": ts.schedule, "waves": ts.waves, "nodes": ts.nodes,
           "simulations_per_row": ts.simulations_per_row, "halving_playouts_per_row": hs.playouts_per_row,
           "repeatable": all(bool(torch.equal(a[k], b[k])) for k in ("sum", "count", "slot", "action", "nodes_used")),
           "rows_with_a_survivor": int(info["found"].sum()), "mean_nodes_used": float(info["nodes_used"].double().mean()),
           "mean_deepest_visited_edge_count": float(T["child_count"][1:].amax(dim=(0, 2)).double().mean()),
           "tree_engine_bytes": int(n * ts.nodes * env.engine.state_bytes_per_env())}
    # the walks: a wave of the last round's shape on the finished tree
    K = ts.schedule[-1][0]
    slot = torch.arange(K, dtype=torch.int32, device=DEV).repeat(n, 1).contiguous()
    full = torch.arange(m, dtype=torch.int32, device=DEV).repeat(n, 1).contiguous()
    leaf = ts.select(T, full)
    terms = torch.zeros((n, m, ts.R, 8), dtype=torch.int32, device=DEV)
    status = torch.zeros((n, m), dtype=torch.int32, device=DEV)
    dead = torch.full((n, m), -1, dtype=torch.int32, device=DEV)            # leaf_slot -1 at the root on every column: the kernel
    at_root = torch.zeros((n, m), dtype=torch.int32, device=DEV)            # reads its arguments and writes nothing (T stays as it is)
    new_node = torch.ones((n, m), dtype=torch.int32, device=DEV)
    # a real wave's backup, on a copy of the tree (it grows the copy's sums; T is what the other timings read): every column
    # one valid playout, its board stored, the new node the tree's last id
    T2 = {k_: v.clone() for k_, v in T.items()}
    played = torch.zeros((n, m, ts.R, 8), dtype=torch.int32, device=DEV)
    played[..., 0], played[..., 2], played[..., 4:] = 1, 1, 7
    stored = torch.ones((n, m), dtype=torch.int32, device=DEV)
    last = torch.full((n, m), ts.nodes - 1, dtype=torch.int32, device=DEV)
    walks = alternate({"select_last_round": lambda: ts.select(T, slot), "select_all_slots": lambda: ts.select(T, full),
                       "backup_all_slots": lambda: ts.backup(T2, leaf[0], leaf[1], last, played, stored),
                       "backup_idle": lambda: ts.backup(T, at_root, dead, new_node, terms, status)}, calls=20)
    res["walks"] = walks
    # expand launches alone: every wave's launch with the leaves of the finished tree (the playouts it plays are as deep)
    players_rep = players

    def expands_only():
        for Kr, Rr in ts.schedule:
            s_ = full[:, :Kr].contiguous()
            ln, _, la, _ = ts.select(T, s_)
            for w in range(Rr):
                ts.expand(n, players_rep, ln, la, ts.round_seed(11, w))

    res.update(alternate({"tree_search": tree, "halving_search": halving, "tree_expands_and_selects_only": expands_only}, calls=2))
    res["share_not_playout_kernels"] = 1.0 - res["tree_expands_and_selects_only"]["device_us"] / res["tree_search"]["device_us"]
    res["tree_over_halving"] = res["tree_search"]["device_us"] / res["halving_search"]["device_us"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        tree()
    torch.cuda.synchronize()
    res["tree_search_wall_us"] = (time.perf_counter() - t0) / 3 * 1e6
    res["host_syncs_per_decision"] = ts.waves + 1
    ts.close()
    return res


# ---- strength (bench_halving.py's matches) --------------------------------------------------------------------------------------
def strength(make, name):
    B, board, eps = args.strength_envs, args.strength_board, args.strength_episodes
    out = {"searcher": name}
    env = GeneralsSelfPlayVecEnv(B, board_width=board, board_height=board, max_players=2, device_outputs=True, seed=42, max_turns=500)
    searcher = make(env)
    arena = Arena(env, [playout_policy(searcher, seed=1), random_policy(seed=2)], names=[name, "random"])
    t0 = time.perf_counter()
    steps = arena.run(episodes_per_env=eps, poll_every=32, max_steps=500 * eps + 64)
    res = arena.results()
    out["vs_random"] = {"steps": steps, "seconds": time.perf_counter() - t0, "games": res.totals["games"], "win_rate": res.entrants["win_rate"].tolist()}
    searcher.close()
    env.close()
    for opponent in ("bot", "random"):
        env = GeneralsVecEnv(B, board_width=board, board_height=board, max_players=2, device_outputs=True, seed=42, max_turns=500, opponent=opponent)
        search = make(env)
        _, info = env.reset()
        mask = info["valid_actions_mask"]
        games = torch.zeros(B, dtype=torch.int64, device=DEV)
        wins, losses, steps = torch.zeros_like(games), torch.zeros_like(games), 0
        t0 = time.perf_counter()
        while steps < 500 * eps + 64:
            actions, _ = search.act(mask.view(B, -1), seed=1000 + steps)
            _, _, terminated, truncated, info = env.step(actions)
            mask = info["valid_actions_mask"]
            count = (terminated | truncated) & (games < eps)
            wins += count & terminated & (info["winner"] == 0)
            losses += count & terminated & (info["winner"] != 0)
            games += count
            steps += 1
            if steps % 32 == 0 and int(games.min()) >= eps:
                break
        g, w, lo = int(games.sum()), int(wins.sum()), int(losses.sum())
        out[f"seat0_vs_{opponent}_seat"] = {"games": g, "wins": w, "losses": lo, "truncated": g - w - lo, "win_rate": w / max(g, 1), "steps": steps,
                                            "seconds": time.perf_counter() - t0}
        search.close()
        env.close()
    return out


def strength_table(out):
    for depth in (int(x) for x in args.strength_depths.split(",")):
        for rollout in ("agent", "bot"):
            for spec in args.strength_searches.split(","):
                m, sims = (int(x) for x in spec.split(":"))
                name = f"tree-{m}/{sims}-d{depth}-{rollout}"
                r = strength(lambda env: TreeSearch(env, candidates=m, simulations=sims, depth=depth, rollout=rollout), name)
                print(json.dumps({"searcher": name, "vs_random": r["vs_random"]["win_rate"], "vs_bot_seat": r["seat0_vs_bot_seat"]["win_rate"],
                                  "vs_random_seat": r["seat0_vs_random_seat"]["win_rate"],
                                  "seconds": [round(r[k]["seconds"], 1) for k in ("vs_random", "seat0_vs_bot_seat", "seat0_vs_random_seat")]}), flush=True)
                out["strength"].append(r)
                save(out)


def save(out):
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "age": args.age,
           "method": "one process; device time from an event pair around `calls` calls; the median of `repeats` repeats, the paths alternating "
                     "inside every repeat; outputs compared before timing",
           "expand": [], "decision": [], "strength": []}
    for spec in args.shapes.split(","):
        n, wh, P = spec.split(":")
        n, P = int(n), int(P)
        W, H = (int(x) for x in wh.split("x"))
        env, mask = aged_roots(n, W, H, P, args.age)
        for s in args.searches.split(","):
            m, sims = (int(x) for x in s.split(":"))
            r = dict(shape=spec, **bench_expand(env, mask, n, P, m, args.depth))
            print(json.dumps({"expand": {k: r[k] for k in ("shape", "candidates", "terms_equal", "boards_stored", "expand", "playouts", "composition",
                                                           "expand_over_playouts", "composition_over_expand")}}), flush=True)
            out["expand"].append(r)
            save(out)
            r = dict(shape=spec, **bench_decision(env, mask, n, P, m, sims, args.depth))
            print(json.dumps({"decision": {k: r[k] for k in ("shape", "candidates", "simulations", "waves", "repeatable", "tree_search", "halving_search",
                                                             "tree_expands_and_selects_only", "share_not_playout_kernels", "tree_over_halving",
                                                             "tree_search_wall_us", "walks")}}), flush=True)
            out["decision"].append(r)
            save(out)
        env.close()
    if args.strength:
        strength_table(out)
    save(out)


if __name__ == "__main__":
    main()
