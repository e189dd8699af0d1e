#!/usr/bin/env python3
"""The playout search (gvec_search_playouts, search_kernel) against the composition of calls that gives the same terms without
it, in one process, and its playing strength.

  search       PlayoutSearch.evaluate + scores: one launch that writes 32 bytes per playout, then the reductions to q [n, K]
  composition  what a caller could do before the kernel existed, on a scratch engine of n * K * R envs without a board pool:
               copy_envs of every root K * R times (a gather / scatter launch and the stream sync of its range check), the
               agent's moves for turn 0 into device memory with the seat's slot overwritten by the decoded candidate (torch
               index arithmetic), one step, rollout(depth - 1, fused), gvec_read_state on the device, the terms from it and
               the same reductions
Roots: the envs of a self-play env after --age turns of uniform random legal play; root i is searched for seat i % P; the
candidates are a uniform draw of K of the seat's legal full moves (PlayoutSearch.propose on the mask without its half-move
column, so that every candidate is accepted and both paths play every row).  Before anything is timed the two paths' terms are
compared: they must be equal.
Times: `device_us` per call from device events around --calls calls (for the composition this includes the time the device
waits for the host across copy_envs' synchronisation: it is what the composition costs); `wall_us` a host clock around the
same calls ending in a synchronise.  Median of --repeats, the two paths alternating inside every repeat.
Rates: playout env-steps/s = turns actually played (the sum of the `turns` term) over the search's device time, beside the
fused rollout's env-steps/s on the scratch engine (n * K * R envs, `depth` turns, the same kernel variant).
  --strength   Arena: playout_policy (uniform prior, --playouts K:R:D) against random_policy on a two-player self-play env; and
               the same searcher as the learner of a GeneralsVecEnv whose other seat is the scripted bot.  Fixed seeds.
  --rollout bot   the search whose playouts play the scripted opponent's rule on every seat (gvec_search_playouts_bot,
               search_bot_kernel) against ITS composition: copy_envs, then per playout turn the agent's moves, gvec_bot_actions
               over them (both into device memory), the candidate on turn 0, one step; and beside both the agent-playout search
               of the same shape (`agent_search`), for the price of a playout turn.  With --strength every match is played once
               with each rollout, in the same run.  Write it to profiles/search_bot_bench.json.
usage: scripts/bench_search.py [--configs roots:K:R:D:WxH:players,...] [--calls N] [--repeats R] [--rollout agent|bot] [--strength]
                               [--out profiles/search_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="4096:16:4:8:15x15:2,1024:8:4:16:20x20:4", help="roots:K:R:D:WxH:players")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--age", type=int, default=60)
ap.add_argument("--strength", action="store_true")
ap.add_argument("--rollout", choices=("agent", "bot"), default="agent")
ap.add_argument("--playouts", default="8:4:8")
ap.add_argument("--strength-envs", type=int, default=1024)
ap.add_argument("--strength-episodes", type=int, default=2)
ap.add_argument("--strength-board", type=int, default=15)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from generalsreinforcementlearning_amd import VecEngine  # noqa: E402
from generalsreinforcementlearning_amd._lib import StateView  # noqa: E402
from generalsreinforcementlearning_amd.arena import Arena, random_policy  # noqa: E402
from generalsreinforcementlearning_amd.search import PlayoutSearch, T_TURNS, T_VALID, T_WON, playout_policy  # noqa: E402
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv  # noqa: E402
from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_search.py measures on the GPU: no device here")
DEV = torch.device("cuda", 0)
MEM_DEVICE = 1


def aged_roots(n, W, H, P, age, seed=7):
    """a self-play env of n boards after `age` turns of uniform random legal play -> (env, mask bool [n, P, 5 * H * W])"""
    env = GeneralsSelfPlayVecEnv(n, board_width=W, board_height=H, max_players=P, device_outputs=True, seed=seed, max_turns=10 ** 6)
    policy = random_policy(seed=3)
    _, info = env.reset()
    mask = info["valid_actions_mask"]
    for _ in range(age):
        a = policy(None, mask.view(n * P, -1)).view(n, P)
        _, _, _, _, info = env.step(a)
        mask = info["valid_actions_mask"]
    return env, mask.clone()


class Composition:
    """the same terms from copy_envs + step + fused rollout + read_state + torch, every buffer allocated once"""

    def __init__(self, engine, n, K, R, D, W, H, P, players, bot_players=0):
        self.src, self.n, self.K, self.R, self.D, self.W, self.P = engine, n, K, R, D, W, P
        self.bot_players = bot_players                           # not 0: every turn is agent_actions + bot_actions + step
        self.V = V = n * K * R
        self.scratch = VecEngine(V, W, H, P)
        self.scratch.set_stream(torch.cuda.current_stream(DEV).cuda_stream)
        v = torch.arange(V, device=DEV)
        self.root = (v // (K * R)).to(torch.int32)
        self.cand_of = v // R                                    # index into candidates.view(-1)
        self.seat = players.to(torch.int64)[v // (K * R)]
        self.rows = v
        self.acts = torch.zeros((V, P, 8), dtype=torch.uint8, device=DEV)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
        self.state = {"turn": z(V, torch.int32), "done": z(V, torch.uint8), "winner": z(V, torch.int8), "alive": z((V, P), torch.uint8),
                      "army_count": z((V, P), torch.int32), "tile_count": z((V, P), torch.int32)}
        self.view = StateView()
        for k, t in self.state.items():
            setattr(self.view, k, t.data_ptr())
        self.turn0 = None

    def terms(self, candidates, seed):
        s, L = self.scratch, self.scratch.L
        s.copy_envs(src_ids=self.root, src=self.src)
        if self.turn0 is None:                                   # the roots do not change between calls
            assert L.gvec_read_state(s.h, 0, self.V, C.byref(self.view), MEM_DEVICE) == 0
            self.turn0 = self.state["turn"].clone()
        assert L.gvec_agent_actions(s.h, seed, 0, self.acts.data_ptr(), MEM_DEVICE) == 0
        a = candidates.reshape(-1)[self.cand_of]
        frm, d = a // 5, a % 5
        fx, fy = frm % self.W, frm // self.W
        dx = (d == 1).to(torch.int64) - (d == 3).to(torch.int64)
        dy = (d == 2).to(torch.int64) - (d == 0).to(torch.int64)
        move = torch.stack([fx, fy, fx + dx, fy + dy, torch.ones_like(a)] + [torch.zeros_like(a)] * 3, dim=1).to(torch.uint8)
        if self.bot_players:
            assert L.gvec_bot_actions(s.h, self.bot_players, seed, 0, self.acts.data_ptr(), MEM_DEVICE) == 0
        self.acts[self.rows, self.seat] = move                   # the candidate, whether the seat is on the rule or not
        s.step_device(self.acts)
        if self.bot_players:
            for _ in range(self.D - 1):
                assert L.gvec_agent_actions(s.h, seed, 0, self.acts.data_ptr(), MEM_DEVICE) == 0
                assert L.gvec_bot_actions(s.h, self.bot_players, seed, 0, self.acts.data_ptr(), MEM_DEVICE) == 0
                s.step_device(self.acts)
        elif self.D > 1:
            s.rollout(self.D - 1, seed, fused=True, want_stats=False)
        assert L.gvec_read_state(s.h, 0, self.V, C.byref(self.view), MEM_DEVICE) == 0
        st = self.state
        seat = self.seat[:, None]
        land, army = st["tile_count"].gather(1, seat)[:, 0], st["army_count"].gather(1, seat)[:, 0]
        t = torch.stack([torch.ones_like(land), st["turn"] - self.turn0, st["alive"].gather(1, seat)[:, 0].to(torch.int32),
                         ((st["done"] != 0) & (st["winner"].to(torch.int64) == self.seat)).to(torch.int32), land, army,
                         st["tile_count"].sum(1, dtype=torch.int32) - land, st["army_count"].sum(1, dtype=torch.int32) - army], dim=1)
        return t.view(self.n, self.K, self.R, 8)


def timed(fn, calls):
    """(device us per call from events, wall us per call) of `calls` calls of fn"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, (time.perf_counter() - t0) * 1e6 / calls


def bench_config(spec):
    n, K, R, D, wh, P = spec.split(":")
    n, K, R, D, P = int(n), int(K), int(R), int(D), int(P)
    W, H = (int(x) for x in wh.split("x"))
    env, mask = aged_roots(n, W, H, P, args.age)
    players = (torch.arange(n, device=DEV) % P).to(torch.int32)
    seat_mask = mask[torch.arange(n, device=DEV), players.to(torch.int64)].clone()
    seat_mask.view(n, -1, 5)[:, :, 4] = False                   # full moves only: every candidate is accepted
    bot = args.rollout == "bot"
    agent_search = PlayoutSearch(env, candidates=K, replicas=R, depth=D)
    search = PlayoutSearch(env, candidates=K, replicas=R, depth=D, rollout="bot") if bot else agent_search
    cand = search.propose(seat_mask, None, seed=1)
    padded = cand < 0
    # padding rows: the composition needs a move to decode - give both paths the seat's first candidate again (a duplicate)
    cand = torch.where(padded, cand[:, :1].expand_as(cand), cand).contiguous()
    playable = bool((cand >= 0).all())
    comp = Composition(env.engine, n, K, R, D, W, H, P, players, search.bot_players)
    seed = 11
    ours = search.evaluate(None, players, cand, seed)
    theirs = comp.terms(cand, seed)
    live = torch.from_numpy(env.engine.game_state(fields=("done",))["done"] == 0).to(DEV)   # a finished root: the kernel plays nothing
    rows_ok = ((cand >= 0) & live[:, None])[:, :, None].expand(n, K, R)
    equal = bool(torch.equal(ours[rows_ok], theirs[rows_ok]))
    q_ours, q_theirs = search.scores(ours)[0], search.scores(torch.where(rows_ok[..., None], theirs, torch.zeros_like(theirs)))[0]
    res = {"config": spec, "rollout": args.rollout, "roots": n, "candidates": K, "replicas": R, "depth": D, "board": [W, H], "players": P, "age": args.age,
           "playouts": n * K * R, "padded_candidates": int(padded.sum()), "all_candidates_playable": playable,
           "valid_rows": int((ours[..., T_VALID] == 1).sum()), "terms_equal": equal, "q_equal": bool(torch.equal(q_ours, q_theirs)),
           "won_rows": int(ours[..., T_WON].sum()), "turns_played": int(ours[..., T_TURNS].sum())}
    res["live_roots"] = int(live.sum())
    if not equal:
        bad = (ours != theirs).any(-1) & rows_ok
        i, k, j = (int(x) for x in bad.nonzero()[0])
        print(f"WARNING {spec}: the search and the composition disagree in {int(bad.sum())} rows; first ({i}, {k}, {j}): "
              f"{ours[i, k, j].tolist()} vs {theirs[i, k, j].tolist()}, candidate {int(cand[i, k])}", flush=True)

    def run_search():
        search.scores(search.evaluate(None, players, cand, seed))

    def run_comp():
        search.scores(comp.terms(cand, seed))

    def run_rollout():
        comp.scratch.rollout(D, seed, fused=True, want_stats=False)

    def run_agent_search():
        agent_search.scores(agent_search.evaluate(None, players, cand, seed))

    for f in (run_search, run_comp) + ((run_agent_search,) if bot else ()):
        for _ in range(3):
            f()
    comp.scratch.copy_envs(src_ids=comp.root, src=env.engine)
    run_rollout()
    samples = {"search": [], "composition": [], "rollout": []}
    if bot:
        samples["agent_search"] = []
        res["agent_turns_played"] = int(agent_search.evaluate(None, players, cand, seed)[..., T_TURNS].sum())
    for _ in range(args.repeats):
        samples["search"].append(timed(run_search, args.calls))
        samples["composition"].append(timed(run_comp, args.calls))
        if bot:
            samples["agent_search"].append(timed(run_agent_search, args.calls))
        comp.scratch.copy_envs(src_ids=comp.root, src=env.engine)          # the rollout starts from the roots every time
        samples["rollout"].append(timed(run_rollout, 1))
    med = lambda xs, k: float(np.median([x[k] for x in xs]))
    for name, xs in samples.items():
        res[name] = {"device_us": med(xs, 0), "wall_us": med(xs, 1), "device_us_all": [round(x[0], 1) for x in xs]}
    res["speedup_device"] = res["composition"]["device_us"] / res["search"]["device_us"]
    res["speedup_wall"] = res["composition"]["wall_us"] / res["search"]["wall_us"]
    res["playout_env_steps_per_s"] = res["turns_played"] / (res["search"]["device_us"] * 1e-6)
    res["rollout_env_steps_per_s"] = n * K * R * D / (res["rollout"]["device_us"] * 1e-6)   # an upper count: finished games freeze
    if bot:                                                      # the price of a playout turn: ns of device time per turn played
        res["ns_per_playout_turn"] = res["search"]["device_us"] * 1e3 / max(res["turns_played"], 1)
        res["agent_ns_per_playout_turn"] = res["agent_search"]["device_us"] * 1e3 / max(res["agent_turns_played"], 1)
        res["turn_cost_ratio"] = res["ns_per_playout_turn"] / res["agent_ns_per_playout_turn"]
    comp.scratch.close()
    env.close()
    return res


def strength(rollout="agent"):
    K, R, D = (int(x) for x in args.playouts.split(":"))
    B, board, eps = args.strength_envs, args.strength_board, args.strength_episodes
    out = {"playouts": [K, R, D], "rollout": rollout, "envs": B, "board": board, "episodes_per_env": eps}
    tag = "playouts" if rollout == "agent" else "playouts-bot"
    env = GeneralsSelfPlayVecEnv(B, board_width=board, board_height=board, max_players=2, device_outputs=True, seed=42, max_turns=500)
    arena = Arena(env, [playout_policy(PlayoutSearch(env, candidates=K, replicas=R, depth=D, rollout=rollout), seed=1), random_policy(seed=2)],
                  names=[f"{tag}-{K}:{R}:{D}", "random"])
    t0 = time.perf_counter()
    steps = arena.run(episodes_per_env=eps, poll_every=32, max_steps=500 * eps + 64)
    res = arena.results()
    out["vs_random"] = {"table": res.table(), "steps": steps, "seconds": time.perf_counter() - t0, "games": res.totals["games"],
                        "win_rate": res.entrants["win_rate"].tolist(), "ratings": res.ratings().tolist()}
    env.close()
    # the searcher as the learner (seat 0) of the single-learner env, the other seat the scripted bot
    for opponent in ("bot", "random"):
        env = GeneralsVecEnv(B, board_width=board, board_height=board, max_players=2, device_outputs=True, seed=42, max_turns=500,
                             opponent=opponent)
        search = PlayoutSearch(env, candidates=K, replicas=R, depth=D, rollout=rollout)
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
        env.close()
    return out


def main():
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "configs": []}
    for spec in args.configs.split(","):
        r = bench_config(spec)
        print(json.dumps({k: r[k] for k in ("config", "terms_equal", "speedup_device", "speedup_wall", "playout_env_steps_per_s",
                                             "rollout_env_steps_per_s")}), flush=True)
        print(json.dumps({k: r[k] for k in ("search", "composition", "rollout", "agent_search", "turn_cost_ratio") if k in r}), flush=True)
        out["configs"].append(r)
    if args.strength:
        out["strength"] = strength()
        runs = [out["strength"]]
        if args.rollout == "bot":                                # the same three matches with the other rollout, in the same run
            out["strength_bot"] = strength("bot")
            runs.append(out["strength_bot"])
        for r in runs:
            print(r["vs_random"]["table"], flush=True)
            print(json.dumps({"rollout": r["rollout"], **{k: v for k, v in r.items() if k.startswith("seat0")}}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
