#!/usr/bin/env python3
"""The sequential-halving search (HalvingSearch, gvec_search_halve, gvec_search_improved_policy) in one
process: what a round's tail and the policy target cost against the same definitions in torch, what a whole decision costs
against the flat search with the same number of playouts, and how the searchers play.

  tail      gvec_search_halve against the torch formulation a caller had before it: PlayoutScore on the terms, the masked sums
            over the replicas, scatter_add into the slots' sums and counts, the keys, topk, three gathers.  Terms: round 0 of a
            real search on aged roots (scripts/bench_search.py's), the columns behind a per-row permutation `slot`.
  policy    gvec_search_improved_policy against the same definition in torch float32, m = 16 visited candidates per row.
  decision  HalvingSearch.search (m = 16, budget 64, depth 8) against PlayoutSearch.evaluate + scores at 8 x 8 x depth 8 on the
            same roots - 64 playouts per row both - and the halving search's playout launches alone (its share that is not
            playout kernels).
  strength  (--strength) bench_search.py's three matches - Arena against random_policy, and seat 0 of a GeneralsVecEnv against
            the scripted bot and against the random opponent; 15x15, two players, fog on, 1,024 envs x 2 games, cut at 500 turns -
            for the flat 8 x 8 search and HalvingSearch m = 16 / budget 64 and m = 64 / budget 256, each with agent and bot
            rollouts at depth 8 and 16.  Fixed seeds; measurements, not thresholds.
Before anything is timed the two paths' outputs are compared.  Times: device microseconds per call from an event pair around
--calls calls, the median of --repeats repeats, the two paths alternating inside every repeat.
usage: scripts/bench_halving.py [--calls N] [--repeats R] [--strength] [--out profiles/halving_bench.json]"""
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
ap.add_argument("--tails", default="16:4,64:1", help="k:replicas of a round")
ap.add_argument("--policy-shapes", default="16384:2000,8192:1125", help="rows:actions")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--age", type=int, default=60)
ap.add_argument("--strength", action="store_true")
ap.add_argument("--strength-envs", type=int, default=1024)
ap.add_argument("--strength-episodes", type=int, default=2)
ap.add_argument("--strength-board", type=int, default=15)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from generalsreinforcementlearning_amd._lib import SEARCH_NONE, SearchHalveArgs, SearchPolicyArgs, check, load  # noqa: E402
from generalsreinforcementlearning_amd.arena import Arena, random_policy  # noqa: E402
from generalsreinforcementlearning_amd.search import HalvingSearch, PlayoutSearch, playout_policy  # noqa: E402
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv  # noqa: E402
from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_halving.py measures on the GPU: no device here")
DEV = torch.device("cuda", 0)
F64 = torch.float64


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


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


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(paths):
    """{name: fn} -> {name: {device_us, device_us_all}}: three warm-up calls each, then the paths in turn inside every repeat"""
    for f in paths.values():
        for _ in range(3):
            f()
    samples = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, f in paths.items():
            samples[k].append(timed(f, args.calls))
    return {k: {"device_us": float(np.median(v)), "device_us_all": [round(x, 1) for x in v]} for k, v in samples.items()}


# ---- a round's tail ---------------------------------------------------------------------------------------------------------
def torch_tail(score, terms, slot64, cand0, prior, total, count, k_next, q_lo, q_inv, c_visit, c_scale):
    ok = terms[..., 0] != 0
    s = torch.where(ok, score(terms), torch.zeros((), dtype=F64, device=DEV)).sum(-1)
    total.scatter_add_(1, slot64, s)
    count.scatter_add_(1, slot64, ok.sum(-1).to(torch.int32))
    nmax = count.max(dim=1, keepdim=True).values.to(F64)
    cs, cand = count.gather(1, slot64), cand0.gather(1, slot64)
    mean = total.gather(1, slot64) / cs.clamp(min=1).to(F64)
    key = prior.gather(1, slot64) + ((c_visit + nmax) * c_scale) * ((mean - q_lo) * q_inv)
    key = torch.where((cs > 0) & (cand != SEARCH_NONE), key, torch.full_like(key, -float("inf")))
    top = key.topk(k_next, dim=1).indices
    return slot64.gather(1, top).to(torch.int32), cand.gather(1, top)


def bench_tail(env, mask, n, P, k, R):
    players = (torch.arange(n, device=DEV) % P).to(torch.int32)
    seat_mask = mask[torch.arange(n, device=DEV), players.to(torch.int64)].contiguous()
    hs = HalvingSearch(env, candidates=k, budget=64, depth=8)
    cand0, prior = hs.propose(seat_mask, None, seed=1)
    slot = torch.argsort(torch.rand((n, k), device=DEV), dim=1).to(torch.int32).contiguous()       # a permutation per row
    slot64 = slot.to(torch.int64)
    terms = PlayoutSearch(env, candidates=k, replicas=R, depth=8).evaluate(None, players, cand0.gather(1, slot64).contiguous(), 11)
    k_next = (k + 1) // 2
    z = lambda dt: torch.zeros((n, k), dtype=dt, device=DEV)                                   # noqa: E731
    sums, counts = [z(F64), z(F64)], [z(torch.int32), z(torch.int32)]
    out_slot, out_cand = torch.empty((n, k_next), dtype=torch.int32, device=DEV), torch.empty((n, k_next), dtype=torch.int64, device=DEV)
    sc = hs.score
    a = SearchHalveArgs(n=n, m=k, k=k, replicas=R, k_next=k_next, reserved=0, terms=terms.data_ptr(), slot=slot.data_ptr(),
                        candidates0=cand0.data_ptr(), prior_key=prior.data_ptr(), win=sc.win, loss=sc.loss, land=sc.land, army=sc.army,
                        q_lo=hs.q_lo, q_inv_range=hs.q_inv_range, c_visit=hs.c_visit, c_scale=hs.c_scale, sum=sums[0].data_ptr(),
                        count=counts[0].data_ptr(), next_slot=out_slot.data_ptr(), next_candidates=out_cand.data_ptr())
    L = load()

    def kernel():
        check(L.gvec_search_halve(0, stream(), C.byref(a)), "gvec_search_halve")

    def formulation():
        return torch_tail(sc, terms, slot64, cand0, prior, sums[1], counts[1], k_next, hs.q_lo, hs.q_inv_range, hs.c_visit, hs.c_scale)

    kernel()
    t_slot, t_cand = formulation()
    same_rows = (out_slot.sort(dim=1).values == t_slot.sort(dim=1).values).all(dim=1)          # as sets: topk breaks ties its own way
    res = {"rows": n, "k": k, "replicas": R, "k_next": k_next, "valid_playouts": int((terms[..., 0] != 0).sum()),
           "counts_equal": bool(torch.equal(counts[0], counts[1])), "sums_max_abs_diff": float((sums[0] - sums[1]).abs().max()),
           "rows_with_equal_survivors": int(same_rows.sum())}
    res.update(alternate({"kernel": kernel, "torch": formulation}))
    res["speedup"] = res["torch"]["device_us"] / res["kernel"]["device_us"]
    return res


# ---- the policy target --------------------------------------------------------------------------------------------------------
def torch_policy(logits, legal, cand, total, count, value, q_lo, q_inv, c_visit, c_scale):
    n, A = legal.shape
    f32 = torch.float32
    ninf, zero = torch.full((), -float("inf"), dtype=f32, device=DEV), torch.zeros((), dtype=f32, device=DEV)
    x = torch.where(legal, logits, ninf)
    in_row = (count > 0) & (cand >= 0) & (cand < A)
    ai = torch.where(in_row, cand, torch.zeros_like(cand))
    xa = torch.where(in_row, x.gather(1, ai), ninf)
    vis = xa > ninf
    q = torch.where(vis, (total / count.clamp(min=1).to(F64)).to(f32), zero)
    vtop = xa.max(dim=1, keepdim=True).values
    w = torch.where(vis, torch.exp(xa - torch.where(torch.isinf(vtop), zero, vtop)), zero)
    den, num = w.sum(1), (w * q).sum(1)
    N = torch.where(vis, count, torch.zeros_like(count)).sum(1).to(f32)
    has = N > 0
    vq = num / torch.where(has, den, torch.ones_like(den))
    vmix = torch.where(has, (value + N * vq) / (1 + N), value)
    scale = ((c_visit + count.max(dim=1).values.to(F64)) * c_scale).to(f32)
    lo, inv = float(np.float32(q_lo)), float(np.float32(q_inv))
    shift = torch.where(has, scale * ((vmix - lo) * inv), zero)
    y = torch.cat([x + shift[:, None], torch.zeros((n, 1), dtype=f32, device=DEV)], dim=1)
    y.scatter_(1, torch.where(vis, ai, torch.full_like(ai, A)), xa + scale[:, None] * ((q - lo) * inv))
    y = y[:, :A]
    top = y.max(dim=1, keepdim=True).values
    e = torch.where(legal, torch.exp(y - torch.where(torch.isinf(top), zero, top)), zero)
    z = e.sum(1, keepdim=True)
    return e / torch.where(z > 0, z, torch.ones_like(z)), vmix


def bench_policy(n, A, m=16):
    g = torch.Generator(device=DEV).manual_seed(5)
    logits = torch.randn((n, A), device=DEV, generator=g) * 2
    legal = torch.rand((n, A), device=DEV, generator=g) < 0.15
    keys = torch.where(legal, torch.rand((n, A), device=DEV, generator=g), torch.full((), -1.0, device=DEV))
    top = keys.topk(m, dim=1)
    cand = torch.where(top.values < 0, torch.full_like(top.indices, SEARCH_NONE), top.indices).contiguous()
    count = torch.randint(0, 9, (n, m), device=DEV, generator=g, dtype=torch.int32)
    total = (torch.rand((n, m), device=DEV, generator=g, dtype=F64) * 2 - 1) * count
    value = torch.rand(n, device=DEV, generator=g) - 0.5
    mask8 = legal.to(torch.uint8)
    target, v_mix = torch.empty((n, A), device=DEV), torch.empty(n, device=DEV)
    q_lo, q_inv, c_visit, c_scale = -1.0, 0.5, 50.0, 1.0
    a = SearchPolicyArgs(n=n, num_actions=A, m=m, reserved=0, logits=logits.data_ptr(), mask=mask8.data_ptr(), candidates0=cand.data_ptr(),
                         sum=total.data_ptr(), count=count.data_ptr(), value=value.data_ptr(), q_lo=q_lo, q_inv_range=q_inv, c_visit=c_visit,
                         c_scale=c_scale, target=target.data_ptr(), v_mix=v_mix.data_ptr())
    L = load()

    def kernel():
        check(L.gvec_search_improved_policy(0, stream(), C.byref(a)), "gvec_search_improved_policy")

    def formulation():
        return torch_policy(logits, legal, cand, total, count, value, q_lo, q_inv, c_visit, c_scale)

    kernel()
    t, v = formulation()
    res = {"rows": n, "actions": A, "m": m, "target_max_abs_diff": float((t - target).abs().max()), "v_mix_max_abs_diff": float((v - v_mix).abs().max()),
           "bytes_moved": n * A * 9}
    res.update(alternate({"kernel": kernel, "torch": formulation}))
    res["speedup"] = res["torch"]["device_us"] / res["kernel"]["device_us"]
    res["kernel_gb_per_s"] = res["bytes_moved"] / res["kernel"]["device_us"] / 1e3
    return res


# ---- a whole decision -----------------------------------------------------------------------------------------------------------
def bench_decision(env, mask, n, P):
    players = (torch.arange(n, device=DEV) % P).to(torch.int32)
    seat_mask = mask[torch.arange(n, device=DEV), players.to(torch.int64)].contiguous()
    hs = HalvingSearch(env, candidates=16, budget=64, depth=8)
    flat = PlayoutSearch(env, candidates=8, replicas=8, depth=8)
    cand0, prior = hs.propose(seat_mask, None, seed=1)
    flat_cand = flat.propose(seat_mask, None, seed=1)
    round_cands = [cand0[:, :K].contiguous() for K, _ in hs.schedule]

    def halving():
        return hs.search(None, players, cand0, prior, 11)

    def playouts_only():                                          # the four playout launches of the same shapes, nothing between them
        for r, c in enumerate(round_cands):
            hs._rounds[r].evaluate(None, players, c, hs.round_seed(11, r))

    def flat_search():
        return flat.scores(flat.evaluate(None, players, flat_cand, 11))

    a, b = halving(), halving()
    res = {"rows": n, "halving": {"candidates": 16, "budget": 64, "depth": 8, "schedule": hs.schedule, "playouts_per_row": hs.playouts_per_row},
           "flat": {"candidates": 8, "replicas": 8, "depth": 8, "playouts_per_row": 64},
           "repeatable": all(bool(torch.equal(a[k], b[k])) for k in a), "rows_with_a_survivor": int(a["found"].sum())}
    res.update(alternate({"halving_search": halving, "halving_playouts_only": playouts_only, "flat_search": flat_search}))
    res["share_not_playout_kernels"] = 1.0 - res["halving_playouts_only"]["device_us"] / res["halving_search"]["device_us"]
    return res


# ---- strength -------------------------------------------------------------------------------------------------------------------
def strength(make, name):
    """bench_search.py's three matches for the searcher make(env)"""
    B, board, eps = args.strength_envs, args.strength_board, args.strength_episodes
    out = {"searcher": name}
    env = GeneralsSelfPlayVecEnv(B, board_width=board, board_height=board, max_players=2, device_outputs=True, seed=42, max_turns=500)
    arena = Arena(env, [playout_policy(make(env), seed=1), random_policy(seed=2)], names=[name, "random"])
    t0 = time.perf_counter()
    steps = arena.run(episodes_per_env=eps, poll_every=32, max_steps=500 * eps + 64)
    res = arena.results()
    out["vs_random"] = {"steps": steps, "seconds": time.perf_counter() - t0, "games": res.totals["games"], "win_rate": res.entrants["win_rate"].tolist()}
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
        env.close()
    return out


def strength_table():
    rows = []
    for depth in (8, 16):
        for rollout in ("agent", "bot"):
            makers = {f"flat-8x8-d{depth}-{rollout}": lambda env, d=depth, r=rollout: PlayoutSearch(env, candidates=8, replicas=8, depth=d, rollout=r),
                      f"halving-16/64-d{depth}-{rollout}": lambda env, d=depth, r=rollout: HalvingSearch(env, candidates=16, budget=64, depth=d, rollout=r),
                      f"halving-64/256-d{depth}-{rollout}": lambda env, d=depth, r=rollout: HalvingSearch(env, candidates=64, budget=256, depth=d, rollout=r)}
            for name, make in makers.items():
                r = strength(make, name)
                print(json.dumps({"searcher": name, "vs_random": r["vs_random"]["win_rate"], "vs_bot_seat": r["seat0_vs_bot_seat"]["win_rate"],
                                  "vs_random_seat": r["seat0_vs_random_seat"]["win_rate"],
                                  "seconds": [round(r[k]["seconds"], 1) for k in ("vs_random", "seat0_vs_bot_seat", "seat0_vs_random_seat")]}), flush=True)
                rows.append(r)
    return rows


def save(out):
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "age": args.age,
           "method": "one process; device time from an event pair around `calls` calls; the median of `repeats` repeats, the paths alternating "
                     "inside every repeat; outputs compared before timing",
           "tail": [], "policy": [], "decision": []}
    for spec in args.shapes.split(","):
        n, wh, P = spec.split(":")
        n, P = int(n), int(P)
        W, H = (int(x) for x in wh.split("x"))
        env, mask = aged_roots(n, W, H, P, args.age)
        for t in args.tails.split(","):
            k, R = (int(x) for x in t.split(":"))
            r = dict(shape=spec, **bench_tail(env, mask, n, P, k, R))
            print(json.dumps({"tail": {x: r[x] for x in ("shape", "k", "replicas", "counts_equal", "sums_max_abs_diff", "rows_with_equal_survivors",
                                                         "kernel", "torch", "speedup")}}), flush=True)
            out["tail"].append(r)
        r = dict(shape=spec, **bench_decision(env, mask, n, P))
        print(json.dumps({"decision": r}), flush=True)
        out["decision"].append(r)
        env.close()
        save(out)
    for spec in args.policy_shapes.split(","):
        n, A = (int(x) for x in spec.split(":"))
        r = bench_policy(n, A)
        print(json.dumps({"policy": r}), flush=True)
        out["policy"].append(r)
        save(out)
    if args.strength:
        out["strength"] = strength_table()
        save(out)


if __name__ == "__main__":
    main()
