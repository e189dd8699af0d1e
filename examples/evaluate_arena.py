#!/usr/bin/env python3
"""Which checkpoint plays better: entrants seated at on-device self-play boards, finished games tallied by one HIP launch
per step (gvec_arena_update), and ratings on the Elo scale fitted to who outlasted whom.

    python examples/train_ppo_selfplay.py --iterations 50 --save a.pt
    python examples/train_ppo_selfplay.py --iterations 200 --save b.pt
    python examples/evaluate_arena.py a.pt b.pt --random --episodes 4

Each positional argument is a checkpoint written by train_ppo_selfplay.py --save; every --random adds an entrant that plays
uniformly over its legal moves; --playouts K:R:D adds a flat Monte Carlo searcher (search.playout_policy: K candidates, R
playouts of D turns each per candidate, one launch per step) whose candidates come from the first checkpoint's logits, or
from a uniform draw when there is no checkpoint; --halving M:N:D adds a sequential-halving searcher beside it
(search.HalvingSearch: M Gumbel-top-m candidates, a budget of N playouts per decision spread over the halving rounds, D turns
deep) with the same prior; --tree M:N:D[:C] adds the search with a tree below the root (search.TreeSearch: M root slots, N
simulations per decision, playouts D turns deep, C child slots per node; the prior also ranks the moves at the nodes below).
--playout-rollout chooses what the searchers' playouts play.
Entrants are seated so that each sits in every column (player seat) equally often (arena.balanced_seating), every env contributes exactly --episodes finished games, and nothing synchronises with the host
between polls.  A multi-player game's pairwise results are treated as independent games by the fit: the ratings rank, their
error bars are not calibrated.  An example, not part of the measured hot path.
"""
import argparse
import importlib.util
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from generalsreinforcementlearning_amd.arena import Arena, random_policy, torch_policy
from generalsreinforcementlearning_amd.features import strategic_features
from generalsreinforcementlearning_amd.search import HalvingSearch, PlayoutSearch, TreeSearch, playout_policy
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv


def _trainer():
    """examples/train_ppo_selfplay.py as a module: the checkpoints' network class lives there"""
    spec = importlib.util.spec_from_file_location("train_ppo_selfplay", os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_ppo_selfplay.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _WithFeatures(torch.nn.Module):
    """a --features checkpoint's input: the observation's nine planes and the five strategic planes computed from them"""
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, obs):
        return self.net(torch.cat([obs, strategic_features(obs)], dim=1))


def load_net(path, board, dev):
    """the network of a checkpoint, in eval mode, taking the observation's nine planes"""
    ck = torch.load(path, map_location=dev)
    if ck["board"] != board:
        raise SystemExit(f"{path} was trained on a {ck['board']}x{ck['board']} board, the arena plays {board}x{board}")
    if ck["memory"]:
        raise SystemExit(f"{path} was trained with --memory: its input carries state from step to step, which an arena entrant "
                         "(a function of the observation) cannot hold")
    net = _trainer().ActorCritic((ck["channels"], board, board), board * board * 5).to(dev)
    net.load_state_dict(ck["model"])
    net.eval()
    return _WithFeatures(net) if ck["features"] else net


def load_entrant(path, board, dev, greedy, seed):
    return torch_policy(load_net(path, board, dev), greedy=greedy, seed=seed)


def parse_playouts(text):
    """'K:R:D' -> (candidates, replicas, depth), each an int >= 1"""
    try:
        k, r, d = (int(x) for x in text.split(":"))
    except ValueError:
        raise SystemExit(f"--playouts wants K:R:D (candidates:replicas:depth), not {text!r}")
    if min(k, r, d) < 1:
        raise SystemExit(f"--playouts {text}: candidates, replicas and depth must be at least 1")
    return k, r, d


def parse_halving(text):
    """'M:N:D' -> (candidates in [1, 64], budget, depth), each an int >= 1"""
    try:
        m, n, d = (int(x) for x in text.split(":"))
    except ValueError:
        raise SystemExit(f"--halving wants M:N:D (candidates:budget:depth), not {text!r}")
    if min(m, n, d) < 1 or m > 64:
        raise SystemExit(f"--halving {text}: candidates (at most 64), budget and depth must be at least 1")
    return m, n, d


def parse_tree(text):
    """'M:N:D' or 'M:N:D:C' -> (candidates in [1, 64], simulations, depth, children in [M, 64] or None), ints >= 1"""
    try:
        parts = [int(x) for x in text.split(":")]
        if len(parts) not in (3, 4):
            raise ValueError
    except ValueError:
        raise SystemExit(f"--tree wants M:N:D or M:N:D:C (candidates:simulations:depth[:children]), not {text!r}")
    m, n, d = parts[:3]
    c = parts[3] if len(parts) == 4 else None
    if min(m, n, d) < 1 or m > 64 or (c is not None and not m <= c <= 64):
        raise SystemExit(f"--tree {text}: candidates (at most 64), simulations and depth must be at least 1, children in [candidates, 64]")
    return m, n, d, c


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoints", nargs="*", help="files written by train_ppo_selfplay.py --save")
    ap.add_argument("--random", action="count", default=0, help="add an entrant that plays uniformly over its legal moves (repeatable)")
    ap.add_argument("--playouts", metavar="K:R:D", default=None,
                    help="add a playout-search entrant: K candidates, R playouts each, D turns deep; its prior is the first checkpoint")
    ap.add_argument("--halving", metavar="M:N:D", default=None,
                    help="add a sequential-halving entrant: M candidates, a budget of N playouts per decision, D turns deep; the same prior")
    ap.add_argument("--tree", metavar="M:N:D[:C]", default=None,
                    help="add a tree-search entrant: M root slots, N simulations per decision, playouts D turns deep, C slots per node")
    ap.add_argument("--playout-rollout", choices=("agent", "bot"), default="agent",
                    help="what the playouts play after the candidate: the random agent, or the scripted opponent's rule on every seat")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--players", type=int, default=2)
    ap.add_argument("--max-turns", type=int, default=500)
    ap.add_argument("--episodes", type=int, default=2, help="finished games every env contributes")
    ap.add_argument("--poll-every", type=int, default=32)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--greedy", action="store_true", help="checkpoints play their legal argmax instead of sampling")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    dev = torch.device("cuda", 0)
    names = [os.path.basename(p) for p in a.checkpoints] + [f"random-{k}" for k in range(a.random)]
    krd = parse_playouts(a.playouts) if a.playouts else None
    if krd:
        names.append(("playouts-bot-%d:%d:%d" if a.playout_rollout == "bot" else "playouts-%d:%d:%d") % krd)
    mnd = parse_halving(a.halving) if a.halving else None
    if mnd:
        names.append(("halving-bot-%d:%d:%d" if a.playout_rollout == "bot" else "halving-%d:%d:%d") % mnd)
    tree = parse_tree(a.tree) if a.tree else None
    if tree:
        names.append(("tree-bot-%d:%d:%d" if a.playout_rollout == "bot" else "tree-%d:%d:%d") % tree[:3])
    if not names:
        raise SystemExit("nothing to evaluate: give checkpoints and / or --random")
    entrants = [load_entrant(p, a.board, dev, a.greedy, a.seed + k) for k, p in enumerate(a.checkpoints)]
    entrants += [random_policy(seed=a.seed + 1000 + k) for k in range(a.random)]
    env = GeneralsSelfPlayVecEnv(a.num_envs, board_width=a.board, board_height=a.board, max_players=a.players, max_turns=a.max_turns,
                                 seed=a.seed, device_outputs=True)
    prior = load_net(a.checkpoints[0], a.board, dev) if a.checkpoints and (krd or mnd or tree) else None
    if krd:
        search = PlayoutSearch(env, candidates=krd[0], replicas=krd[1], depth=krd[2], rollout=a.playout_rollout)
        entrants.append(playout_policy(search, net=prior, seed=a.seed + 2000))
    if mnd:
        halving = HalvingSearch(env, candidates=mnd[0], budget=mnd[1], depth=mnd[2], rollout=a.playout_rollout)
        entrants.append(playout_policy(halving, net=prior, seed=a.seed + 3000))
    if tree:
        def node_prior(obs, mask, net=prior):                    # the checkpoint ranks the moves of the nodes below the root too
            out = net(obs.view(-1, 9, a.board, a.board))
            return out[0] if isinstance(out, (tuple, list)) else out
        searcher = TreeSearch(env, candidates=tree[0], simulations=tree[1], depth=tree[2], children=tree[3], rollout=a.playout_rollout,
                              prior_fn=node_prior if prior is not None else None)
        entrants.append(playout_policy(searcher, net=prior, seed=a.seed + 4000))
    arena = Arena(env, entrants, names=names)
    steps = arena.run(episodes_per_env=a.episodes, poll_every=a.poll_every, max_steps=a.max_steps)
    res = arena.results()
    ratings = res.ratings()
    print(res.table())
    out = {"names": names, "steps": steps, "games": res.totals["games"], "ratings": ratings.tolist(), "score": res.score.tolist(),
           "pair_games": res.games.tolist(), "win_rate": res.entrants["win_rate"].tolist(),
           "elimination_rate": res.entrants["elimination_rate"].tolist(), "mean_length": res.entrants["mean_length"].tolist(),
           "mean_return": res.entrants["mean_return"].tolist(), "games_per_env": res.totals["per_env"]["games"].tolist()}
    print(json.dumps({k: out[k] for k in ("names", "steps", "games", "ratings")}))
    env.close()
    return out


if __name__ == "__main__":
    main()
