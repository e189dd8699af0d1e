#!/usr/bin/env python3
"""A search-distillation learner over on-device self-play: the network's logits are the prior of a sequential-halving
playout search, the search acts, and the network learns the search's improved policy - the AlphaZero-style loop (search,
target, train the prior, search with it) with env, search, rollout store and loss all on one MI355X:

    GeneralsSelfPlayVecEnv(device_outputs=True)  ->  network  ->  HalvingSearch.act (gvec_search_playouts, gvec_search_halve)
        ->  HalvingSearch.policy_target (gvec_search_improved_policy)
        ->  SelfPlayRolloutBuffer(policy_target=True).step (the target and v_mix beside the row)  ->  finish (gvec_traj_gae)
        ->  minibatches  ->  distill_loss / MaskedCategoricalHead.distill (gvec_policy_distill / _backward)

The policy loss is the cross-entropy of the network against the stored target (distill_loss), minus an entropy bonus from
MaskedCategoricalHead.distill on the same rows; there is no PPO ratio.  The value head learns the GAE returns of the rollout as in examples/train_ppo_selfplay.py, whose
network this is.  Every term is weighted by batch["weight"] (0 for re-deal rows and eliminated learners).  An example, not part
of the measured hot path.

    python examples/train_search_distill.py --num-envs 256 --iterations 20 --halving 8:32:8 --playout-rollout bot

--save PATH writes the network where examples/evaluate_arena.py reads it, as the PPO example's.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn as nn

from generalsreinforcementlearning_amd.policy_head import MaskedCategoricalHead, distill_loss
from generalsreinforcementlearning_amd.rollout import SelfPlayRolloutBuffer
from generalsreinforcementlearning_amd.search import HalvingSearch, TreeSearch
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv

from evaluate_arena import parse_halving
from train_ppo_selfplay import ActorCritic


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--players", type=int, default=2)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--max-turns", type=int, default=500)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--value-coef", type=float, default=0.5)
    ap.add_argument("--entropy-coef", type=float, default=0.01)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--halving", metavar="M:N:D", default="8:32:8",
                    help="the acting search: M Gumbel-top-m candidates, a budget of N playouts per decision, D turns deep")
    ap.add_argument("--search", choices=("halving", "tree"), default="halving",
                    help="halving: the one-ply search; tree: TreeSearch, M root slots and N simulations with a tree below the root, "
                         "the network ranking the moves of the inner nodes too")
    ap.add_argument("--playout-rollout", choices=("agent", "bot"), default="agent",
                    help="who plays the playouts' turns: the random agent, or the scripted expander bot in every seat")
    ap.add_argument("--bot-random-permille", type=int, default=0,
                    help="with --playout-rollout bot: the share of turns in which a seat plays the agent's draw after all")
    ap.add_argument("--save", default=None, metavar="PATH", help="write the final network (examples/evaluate_arena.py loads it)")
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    dev = torch.device("cuda", 0)
    obs_shape, n_actions = (9, a.board, a.board), a.board * a.board * 5
    net = ActorCritic(obs_shape, n_actions).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=a.lr)
    start = [p.detach().clone() for p in net.parameters()]
    env = GeneralsSelfPlayVecEnv(a.num_envs, board_width=a.board, board_height=a.board, max_players=a.players, max_turns=a.max_turns,
                                 seed=a.seed, device_outputs=True)
    B, L = env.num_envs, env.num_learners
    m, n, d = parse_halving(a.halving)
    if a.search == "tree":
        search = TreeSearch(env, candidates=m, simulations=n, depth=d, rollout=a.playout_rollout, bot_random_permille=a.bot_random_permille,
                            prior_fn=lambda obs, mask: net(obs.view(-1, *obs_shape))[0])
    else:
        search = HalvingSearch(env, candidates=m, budget=n, depth=d, rollout=a.playout_rollout, bot_random_permille=a.bot_random_permille)
    buf = SelfPlayRolloutBuffer(env, horizon=a.horizon, gamma=a.gamma, gae_lambda=a.gae_lambda, policy_target=True)
    head = MaskedCategoricalHead(dev)
    current = lambda: buf.obs.view(B * L, *obs_shape)

    buf.begin(*env.reset())
    out, draws, t0 = [], 0, time.perf_counter()
    for it in range(a.iterations):
        with torch.no_grad():
            while not buf.full:
                logits, value = net(current())
                logits = logits.contiguous()
                mask = buf.valid_actions_mask.view(B * L, n_actions)
                draws += 1                          # one seed per step: candidates and playouts are keyed by it
                actions, info = search.act(mask, logits, seed=(a.seed << 32) + draws)
                slot = buf.policy_target_slot       # the search writes the step's row of the store: step() copies nothing
                target, v_mix = search.policy_target(logits, mask, info, value=None, out=slot.view(B * L, n_actions))
                logp, _ = head.evaluate(logits, mask, actions)
                buf.step(actions, logp, value, policy_target=slot, search_value=v_mix)
            buf.finish(net(current())[1])
        sums = torch.zeros(5, device=dev)           # ce, kl, value loss, entropy, batches
        for batch in buf.minibatches(a.batch_size, epochs=a.epochs, seed=a.seed + it):
            w = batch["weight"]
            cnt = w.sum().clamp_min(1.0)
            logits, value = net(batch["obs"])
            mask, target = batch["valid_actions_mask"], batch["policy_target"]
            ce = distill_loss(logits, mask, target, w)
            _, kl, entropy = head.distill(logits, mask, target)         # kl for the log, the entropy for its bonus
            vl = (0.5 * (value - batch["returns"]) ** 2 * w).sum() / cnt
            ent = (entropy * w).sum() / cnt
            loss = ce + a.value_coef * vl - a.entropy_coef * ent
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(net.parameters(), 0.5)
            opt.step()
            with torch.no_grad():
                sums += torch.stack([ce, (kl * w).sum() / cnt, vl, ent, torch.ones((), device=dev)])
        valid = float(buf.stats[0])                 # the iteration's one host read (with the sums below)
        buf.next_rollout()
        s = (sums[:4] / sums[4].clamp_min(1.0)).tolist()
        row = {"iteration": it, "ce": s[0], "kl": s[1], "value_loss": s[2], "entropy": s[3],
               "valid_rows": valid / (a.horizon * B * L), "env_steps": (it + 1) * a.horizon * B,
               "playouts_per_decision": search.playouts_per_row, "seconds": time.perf_counter() - t0}
        print(json.dumps(row))
        out.append(row)
    moved = max(float((p.detach() - q).abs().max()) for p, q in zip(net.parameters(), start))
    result = {"iterations": out, "rejected": int(buf.rejected.item()), "parameter_change": moved}
    if a.save:
        torch.save({"model": net.state_dict(), "board": a.board, "players": a.players, "channels": 9, "features": False,
                    "memory": False}, a.save)
    env.close()
    return result


if __name__ == "__main__":
    main()
