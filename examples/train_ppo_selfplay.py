#!/usr/bin/env python3
"""A PPO learner over on-device self-play - every player of every board is a learner of one shared network, and env,
rollout store, action head and learner all stay on one MI355X:

    GeneralsSelfPlayVecEnv(device_outputs=True)  ->  network  ->  MaskedCategoricalHead.sample (gvec_policy_sample)
        ->  SelfPlayRolloutBuffer.step (gvec_gym_step_players into slot t + 1, gvec_traj_record)  ->  finish (gvec_traj_gae)
        ->  minibatches (gvec_traj_gather)  ->  MaskedCategoricalHead.evaluate (gvec_policy_evaluate / _backward)

The loss is the clipped PPO surrogate with a value loss and an entropy bonus, every term weighted by batch["weight"] (0 for
re-deal rows and eliminated learners).  The reference plans this phase (documentation/MASTER_PLAN.md:158-172) and has no
learner for it; the code is this repo's own.  An example, not part of the measured hot path.

    python examples/train_ppo_selfplay.py --num-envs 1024 --iterations 50

--features adds the five strategic feature planes (features.strategic_features: distances to the own general, the nearest
enemy, city and fogged tile, and the front line) to the nine of the observation.  The store keeps nine planes per row: the
five are recomputed from them where they are consumed, while acting and on every minibatch.

--memory adds the four fog-of-war memory planes (memory.ObservationMemory: seen, last owner, last army, age): what the learner
last saw of every tile, which the observation forgets the moment the tile is fogged again.  They are state, not a function of
one observation, so the rollout buffer stores them per step (SelfPlayRolloutBuffer(memory=)).  With --features as well the
features are computed from remembered_observation: the distance to the nearest enemy tile seen so far.

--actor-lag K lets a frozen copy of the network act, refreshed from the learner every K iterations: the actor-learner
pattern, in one process.  --vtrace replaces GAE by V-trace targets (SelfPlayRolloutBuffer.evaluate_rollout re-scores the
stored rows with the learner in place, finish_vtrace runs gvec_traj_vtrace), recomputed before every epoch, so that neither
the lag nor the gradient steps already taken on this rollout bias them; --rho-bar / --c-bar are its two truncation levels.
The surrogate stays PPO's, on the ratio to the stored (behaviour) log-probs, with V-trace's pg as the advantage and vs as
the value target.

--arena-every K --arena-episodes k rates the learner as it goes: every K iterations the current network plays the frozen
snapshots taken K, 2K, ... iterations ago (at most four are kept) in a match arena (arena.Arena: its own small batch of
boards, k finished games per board, every entrant in every seat equally often), the row of that iteration gains its rating
with the oldest snapshot anchored at 1500, and the current network joins the snapshots.  --save PATH writes the final network
where examples/evaluate_arena.py reads it.
"""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from generalsreinforcementlearning_amd.arena import Arena, torch_policy
from generalsreinforcementlearning_amd.features import NUM_STRATEGIC_FEATURES, strategic_features
from generalsreinforcementlearning_amd.memory import NUM_MEMORY_PLANES, ObservationMemory, remembered_observation
from generalsreinforcementlearning_amd.policy_head import MaskedCategoricalHead
from generalsreinforcementlearning_amd.reward import RewardConfig
from generalsreinforcementlearning_amd.rollout import SelfPlayRolloutBuffer
from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv


class ActorCritic(nn.Module):
    def __init__(self, obs_shape, n_actions, width=64):
        super().__init__()
        c, h, w = obs_shape
        self.torso = nn.Sequential(nn.Conv2d(c, width, 3, padding=1), nn.ReLU(), nn.Conv2d(width, width, 3, padding=1), nn.ReLU())
        self.policy = nn.Conv2d(width, 5, 1)
        self.value = nn.Sequential(nn.Conv2d(width, 4, 1), nn.ReLU(), nn.Flatten(), nn.Linear(4 * h * w, 1))
        self.n_actions = n_actions

    def forward(self, x):
        # five action planes (up, right, down, left, half) per tile -> the env's index tile * 5 + d
        z = self.torso(x)
        return self.policy(z).permute(0, 2, 3, 1).reshape(x.shape[0], self.n_actions), self.value(z).squeeze(1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--players", type=int, default=2)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--max-turns", type=int, default=500)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--value-coef", type=float, default=0.5)
    ap.add_argument("--entropy-coef", type=float, default=0.01)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--features", action="store_true", help="feed the five strategic feature planes next to the observation's nine")
    ap.add_argument("--memory", action="store_true", help="feed the four fog-of-war memory planes (what each tile last showed, and how long ago)")
    ap.add_argument("--vtrace", action="store_true", help="V-trace targets from the learner's own log-probs and values, before every epoch")
    ap.add_argument("--rho-bar", type=float, default=1.0, help="V-trace: truncation of the importance weight of the TD error")
    ap.add_argument("--c-bar", type=float, default=1.0, help="V-trace: truncation of the trace coefficient")
    ap.add_argument("--actor-lag", type=int, default=0, metavar="K",
                    help="a frozen copy of the network acts, refreshed every K iterations (0: the learner itself acts)")
    ap.add_argument("--arena-every", type=int, default=0, metavar="K",
                    help="every K iterations, rate the network against frozen snapshots of itself (0: never)")
    ap.add_argument("--arena-episodes", type=int, default=2, metavar="k", help="finished games per arena board")
    ap.add_argument("--arena-envs", type=int, default=256, help="boards of the arena's own env")
    ap.add_argument("--save", default=None, metavar="PATH", help="write the final network (examples/evaluate_arena.py loads it)")
    ap.add_argument("--reward", choices=("gym", "go", "sparse"), default="gym",
                    help="gym: GeneralsEnv's own reward; go: the reference's DefaultRewardConfig, clipped, -0.1 for a refused action; "
                         "sparse: +-1 on the last step of a game and nothing else (RewardConfig)")
    a = ap.parse_args(argv)
    if a.arena_every > 0 and a.memory:
        ap.error("--arena-every cannot rate a --memory network: an arena entrant is a function of the observation alone")

    torch.manual_seed(a.seed)
    dev = torch.device("cuda", 0)
    obs_shape, n_actions = (9, a.board, a.board), a.board * a.board * 5
    channels = 9 + (NUM_MEMORY_PLANES if a.memory else 0) + (NUM_STRATEGIC_FEATURES if a.features else 0)
    net = ActorCritic((channels,) + obs_shape[1:], n_actions).to(dev)

    def inputs(o, m):
        """the network's input of observations [N, 9, H, W] and their memory planes [N, 4, H, W] (None without --memory).
        The features are a pure function of those, so stored rows need no planes for them."""
        planes = [o] if m is None else [o, m]
        if a.features:
            planes.append(strategic_features(o if m is None else remembered_observation(o, m)))
        return torch.cat(planes, dim=1) if len(planes) > 1 else o

    opt = torch.optim.Adam(net.parameters(), lr=a.lr)
    start = [p.detach().clone() for p in net.parameters()]
    reward_config = {"gym": None, "go": RewardConfig.clipped(), "sparse": RewardConfig.sparse()}[a.reward]
    env = GeneralsSelfPlayVecEnv(a.num_envs, board_width=a.board, board_height=a.board, max_players=a.players, max_turns=a.max_turns,
                                 seed=a.seed, device_outputs=True, reward_config=reward_config)
    B, L = env.num_envs, env.num_learners
    memory = ObservationMemory((B, L), a.board, a.board, device=dev) if a.memory else None
    buf = SelfPlayRolloutBuffer(env, horizon=a.horizon, gamma=a.gamma, gae_lambda=a.gae_lambda, memory=memory)
    head = MaskedCategoricalHead(dev)
    current = lambda: inputs(buf.obs.view(B * L, *obs_shape), buf.memory.view(B * L, NUM_MEMORY_PLANES, *obs_shape[1:]) if a.memory else None)
    actor = copy.deepcopy(net).requires_grad_(False) if a.actor_lag > 0 else net
    rho_stats = torch.zeros(4, dtype=torch.float64, device=dev)

    def passes(it):
        """the iteration's minibatches; with --vtrace the targets are rebuilt from the learner as it stands before each epoch"""
        if not a.vtrace:
            yield from buf.minibatches(a.batch_size, epochs=a.epochs, seed=a.seed + it)
            return
        for epoch in range(a.epochs):
            logp, value = buf.evaluate_rollout(lambda o, m: net(inputs(o, m)), head, chunk_rows=a.batch_size)
            with torch.no_grad():
                last = net(current())[1]
            buf.finish_vtrace(last, logp, value=value, rho_bar=a.rho_bar, c_bar=a.c_bar)
            if epoch == 0:
                rho_stats.copy_(buf.stats)          # how far off-policy the rollout is before the first gradient step
            yield from buf.minibatches(a.batch_size, epochs=1, seed=(a.seed + it) * a.epochs + epoch)

    snapshots, arena_env = [], None

    def rate(it):
        """the current network against the snapshots in an arena of its own -> the row's "arena" entry (None before the
        first snapshot exists); then the current network becomes the newest snapshot, and the oldest of five leaves"""
        nonlocal arena_env
        entry = None
        if snapshots:
            if arena_env is None:
                arena_env = GeneralsSelfPlayVecEnv(a.arena_envs, board_width=a.board, board_height=a.board, max_players=a.players,
                                                   max_turns=a.max_turns, seed=a.seed + 1, device_outputs=True)
            play = lambda n, k: torch_policy(lambda o: n(inputs(o, None)), head, seed=a.seed + 7919 * it + k)
            arena = Arena(arena_env, [play(n, k) for k, n in enumerate(snapshots)] + [play(net, len(snapshots))],
                          names=[f"iteration {i}" for i in snapshot_its] + ["current"])
            arena.reset(seed=a.seed + 1 + it)
            arena.run(episodes_per_env=a.arena_episodes)
            res = arena.results()
            ratings = res.ratings(anchor=0)
            entry = {"rating": float(ratings[-1]), "snapshot_ratings": ratings[:-1].tolist(), "snapshot_iterations": list(snapshot_its),
                     "win_rate": float(res.entrants["win_rate"][-1]), "games": int(res.totals["games"])}
        snapshots.append(copy.deepcopy(net).requires_grad_(False))
        snapshot_its.append(it)
        del snapshots[:-4], snapshot_its[:-4]
        return entry

    snapshot_its = []
    buf.begin(*env.reset())
    out, draws, t0 = [], 0, time.perf_counter()
    for it in range(a.iterations):
        if a.actor_lag > 0 and it % a.actor_lag == 0:
            actor.load_state_dict(net.state_dict())
        with torch.no_grad():
            while not buf.full:
                logits, value = actor(current())
                draws += 1                          # one seed per step: a draw is keyed by (seed, row, action index)
                actions, logp, _ = head.sample(logits.view(B, L, n_actions), buf.valid_actions_mask, seed=(a.seed << 32) + draws)
                buf.step(actions, logp, value)
            if not a.vtrace:
                buf.finish(net(current())[1])
        sums = torch.zeros(5, device=dev)           # policy loss, value loss, entropy, clipped share, batches
        for batch in passes(it):
            w = batch["weight"]
            n = w.sum().clamp_min(1.0)
            logits, value = net(inputs(batch["obs"], batch.get("memory")))
            logp, entropy = head.evaluate(logits, batch["valid_actions_mask"], batch["action"])
            ratio = (logp - batch["logp"]).exp()
            adv = batch["advantages"]
            pg = -(torch.min(ratio * adv, ratio.clamp(1 - a.clip, 1 + a.clip) * adv) * w).sum() / n
            vl = (0.5 * (value - batch["returns"]) ** 2 * w).sum() / n
            ent = (entropy * w).sum() / n
            loss = pg + a.value_coef * vl - a.entropy_coef * ent
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(net.parameters(), 0.5)
            opt.step()
            with torch.no_grad():
                sums += torch.stack([pg, vl, ent, (((ratio - 1).abs() > a.clip).float() * w).sum() / n, torch.ones((), device=dev)])
        valid = float(buf.stats[0])                 # the iteration's one host read (with the sums below)
        mean_rho = float(rho_stats[3] / rho_stats[0].clamp_min(1.0)) if a.vtrace else None
        buf.next_rollout()
        s = (sums[:4] / sums[4].clamp_min(1.0)).tolist()
        row = {"iteration": it, "policy_loss": s[0], "value_loss": s[1], "entropy": s[2], "clip_fraction": s[3],
               "valid_rows": valid / (a.horizon * B * L), "env_steps": (it + 1) * a.horizon * B,
               "mean_rho": mean_rho, "seconds": time.perf_counter() - t0}
        if a.arena_every > 0 and (it + 1) % a.arena_every == 0:
            row["arena"] = rate(it)
        print(json.dumps(row))
        out.append(row)
    moved = max(float((p.detach() - q).abs().max()) for p, q in zip(net.parameters(), start))
    result = {"iterations": out, "bad_actions": head.bad_actions, "rejected": int(buf.rejected.item()), "parameter_change": moved}
    if reward_config is not None:
        result["reward"] = a.reward
    if a.save:
        torch.save({"model": net.state_dict(), "board": a.board, "players": a.players, "channels": channels, "features": a.features,
                    "memory": a.memory}, a.save)
    if arena_env is not None:
        arena_env.close()
    env.close()
    return result


if __name__ == "__main__":
    main()
