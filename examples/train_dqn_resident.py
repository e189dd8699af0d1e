#!/usr/bin/env python3
"""A DQN learner over the resident collection loop - what `python/train_dqn_parallel.py` of the reference does with
ParallelEnvPool + ReplayBuffer over gRPC, here with env, policy, replay ring and learner all on one MI355X:

    GeneralsVecEnv(device_outputs=True)  ->  epsilon-greedy over the masked Q values (one forward for all envs)
        ->  gvec_gym_step  ->  gvec_pool_collect (ring in HBM, episode results)  ->  DeviceReplayBuffer.sample_arrays

The network, loss and exploration scheme follow the reference's choices in outline (a small conv net over the (9, H, W)
observation, Huber loss, gradient clipping at 1.0, a hard target update, fixed per-worker exploration rates spread
geometrically over the workers); the code is this repo's own.  An example, not part of the measured hot path.

    python examples/train_dqn_resident.py --num-envs 4096 --updates 200 [--prioritized] [--n-step 3]
        [--masked-targets | --double | --categorical --atoms 51 --v-min -110 --v-max 110] [--augment]

--masked-targets bootstraps from the best LEGAL action of the next state (the mask is rebuilt from the sampled next
observation: the ring stores none), --double picks that action with the online network (Double DQN), --categorical learns a
distribution over --atoms returns per action (C51) with the same masked Double selection: q_targets.py, one launch per batch.
--augment gives every sampled row a board symmetry of its own (symmetry.py, one launch per batch) before the targets: the
network ends in a Linear over the flattened board, so it shares nothing between a position and its mirror image.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

from generalsreinforcementlearning_amd.env_pool import ParallelVecEnvPool
from generalsreinforcementlearning_amd.q_targets import categorical_target, double_q_target
from generalsreinforcementlearning_amd.reward import RewardConfig
from generalsreinforcementlearning_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
from generalsreinforcementlearning_amd.symmetry import augment_transition
from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv


class QNet(nn.Module):
    def __init__(self, obs_shape, n_actions, width=64):
        super().__init__()
        c, h, w = obs_shape
        self.body = nn.Sequential(nn.Conv2d(c, width, 3, padding=1), nn.ReLU(), nn.Conv2d(width, width, 3, padding=1), nn.ReLU(),
                                  nn.Conv2d(width, 5, 1))
        self.n_actions = n_actions

    def forward(self, x):
        # five action planes (up, right, down, left, half) per tile -> the env's index tile * 5 + d
        return self.body(x).permute(0, 2, 3, 1).reshape(x.shape[0], self.n_actions)


class CategoricalQNet(nn.Module):
    """N atom logits per action.  The last 1x1 convolution has 5 * N channels and runs in channels_last, so its output read
    as [B, H, W, 5, N] - which is [B, A, N] with the env's action index, atoms innermost - is a view: no permute copy."""

    def __init__(self, obs_shape, n_actions, atoms, v_min, v_max, width=64):
        super().__init__()
        c, h, w = obs_shape
        self.body = nn.Sequential(nn.Conv2d(c, width, 3, padding=1), nn.ReLU(), nn.Conv2d(width, width, 3, padding=1), nn.ReLU(),
                                  nn.Conv2d(width, 5 * atoms, 1)).to(memory_format=torch.channels_last)
        self.n_actions, self.atoms = n_actions, atoms
        self.register_buffer("support", torch.linspace(v_min, v_max, atoms))

    def forward(self, x):
        y = self.body(x.contiguous(memory_format=torch.channels_last))
        return y.permute(0, 2, 3, 1).reshape(x.shape[0], self.n_actions, self.atoms)

    def expected(self, logits):
        return (torch.softmax(logits, -1) * self.support).sum(-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--collect-per-update", type=int, default=4, help="vector steps between two learner steps")
    ap.add_argument("--warmup-steps", type=int, default=8)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--target-every", type=int, default=50)
    ap.add_argument("--max-steps-per-episode", type=int, default=200)
    ap.add_argument("--eps-base", type=float, default=0.4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--prioritized", action="store_true", help="prioritized replay: weighted loss, priorities from the batch's TD errors")
    ap.add_argument("--per-alpha", type=float, default=0.6)
    ap.add_argument("--per-beta", type=float, default=0.4)
    ap.add_argument("--n-step", type=int, default=1, help="multi-step targets: returns + discounts * (1 - dones) * max Q(next), from the ring's links")
    ap.add_argument("--masked-targets", action="store_true", help="bootstrap from the best LEGAL action of the next state")
    ap.add_argument("--double", action="store_true", help="Double DQN: the online network picks the next action among the legal ones")
    ap.add_argument("--categorical", action="store_true", help="C51: a distribution over --atoms returns per action, masked Double targets")
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--v-min", type=float, default=None,
                    help="the support's bounds; default: -110 / 110 for --reward gym (the env's terminal +-100), else the config's "
                         "lose_game / win_game widened by a tenth and by invalid_action")
    ap.add_argument("--v-max", type=float, default=None)
    ap.add_argument("--reward", choices=("gym", "go", "sparse"), default="gym",
                    help="gym: GeneralsEnv's own reward; go: the reference's DefaultRewardConfig, clipped, -0.1 for a refused action; "
                         "sparse: +-1 on the last step of a game and nothing else (RewardConfig)")
    ap.add_argument("--augment", action="store_true", help="a random board symmetry per sampled row (mirrors, quarter turns)")
    a = ap.parse_args(argv)
    reward_config = {"gym": None, "go": RewardConfig.clipped(), "sparse": RewardConfig.sparse()}[a.reward]
    if reward_config is None:
        lo, hi = -110.0, 110.0
    else:      # an episode's return is dominated by its last step: the outcome, a margin for the shaped steps before it
        lo = 1.1 * min(reward_config.lose_game, -reward_config.win_game) - abs(reward_config.invalid_action)
        hi = 1.1 * max(reward_config.win_game, -reward_config.lose_game) + abs(reward_config.invalid_action)
    a.v_min, a.v_max = (lo if a.v_min is None else a.v_min), (hi if a.v_max is None else a.v_max)

    torch.manual_seed(a.seed)
    dev = torch.device("cuda", 0)
    B, n_actions, obs_shape = a.num_envs, a.board * a.board * 5, (9, a.board, a.board)
    if a.categorical:
        q, target = (CategoricalQNet(obs_shape, n_actions, a.atoms, a.v_min, a.v_max).to(dev) for _ in range(2))
    else:
        q, target = QNet(obs_shape, n_actions).to(dev), QNet(obs_shape, n_actions).to(dev)
    target.load_state_dict(q.state_dict())
    opt = torch.optim.Adam(q.parameters(), lr=a.lr)
    # one fixed exploration rate per worker, eps_base ** (1 .. 8) across the pool
    eps = a.eps_base ** (1 + 7 * torch.arange(B, device=dev) / max(B - 1, 1))

    def policy(states, masks, _workers, gen):
        with torch.no_grad():
            qv = q(states)
            if a.categorical:
                qv = q.expected(qv)             # greedy over expected values
            qv = qv.masked_fill(~masks, float("-inf"))
            greedy = qv.argmax(1)
            explore = (masks * torch.rand(masks.shape, device=dev, generator=gen)).argmax(1)      # a uniform valid action
            return torch.where(torch.rand(B, device=dev, generator=gen) < eps, explore, greedy)

    if a.prioritized:
        buf = PrioritizedDeviceReplayBuffer(a.buffer_size, alpha=a.per_alpha, beta=a.per_beta, n_step=a.n_step, gamma=a.gamma)
    else:
        buf = DeviceReplayBuffer(a.buffer_size, n_step=a.n_step, gamma=a.gamma)
    pool = ParallelVecEnvPool(B, lambda n: GeneralsVecEnv(n, board_width=a.board, board_height=a.board, max_players=2, max_turns=a.max_steps_per_episode,
                                                         seed=a.seed, device_outputs=True, reward_config=reward_config),
                              policy, buf, max_steps_per_episode=a.max_steps_per_episode, seed=a.seed, batched_actions=True)
    sym_gen = torch.Generator(device=dev)
    sym_gen.manual_seed(a.seed)
    pool.collect(a.warmup_steps)
    losses, t0 = [], time.perf_counter()
    for u in range(a.updates):
        pool.collect(a.collect_per_update)
        if a.n_step > 1:                            # r: the discounted sum of up to n rewards; ns, d: the chain's last row
            if a.prioritized:
                s, act, r, ns, d, disc, _steps, slots, weights = buf.sample_nstep_prioritized(a.batch_size)
            else:
                s, act, r, ns, d, disc, _steps = buf.sample_nstep(a.batch_size)
            disc = disc.float()                     # gamma ** steps: a chain cut short by its episode's end bootstraps sooner
        else:
            if a.prioritized:
                s, act, r, ns, d, slots, weights = buf.sample_prioritized(a.batch_size)
            else:
                s, act, r, ns, d = buf.sample_arrays(a.batch_size)
            disc = a.gamma
        if a.augment:                               # s, act and ns under one symmetry per row; the masked targets rebuild the mask from ns
            s, act, ns, _ = augment_transition(s, act, ns, generator=sym_gen)
        if a.categorical:
            with torch.no_grad():               # the projected distribution of the best legal next action (picked by the online net)
                m, _ = categorical_target(ns, target(ns), r, disc, d, a.v_min, a.v_max, logits_select=q(ns))
            logp = F.log_softmax(q(s)[torch.arange(len(act), device=dev), act], -1)
            ce = -(m * logp).sum(-1)            # per row: the loss, and the priority
            if a.prioritized:
                loss = (weights * ce).mean()
                buf.update_priorities(slots, ce.detach())
            else:
                loss = ce.mean()
        else:
            with torch.no_grad():
                if a.masked_targets or a.double:
                    tq, _ = double_q_target(ns, target(ns), r, disc, d, q_select=q(ns) if a.double else None)
                else:
                    tq = r.float() + disc * target(ns).max(1).values * (~d).float()
            qsa = q(s).gather(1, act[:, None]).squeeze(1)
            if a.prioritized:
                loss = (weights * F.smooth_l1_loss(qsa, tq, reduction="none")).mean()
                buf.update_priorities(slots, (qsa.detach() - tq))
            else:
                loss = F.smooth_l1_loss(qsa, tq)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        nn.utils.clip_grad_norm_(q.parameters(), 1.0)
        opt.step()
        if (u + 1) % a.target_every == 0:
            target.load_state_dict(q.state_dict())
        if (u + 1) % 50 == 0 or u + 1 == a.updates:
            losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    results = pool.pop_episode_results()
    out = {"updates": a.updates, "env_steps": pool.total_env_steps, "episodes": pool.total_episodes, "seconds": dt,
           "env_steps_per_s": a.updates * a.collect_per_update * B / dt, "updates_per_s": a.updates / dt, "loss": losses,
           "mean_episode_reward": sum(x[0] for x in results) / max(len(results), 1), "ring_fill": len(buf), "n_step": a.n_step}
    if a.categorical or a.masked_targets or a.double:
        out["targets"] = f"categorical{a.atoms}" if a.categorical else "double" if a.double else "masked"
    if a.augment:
        out["augment"] = True
    if reward_config is not None:
        out["reward"], out["v_min"], out["v_max"] = a.reward, a.v_min, a.v_max
    pool._env.close()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
