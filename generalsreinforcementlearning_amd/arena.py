"""Match arena — which agent is better: finished games counted on the device, entrants seated at self-play boards, and an
Elo-scale rating fitted to the pairwise results (include/generals_vec.h "match arena").

    env = GeneralsSelfPlayVecEnv(4096, max_players=4, device_outputs=True)
    arena = Arena(env, [torch_policy(net_a), torch_policy(net_b), random_policy(seed=1)])
    arena.run(episodes_per_env=4)                 # every env contributes exactly its first four finished games
    res = arena.results()
    print(res.table())                            # win rate, elimination rate, mean length and return per entrant, and ratings

EpisodeTally is the counting half and works on its own inside any training loop:

    tally = EpisodeTally(env.num_envs, env.num_learners, env.player_ids)
    obs, reward, terminated, truncated, info = env.step(actions)
    tally.update_from_step(obs, reward, terminated, truncated, info)      # one launch, no host sync
    ...
    print(tally.totals()["wins"])                                         # the one synchronising call

One HIP launch per env step (gvec_arena_update: one wavefront per env, all state per env, no atomics) on the current torch
stream.  A column is one learner seat of the env (player_ids[column]); an entrant is a policy; the seating says which entrant
plays which column of which env, and stays fixed for an arena's lifetime.
"""
import ctypes as C
import itertools

import numpy as np

from . import _obs_batch as ob
from ._lib import ArenaArgs, check, load

MAX_LEARNERS = 8      # GVEC_MAX_PLAYERS

# (name, torch dtype name, shape letters) of the per-env state, in the order state_dict() and totals() walk it
_RUNNING = (("death", "int32", "BL"), ("ep_len", "int32", "B"), ("ep_return", "float64", "BL"))
_TOTALS = (("games", "int32", "B"), ("wins", "int32", "BL"), ("eliminated", "int32", "BL"), ("len_sum", "int64", "B"),
           ("ret_sum", "float64", "BL"), ("pair2", "int32", "BLL"))


def _int(v, name, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an int, not {type(v).__name__}")
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} {v} outside [{lo}, {'...' if hi is None else hi}]")
    return int(v)


class EpisodeTally:
    def __init__(self, num_envs, num_learners, player_ids=None, games_cap=0, device=None):
        """num_envs B, num_learners L in [1, 8].  player_ids: the player id of every column (None: 0..L-1), what `winner` is
        compared with.  games_cap k > 0: an env counts its first k finished games and ignores the later ones (0: no cap).
        device: a CUDA device (None: the first update's).  Nothing is allocated until the state is read or updated."""
        import torch
        self._t = torch
        self.num_envs = _int(num_envs, "num_envs", 0, 2 ** 31 - 1)
        self.num_learners = _int(num_learners, "num_learners", 1, MAX_LEARNERS)
        ids = list(range(self.num_learners)) if player_ids is None else [_int(p, "a player id", -128, 127) for p in player_ids]
        if len(ids) != self.num_learners:
            raise ValueError(f"player_ids {ids} does not name {self.num_learners} columns")
        self.player_ids = ids
        self.games_cap = games_cap
        self._dev = None if device is None else torch.device(device)
        if self._dev is not None and self._dev.type != "cuda":
            raise ValueError(f"device {self._dev} is not a CUDA device: the tally is kept by a HIP kernel (there is no host path)")
        self._state = None           # None: all zeros, and not materialised yet
        self._ids = None

    @property
    def games_cap(self):
        return self._cap

    @games_cap.setter
    def games_cap(self, k):
        self._cap = _int(k, "games_cap", 0, 2 ** 31 - 1)

    # ---- state --------------------------------------------------------------------------------------------------------
    def _shape(self, letters):
        return tuple({"B": self.num_envs, "L": self.num_learners}[c] for c in letters)

    def _device(self):
        if self._dev is None or self._dev.index is None:
            self._dev = self._t.device("cuda", self._t.cuda.current_device())
        return self._dev

    @property
    def state(self):
        """{name: tensor} of the running state (death, ep_len, ep_return) and the totals (games, wins, eliminated, len_sum,
        ret_sum, pair2): the tensors the kernel updates, on the device."""
        if self._state is None:
            t, dev = self._t, self._device()
            self._state = {n: t.zeros(self._shape(s), dtype=getattr(t, d), device=dev) for n, d, s in _RUNNING + _TOTALS}
            self._ids = t.tensor(self.player_ids, dtype=t.int32, device=dev)
        return self._state

    def __getattr__(self, name):                 # tally.games, tally.pair2, ...: the state tensors by name
        if name in {n for n, _, _ in _RUNNING + _TOTALS}:
            return self.state[name]
        raise AttributeError(name)

    def reset_all(self):
        """Every total and every running episode starts from zero again."""
        if self._state is not None:
            for v in self._state.values():
                v.zero_()

    def state_dict(self):
        """A copy of the state with what it was built for."""
        return {"state": {k: v.clone() for k, v in self.state.items()}, "num_envs": self.num_envs, "num_learners": self.num_learners,
                "player_ids": list(self.player_ids), "games_cap": self.games_cap}

    def load_state_dict(self, sd):
        for k in ("num_envs", "num_learners", "player_ids"):
            if (list(sd[k]) if k == "player_ids" else sd[k]) != getattr(self, k):
                raise ValueError(f"load_state_dict: the state was saved with {k} = {sd[k]}, this tally has {getattr(self, k)}")
        mine = self.state
        for k, v in mine.items():
            src = sd["state"][k]
            if tuple(src.shape) != tuple(v.shape) or src.dtype != v.dtype:
                raise ValueError(f"load_state_dict: {k} {tuple(src.shape)} {src.dtype} is not {v.dtype} {tuple(v.shape)}")
        for k, v in mine.items():
            v.copy_(sd["state"][k])
        self.games_cap = sd["games_cap"]

    # ---- the update ---------------------------------------------------------------------------------------------------
    def update(self, alive, terminated, truncated, winner, reward, reset=None, obs=None):
        """One env step.  alive bool / uint8 [B, L] or None (nobody is ever recorded as eliminated), terminated, truncated and
        reset (None: no env was re-dealt) bool / uint8 [B], winner int8 [B], reward float64 [B, L], obs float32
        [B, L, 9, H, W] or None (then survivors of a truncated game tie) - CUDA tensors on the tally's device; obs is read in
        place when its rows have one common stride (a rollout slot) and copied otherwise.  One launch on the current stream;
        TypeError / ValueError before any launch."""
        t = self._t
        B, L = self.num_envs, self.num_learners
        flags = (t.bool, t.uint8)
        # types and shapes first, devices after: a wrong shape is reported as such whatever holds the tensor
        per_env = {"terminated": terminated, "truncated": truncated, "reset": reset}
        for name, x in per_env.items():
            if x is not None or name != "reset":
                ob.check_tensor(x, name, flags)
        if alive is not None:
            ob.check_tensor(alive, "alive", flags)
        ob.check_tensor(winner, "winner", (t.int8,))
        ob.check_tensor(reward, "reward", (t.float64,))
        if obs is not None:
            ob.check_tensor(obs, "obs", (t.float32,))
        for name, x in {**per_env, "winner": winner}.items():
            if x is not None and tuple(x.shape) != (B,):
                raise ValueError(f"{name} {tuple(x.shape)} is not {(B,)}")
        for name, x in (("alive", alive), ("reward", reward)):
            if x is not None and tuple(x.shape) != (B, L):
                raise ValueError(f"{name} {tuple(x.shape)} is not {(B, L)}")
        W = H = stride = 0
        if obs is not None:
            lead, _, H, W = ob.read_shape(obs, "obs")
            if lead != (B, L):
                raise ValueError(f"obs {tuple(obs.shape)} is not {(B, L, 9, H, W)}")
        dev = ob.check_device("the tally is kept by a HIP kernel", "terminated", terminated=terminated, truncated=truncated, winner=winner,
                              reward=reward, alive=alive, reset=reset, obs=obs)
        if self._dev is None or self._dev.index is None:
            self._dev = dev
        if dev != self._dev:
            raise ValueError(f"terminated is on {dev}, the tally on {self._dev}")
        s = self.state
        if not B:
            return
        if obs is not None:
            obs, stride = ob.in_place(obs, 3, H, W)
        p = lambda x: None if x is None else x.contiguous().data_ptr()     # per-env and per-column arrays: dense already
        a = ArenaArgs(rows=B, width=W, height=H, num_learners=L, games_cap=self._cap, obs_row_stride=stride, alive=p(alive),
                      terminated=p(terminated), truncated=p(truncated), reset=p(reset), winner=p(winner), reward=p(reward),
                      player_ids=self._ids.data_ptr(), obs=ob.ptr(obs), **{k: v.data_ptr() for k, v in s.items()})
        check(load().gvec_arena_update(dev.index, ob.stream(dev), C.byref(a)), "gvec_arena_update")

    def update_from_step(self, obs, reward, terminated, truncated, info):
        """update() from what GeneralsSelfPlayVecEnv.step (device_outputs=True) returned."""
        self.update(info["alive"], terminated, truncated, info["winner"], reward, reset=info["reset"], obs=obs)

    # ---- reading ------------------------------------------------------------------------------------------------------
    def totals(self):
        """The totals on the host: ONE device-to-host copy (the only synchronising call of this class), then numpy.
        {"games": int, "len_sum": int, "wins", "eliminated", "ret_sum": [L], "pair2": [L, L]} summed over the envs, and
        "per_env": the six tables as they are."""
        t = self._t
        s = self.state
        packed = t.cat([s[n].reshape(-1).view(t.uint8) for n, _, _ in _TOTALS]).cpu().numpy()
        per_env, at = {}, 0
        for n, d, letters in _TOTALS:
            shape = self._shape(letters)
            nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(d).itemsize
            per_env[n] = packed[at:at + nbytes].view(d).reshape(shape).copy()
            at += nbytes
        out = {n: per_env[n].sum(axis=0, dtype=np.float64 if d == "float64" else np.int64) for n, d, _ in _TOTALS}
        out["games"], out["len_sum"] = int(out["games"]), int(out["len_sum"])
        out["per_env"] = per_env
        return out


# ---- seating ----------------------------------------------------------------------------------------------------------------
def balanced_seating(num_envs, num_learners, num_entrants):
    """int64 [num_envs, num_learners]: the entrant of env b, column l.  The envs cycle through all ordered selections of L
    entrants out of E in lexicographic order - without repetition when E >= L; when E < L, every assignment of the L columns
    that uses each entrant at least once.  Over one period every entrant sits in every column equally often."""
    B, L, E = _int(num_envs, "num_envs", 0), _int(num_learners, "num_learners", 1, MAX_LEARNERS), _int(num_entrants, "num_entrants", 1)
    if E >= L:
        sel = itertools.permutations(range(E), L)
    else:
        sel = (s for s in itertools.product(range(E), repeat=L) if len(set(s)) == E)
    period = list(itertools.islice(sel, B)) if B else []      # a period longer than the batch is never walked to its end
    table = np.empty((B, L), dtype=np.int64)
    for b in range(B):
        table[b] = period[b % len(period)]
    return table


def seating_period(num_learners, num_entrants):
    """How many envs one period of balanced_seating takes."""
    L, E = _int(num_learners, "num_learners", 1, MAX_LEARNERS), _int(num_entrants, "num_entrants", 1)
    if E >= L:
        return int(np.prod(np.arange(E - L + 1, E + 1), dtype=np.int64))
    return sum(1 for s in itertools.product(range(E), repeat=L) if len(set(s)) == E)


# ---- ratings ----------------------------------------------------------------------------------------------------------------
def expected_score(ra, rb):
    """The expected score of a player rated ra against one rated rb: the logistic curve of the Elo scale."""
    return 1.0 / (1.0 + 10.0 ** ((np.asarray(rb, dtype=np.float64) - np.asarray(ra, dtype=np.float64)) / 400.0))


def fit_elo(score, games, anchor=0, anchor_rating=1500.0, prior_draws=1.0, max_iter=200000):
    """Ratings [E] on the Elo scale from score[i, j] (what i scored against j: a win 1, a tie 1/2) and games[i, j] (how many
    they played, symmetric); the diagonals are ignored.  The Bradley-Terry maximum-likelihood strengths by minorise-maximise,
    p_i <- W_i / sum_j n_ij / (p_i + p_j), with prior_draws virtual drawn games between every pair, so the fit is connected
    and finite whatever was played; numpy float64 until max |d log p| < 1e-10.  The order in which games finished plays no
    part.  Ratings are 400 log10 p, shifted so that entrant `anchor` sits at anchor_rating."""
    s, g = np.array(score, dtype=np.float64), np.array(games, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != s.shape[1] or g.shape != s.shape:
        raise ValueError(f"score {s.shape} and games {g.shape} must be square matrices of one size")
    E = s.shape[0]
    if not 0 <= anchor < E:
        raise ValueError(f"anchor {anchor} outside [0, {E})")
    if prior_draws < 0 or not np.isfinite(prior_draws):
        raise ValueError(f"prior_draws {prior_draws} must be finite and >= 0")
    np.fill_diagonal(s, 0.0)
    np.fill_diagonal(g, 0.0)
    if (s < 0).any() or (g < 0).any() or not np.allclose(g, g.T) or (s + s.T > g + 1e-9).any():
        raise ValueError("games must be symmetric and non-negative, and score[i, j] + score[j, i] at most games[i, j]")
    off = 1.0 - np.eye(E)
    n = g + prior_draws * off
    wins = s.sum(axis=1) + 0.5 * prior_draws * (E - 1)
    if E > 1 and ((wins <= 0).any() or (n.sum(axis=1) - wins <= 0).any()):
        raise ValueError("an entrant that scored nothing, or lost nothing, has no finite rating: use prior_draws > 0")
    logp = np.zeros(E)
    for it in range(max_iter + 1):
        if it == max_iter:
            raise RuntimeError(f"fit_elo: no convergence in {max_iter} iterations (entrants that never met, even indirectly: use prior_draws > 0)")
        p = np.exp(logp)
        denom = (n / (p[:, None] + p[None, :])).sum(axis=1)
        new = np.log(wins / denom) if E > 1 else np.zeros(1)
        new -= new.mean()                                   # the scale is free: keep the geometric mean at 1
        delta = np.abs(new - logp).max()
        logp = new
        if delta < 1e-10:
            break
    r = 400.0 * logp / np.log(10.0)
    return r - r[anchor] + anchor_rating


# ---- entrants ---------------------------------------------------------------------------------------------------------------
class _RandomPolicy:
    def __init__(self, seed, head=None):
        self.seed, self.head, self._calls, self._zeros = int(seed), head, 0, None

    def __call__(self, obs, mask):
        import torch
        if self.head is None:
            from .policy_head import MaskedCategoricalHead
            self.head = MaskedCategoricalHead(mask.device)
        if self._zeros is None or self._zeros.shape != mask.shape or self._zeros.device != mask.device:
            self._zeros = torch.zeros(mask.shape, dtype=torch.float32, device=mask.device)
        self._calls += 1                                     # one seed per call: a draw is keyed by (seed, row, action index)
        return self.head.sample(self._zeros, mask, seed=(self.seed << 32) + self._calls)[0]


class _TorchPolicy:
    def __init__(self, net, head=None, greedy=False, seed=0):
        self.net, self.head, self.greedy, self.seed, self._calls = net, head, bool(greedy), int(seed), 0

    def __call__(self, obs, mask):
        import torch
        if self.head is None:
            from .policy_head import MaskedCategoricalHead
            self.head = MaskedCategoricalHead(mask.device)
        with torch.no_grad():
            out = self.net(obs)
        logits = out[0] if isinstance(out, (tuple, list)) else out      # an actor-critic returns (logits, value)
        self._calls += 1
        return self.head.sample(logits.reshape(mask.shape), mask, seed=(self.seed << 32) + self._calls, greedy=self.greedy)[0]


def random_policy(seed, head=None):
    """An entrant that plays uniformly over its legal actions: MaskedCategoricalHead.sample on zero logits."""
    return _RandomPolicy(seed, head)


def torch_policy(net, head=None, greedy=False, seed=0):
    """An entrant that plays net(obs) - logits [n, 5 * H * W], or (logits, value) - through the masked head: sampled, or
    the legal argmax with greedy=True.  The net is called under no_grad and left in the mode it is in."""
    return _TorchPolicy(net, head, greedy, seed)


# ---- the arena --------------------------------------------------------------------------------------------------------------
class ArenaResult:
    """What Arena.results() returns.  entrants / columns: {"games", "win_rate", "elimination_rate", "mean_length",
    "mean_return"} -> float64 [E] / [L] (NaN where nothing was played).  score, games: float64 [E, E], what entrant i scored
    against j over the games they shared a board in, the diagonal zero.  totals: EpisodeTally.totals()."""

    def __init__(self, entrants, columns, score, games, totals, names=None):
        self.entrants, self.columns, self.score, self.games, self.totals = entrants, columns, score, games, totals
        self.names = list(names) if names is not None else [f"entrant {e}" for e in range(score.shape[0])]

    def ratings(self, **kw):
        """fit_elo of the score and game matrices (keyword arguments are fit_elo's)."""
        return fit_elo(self.score, self.games, **kw)

    def table(self, **kw):
        r = self.ratings(**kw)
        w = max(len(n) for n in self.names + ["entrant"])
        lines = [f"{'entrant':<{w}}  {'games':>8}  {'win':>6}  {'elim':>6}  {'length':>8}  {'return':>9}  {'rating':>7}"]
        e = self.entrants
        for k, n in enumerate(self.names):
            lines.append(f"{n:<{w}}  {int(e['games'][k]):>8}  {e['win_rate'][k]:>6.3f}  {e['elimination_rate'][k]:>6.3f}  "
                         f"{e['mean_length'][k]:>8.1f}  {e['mean_return'][k]:>9.3f}  {r[k]:>7.0f}")
        return "\n".join(lines)


def _rates(games, wins, eliminated, len_sum, ret_sum):
    with np.errstate(divide="ignore", invalid="ignore"):
        g = games.astype(np.float64)
        return {"games": games, "win_rate": wins / g, "elimination_rate": eliminated / g, "mean_length": len_sum / g, "mean_return": ret_sum / g}


def reduce_through_seating(per_env, seating, num_entrants):
    """(entrants, columns, score [E, E], games [E, E]) of EpisodeTally.totals()["per_env"] under a seating [B, L]: host numpy.
    Pairs of columns seated with the same entrant land on the diagonal, which is then cleared."""
    seat = np.asarray(seating, dtype=np.int64)
    B, L = seat.shape
    E = int(num_entrants)
    games_bl = np.broadcast_to(per_env["games"].astype(np.int64)[:, None], (B, L))
    len_bl = np.broadcast_to(per_env["len_sum"][:, None], (B, L))
    by = lambda x, dt: np.bincount(seat.reshape(-1), weights=None if x is None else x.reshape(-1).astype(np.float64), minlength=E).astype(dt)
    entrants = _rates(by(games_bl, np.int64), by(per_env["wins"], np.int64), by(per_env["eliminated"], np.int64), by(len_bl, np.int64),
                      by(per_env["ret_sum"], np.float64))
    columns = _rates(games_bl.sum(axis=0), per_env["wins"].sum(axis=0, dtype=np.int64), per_env["eliminated"].sum(axis=0, dtype=np.int64),
                     len_bl.sum(axis=0), per_env["ret_sum"].sum(axis=0))
    score, games = np.zeros((E, E)), np.zeros((E, E))
    si, sj = np.broadcast_to(seat[:, :, None], (B, L, L)), np.broadcast_to(seat[:, None, :], (B, L, L))
    off = np.broadcast_to(~np.eye(L, dtype=bool), (B, L, L))
    np.add.at(score, (si[off], sj[off]), per_env["pair2"][off] * 0.5)
    np.add.at(games, (si[off], sj[off]), np.broadcast_to(per_env["games"][:, None, None], (B, L, L))[off].astype(np.float64))
    np.fill_diagonal(score, 0.0)
    np.fill_diagonal(games, 0.0)
    return entrants, columns, score, games


class Arena:
    def __init__(self, env, entrants, seating=None, head=None, names=None):
        """env: a GeneralsSelfPlayVecEnv(device_outputs=True).  entrants: callables policy(obs [n, 9, H, W], mask bool
        [n, 5 * H * W]) -> actions int64 [n], rows in a fixed order: the (env, column) pairs the entrant is seated at,
        ascending.  seating: int [B, L], the entrant of every column (None: balanced_seating), fixed for the arena's lifetime.
        head: a MaskedCategoricalHead that random_policy / torch_policy entrants built without one share.
        A step is one index_select pair and one scatter per entrant, env.step and the tally's launch: no host sync."""
        import torch
        self._t = t = torch
        if not getattr(env, "device_outputs", False):
            raise ValueError("Arena needs an env built with device_outputs=True: entrants act on the step's device tensors")
        self.env, self.entrants = env, list(entrants)
        B, L, E = env.num_envs, env.num_learners, len(self.entrants)
        if E < 1 or not all(callable(p) for p in self.entrants):
            raise ValueError("entrants must be a non-empty list of callables policy(obs, mask) -> actions")
        seat = balanced_seating(B, L, E) if seating is None else np.array(t.as_tensor(seating).cpu().numpy(), dtype=np.int64)
        if seat.shape != (B, L) or (seat < 0).any() or (seat >= E).any():
            raise ValueError(f"seating {seat.shape} must be [{B}, {L}] of entrant indices in [0, {E})")
        self.seating = seat
        self.names = list(names) if names is not None else None
        dev = env._dev
        flat = t.from_numpy(seat.reshape(-1)).to(dev)
        self._rows = [t.nonzero(flat == e).reshape(-1) for e in range(E)]          # built once: a sync here, none per step
        self._rows = [r if r.numel() else None for r in self._rows]
        for p, r in zip(self.entrants, self._rows):
            if hasattr(p, "bind"):
                p.bind(env, r)              # an entrant that needs to know where it sits (search.playout_policy)
        for p in self.entrants:
            if isinstance(p, (_RandomPolicy, _TorchPolicy)) and p.head is None:
                if head is None:
                    from .policy_head import MaskedCategoricalHead
                    head = MaskedCategoricalHead(dev)
                p.head = head
        self.head = head
        self.tally = EpisodeTally(B, L, env.player_ids, device=dev)
        self._actions = t.zeros(B * L, dtype=t.int64, device=dev)
        self._obs = self._mask = None
        self.steps = 0

    def reset(self, seed=None):
        """Re-deals every env and clears the tally."""
        self._obs, info = self.env.reset(seed)
        self._mask = info["valid_actions_mask"]
        self.tally.reset_all()
        self.steps = 0

    def step(self):
        """Every entrant acts on its rows, the env steps, the tally counts.  Returns what env.step returned."""
        if self._obs is None:
            self.reset()
        env = self.env
        n = env.num_envs * env.num_learners
        obs = self._obs.view(n, 9, env.board_height, env.board_width)
        mask = self._mask.view(n, env.single_action_n)
        single = len(self.entrants) == 1
        for policy, rows in zip(self.entrants, self._rows):
            if rows is None:
                continue
            if single:
                self._actions.copy_(policy(obs, mask).reshape(-1))
            else:
                self._actions.index_copy_(0, rows, policy(obs.index_select(0, rows), mask.index_select(0, rows)).reshape(-1))
        out = env.step(self._actions.view(env.num_envs, env.num_learners))
        self.tally.update_from_step(*out)
        self._obs, self._mask = out[0], out[4]["valid_actions_mask"]
        self.steps += 1
        return out

    def run(self, episodes_per_env=1, poll_every=32, max_steps=None):
        """Plays until every env has finished episodes_per_env games: the tally's cap is set to that number, so every env
        contributes exactly its first k games - stopping at a total count would over-represent the envs whose games are
        short.  games.min() is read every poll_every steps, the only host sync; max_steps ends the run regardless (the
        result then holds fewer games).  Returns the number of steps taken."""
        k = _int(episodes_per_env, "episodes_per_env", 1, 2 ** 31 - 1)
        poll = _int(poll_every, "poll_every", 1)
        limit = None if max_steps is None else _int(max_steps, "max_steps", 0)
        self.tally.games_cap = k
        taken = 0
        while limit is None or taken < limit:
            self.step()
            taken += 1
            if taken % poll == 0 and int(self.tally.games.min()) >= k:
                break
        return taken

    def results(self):
        """ArenaResult of everything counted so far (synchronises: one copy of the tally's tables)."""
        totals = self.tally.totals()
        entrants, columns, score, games = reduce_through_seating(totals["per_env"], self.seating, len(self.entrants))
        return ArenaResult(entrants, columns, score, games, totals, self.names)
