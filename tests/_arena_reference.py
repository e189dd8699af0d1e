"""The episode tally of the match arena restated in numpy, sequential per env (include/generals_vec.h "match arena",
DESIGN.md section 4.18): what gvec_arena_update must reproduce bit for bit.  Plain loops, one env and one column at a time, in
the order the definition gives; `events` counts what happened, so that a test can first make sure its inputs exercised
every kind of episode ending."""
import numpy as np

SURVIVOR_KEY = 1 << 20

EVENTS = ("win", "same_step_deaths", "trunc_distinct_land", "trunc_equal_land", "term_and_trunc", "outside_winner",
          "reset_mid_episode", "capped")


class TallyReference:
    def __init__(self, num_envs, num_learners, player_ids=None, games_cap=0):
        B, L = num_envs, num_learners
        self.B, self.L, self.games_cap = B, L, games_cap
        self.player_ids = list(range(L)) if player_ids is None else list(player_ids)
        self.death = np.zeros((B, L), np.int32)
        self.ep_len = np.zeros(B, np.int32)
        self.ep_return = np.zeros((B, L), np.float64)
        self.games = np.zeros(B, np.int32)
        self.wins = np.zeros((B, L), np.int32)
        self.eliminated = np.zeros((B, L), np.int32)
        self.len_sum = np.zeros(B, np.int64)
        self.ret_sum = np.zeros((B, L), np.float64)
        self.pair2 = np.zeros((B, L, L), np.int32)
        self.events = {e: 0 for e in EVENTS}

    NAMES = ("death", "ep_len", "ep_return", "games", "wins", "eliminated", "len_sum", "ret_sum", "pair2")

    def state(self):
        return {n: getattr(self, n) for n in self.NAMES}

    def _clear(self, b):
        self.death[b] = 0
        self.ep_len[b] = 0
        self.ep_return[b] = 0.0

    def update(self, alive, terminated, truncated, winner, reward, reset=None, obs=None):
        """alive [B, L] or None, terminated / truncated / reset [B], winner [B], reward [B, L] float64, obs [B, L, 9, H, W]
        float32 or None"""
        L = self.L
        for b in range(self.B):
            if reset is not None and reset[b]:
                self.events["reset_mid_episode"] += int(self.ep_len[b] > 0)
                self._clear(b)
                continue
            self.ep_len[b] += 1
            for l in range(L):
                self.ep_return[b, l] = self.ep_return[b, l] + np.float64(reward[b, l])
                if self.death[b, l] == 0 and alive is not None and not alive[b, l]:
                    self.death[b, l] = self.ep_len[b]
            if not (terminated[b] or truncated[b]):
                continue
            if self.games_cap > 0 and self.games[b] == self.games_cap:
                self.events["capped"] += 1
                self._clear(b)
                continue
            count_land = obs is not None and bool(truncated[b]) and not bool(terminated[b])
            key = []
            for l in range(L):
                if self.death[b, l] != 0:
                    key.append(int(self.death[b, l]))
                else:
                    land = int((obs[b, l, 1] == np.float32(0.5)).sum()) if count_land else 0
                    key.append(SURVIVOR_KEY + land)
            for i in range(L):
                for j in range(L):
                    if i != j:
                        self.pair2[b, i, j] += 2 if key[i] > key[j] else (1 if key[i] == key[j] else 0)
            self.games[b] += 1
            self.len_sum[b] += int(self.ep_len[b])
            for l in range(L):
                self.wins[b, l] += int(int(winner[b]) == self.player_ids[l])
                self.eliminated[b, l] += int(self.death[b, l] != 0)
                self.ret_sum[b, l] = self.ret_sum[b, l] + self.ep_return[b, l]
            # what kind of ending this was
            dead = [k for k in key if k < SURVIVOR_KEY]
            lands = [k for k in key if k >= SURVIVOR_KEY]
            ev = self.events
            ev["win"] += int(int(winner[b]) in self.player_ids)
            ev["outside_winner"] += int(int(winner[b]) >= 0 and int(winner[b]) not in self.player_ids)
            ev["same_step_deaths"] += int(len(set(dead)) < len(dead))
            ev["term_and_trunc"] += int(bool(terminated[b]) and bool(truncated[b]))
            if count_land and len(lands) >= 2:
                ev["trunc_distinct_land"] += int(len(set(lands)) > 1)
                ev["trunc_equal_land"] += int(len(set(lands)) < len(lands))
            self._clear(b)


OBS_POOL = 4


def scripted_steps(B, L, HW, steps, seed, with_alive=True):
    """A seeded sequence of synthetic step outputs, no env behind them -> (steps, pool).  A step is a dict with alive [B, L]
    bool (None without with_alive), terminated, truncated, reset [B] bool, winner [B] int8, reward [B, L] float64 and obs, an
    index into pool (None without HW); pool holds OBS_POOL observations [B, L, 9, H, W] float32 for HW = (H, W), whose plane 1
    takes values in {0, 0.5, 1} and whose planes 0 and 2 are 0.5 everywhere (a kernel that read the wrong plane would count
    every tile).  Flags follow an env's protocol loosely (the step after an ending is a re-deal step) and every kind of ending
    is made on purpose with a small probability: two columns dying on one step, both flags at once, a winner that is no
    learner, equal and distinct land at a truncation, a re-deal in mid-episode.  Player ids are 0 .. L-1, so winner L stands
    for a player that is no learner."""
    rng = np.random.default_rng(seed)
    alive_now = np.ones((B, L), bool)
    pending = np.zeros(B, bool)
    out = []
    for k in range(steps):
        reset = pending.copy() | (rng.random(B) < 0.04)                 # a re-deal in mid-episode (force_reset)
        alive_now[reset] = True
        terminated, truncated = np.zeros(B, bool), np.zeros(B, bool)
        winner = np.full(B, -1, np.int8)
        for b in range(B):
            if reset[b]:
                continue
            u = rng.random()
            if with_alive and u < 0.08 and alive_now[b].sum() > 1:      # one column dies
                alive_now[b, rng.choice(np.flatnonzero(alive_now[b]))] = False
            elif with_alive and u < 0.14 and alive_now[b].sum() > 1:    # two die on the same step (all of them, when L == 2)
                alive_now[b, rng.choice(np.flatnonzero(alive_now[b]), 2, replace=False)] = False
            n = int(alive_now[b].sum())
            if n == 0:                                                  # every learner is out: somebody else won
                terminated[b], winner[b] = True, L
            elif n == 1 and L > 1:
                terminated[b], winner[b] = True, int(np.flatnonzero(alive_now[b])[0])
            elif L == 1 and rng.random() < 0.10:
                terminated[b], winner[b] = True, (0 if rng.random() < 0.5 else 1)
            if rng.random() < 0.15:
                truncated[b] = True                                     # on a terminated step too: termination wins
        pending = terminated | truncated
        out.append({"alive": alive_now.copy() if with_alive else None, "terminated": terminated, "truncated": truncated, "reset": reset,
                    "winner": winner, "reward": rng.normal(size=(B, L)).astype(np.float64), "obs": None if HW is None else k % OBS_POOL})
    pool = []
    if HW is not None:
        H, W = HW
        for _ in range(OBS_POOL):
            obs = np.full((B, L, 9, H, W), 0.5, np.float32)
            obs[:, :, 3:] = 0.0
            owner = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(B, L, H * W), p=[0.5, 0.3, 0.2])
            same = rng.random(B) < 0.5                                  # half of the envs: every column holds the same land
            owner[same] = owner[same][:, :1]
            obs[:, :, 1] = owner.reshape(B, L, H, W)
            pool.append(obs)
    return out, pool


def feed(ref, step, pool):
    """one scripted step into a TallyReference"""
    ref.update(**{**step, "obs": None if step["obs"] is None else pool[step["obs"]]})
