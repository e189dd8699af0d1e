"""Flat Monte Carlo search on the device: what happens if this seat plays move a here?  (include/generals_vec.h "flat Monte
Carlo search")

    env = GeneralsSelfPlayVecEnv(4096, max_players=2, device_outputs=True)
    search = PlayoutSearch(env, candidates=8, replicas=4, depth=8)
    obs, info = env.reset()
    mask = info["valid_actions_mask"].view(-1, env.single_action_n)
    actions, found = search.act(mask, logits=net(obs.flatten(0, 1)), seed=step)   # one launch: n * 8 * 4 playouts of 8 turns
    target = search.policy_target(found["candidates"], found["q"], found["valid"])   # the AlphaZero-style policy target
    arena = Arena(env, [playout_policy(search), random_policy(seed=1)])           # ... or a baseline to measure against

One HIP launch per evaluation (gvec_search_playouts: one wavefront per playout; the roots are read only and 32 bytes come
back per playout); proposing the candidates and reducing the terms are a handful of torch calls on [n, K]-sized tensors.
The playouts see the true state, not the seat's fogged view: a baseline and a teacher, not a fair fogged player.

HalvingSearch spends the same playouts by sequential halving over Gumbel-top-m candidates (one gvec_search_halve launch
between two playout launches) and gives a policy target over every legal action from completed Q values
(gvec_search_improved_policy): include/generals_vec.h "sequential-halving search", DESIGN.md section 4.22.
"""
import ctypes as C

import numpy as np

from ._lib import SEARCH_NONE, SEARCH_PASS, SEARCH_TERMS, SearchArgs, check

TERM_NAMES = ("valid", "turns", "alive", "won", "land", "army", "land_others", "army_others")   # terms[..., i]
T_VALID, T_TURNS, T_ALIVE, T_WON, T_LAND, T_ARMY, T_LAND_OTHERS, T_ARMY_OTHERS = range(SEARCH_TERMS)


def search_playouts_device(engine, num_roots, candidates_ptr, root_players_ptr, terms_ptr, num_candidates, replicas, depth, seed=0,
                           root_envs_ptr=None, bot_players=0, bot_random_permille=0):
    """gvec_search_playouts on device memory (VecEngine.search_playouts_device): pointers are ints or None; enqueued on the
    engine's stream, not synchronised.  With bot_players (a seat mask) or bot_random_permille set: gvec_search_playouts_bot,
    whose playouts play the scripted opponent's rule on those seats."""
    a = SearchArgs(num_roots=int(num_roots), num_candidates=int(num_candidates), replicas=int(replicas), depth=int(depth),
                   root_envs=root_envs_ptr, root_players=root_players_ptr, candidates=candidates_ptr, seed=int(seed) & (2 ** 64 - 1),
                   terms=terms_ptr)
    if not bot_players and not bot_random_permille:
        check(engine.L.gvec_search_playouts(engine.h, C.byref(a)), "gvec_search_playouts")
        return
    if not 0 <= int(bot_players) < 2 ** 32:
        raise ValueError(f"bot_players must be a mask of seats below 32, not {bot_players!r}")
    check(engine.L.gvec_search_playouts_bot(engine.h, C.byref(a), int(bot_players), int(bot_random_permille)), "gvec_search_playouts_bot")


def _terms_tensor(terms):
    import torch
    if not isinstance(terms, torch.Tensor) or terms.dtype != torch.int32 or terms.dim() < 1 or terms.shape[-1] != SEARCH_TERMS:
        raise ValueError(f"terms must be an int32 tensor [..., {SEARCH_TERMS}], not "
                         f"{tuple(terms.shape) if isinstance(terms, torch.Tensor) else type(terms).__name__}")
    return terms


class PlayoutScore:
    """The value of one playout row, float64: `win` if the seat won, `loss` if it is not alive, else
    land * land / (land + land_others) + army * army / (army + army_others) - (land + army) / 2 with the weights `land` and
    `army` (a ratio with a zero denominator counts as 0.5): 0 for an even position, in [-(land + army) / 2, (land + army) / 2]."""

    def __init__(self, win=1.0, loss=-1.0, land=0.5, army=0.5):
        self.win, self.loss, self.land, self.army = float(win), float(loss), float(land), float(army)
        if not all(np.isfinite(v) for v in (self.win, self.loss, self.land, self.army)):
            raise ValueError("PlayoutScore weights must be finite")

    def __call__(self, terms):
        """terms int32 [..., 8] -> float64 [...] (the value of an invalid row means nothing: PlayoutSearch.scores drops it)"""
        import torch
        t = _terms_tensor(terms).to(torch.float64)

        def ratio(mine, others):
            den = mine + others
            return torch.where(den != 0, mine / torch.where(den != 0, den, torch.ones_like(den)), torch.full_like(den, 0.5))

        shaped = (self.land * ratio(t[..., T_LAND], t[..., T_LAND_OTHERS]) + self.army * ratio(t[..., T_ARMY], t[..., T_ARMY_OTHERS])
                  - (self.land + self.army) / 2)
        out = torch.where(t[..., T_ALIVE] == 0, torch.full_like(shaped, self.loss), shaped)
        return torch.where(t[..., T_WON] != 0, torch.full_like(shaped, self.win), out)


def _uniform_keys(seed, n, A, device):
    """float64 [n, A] in [0, 1): a counter hash of (seed, row, action index) - the same keys on any device, whatever the
    batch is split into.  With no prior the Gumbel key -log(-log(u)) ranks the actions as u itself does."""
    import torch
    M = 0xFFFFFFFF
    r = torch.arange(n, dtype=torch.int64, device=device)[:, None]
    a = torch.arange(A, dtype=torch.int64, device=device)[None, :]
    s = int(seed) & (2 ** 64 - 1)
    x = ((s & M) ^ ((s >> 32) * 0x9E3779B1 & M)) + r * 0x85EBCA6B + a * 0xC2B2AE35
    for mul in (0x7FEB352D, 0x846CA68B):                    # two multiply-xorshift rounds on 32 bits, in int64 lanes
        x = x & M
        x = x ^ (x >> 16)
        x = (x * mul) & M
    x = x ^ (x >> 15)
    return (x & M).to(torch.float64) / 4294967296.0


class PlayoutSearch:
    def __init__(self, env_or_engine, candidates=8, replicas=4, depth=8, score=None, rollout="agent", bot_players=None,
                 bot_random_permille=0):
        """env_or_engine: a gym vector env (GeneralsVecEnv / GeneralsSelfPlayVecEnv with device_outputs=True; rows are its
        (env, learner column) pairs) or a VecEngine (rows are (env, seat) pairs the caller names).  candidates K, replicas R
        and depth D >= 1: every evaluated row costs K * R playouts of at most D turns.
        rollout: "agent" - every seat of a playout plays the random agent (gvec_search_playouts) - or "bot": the seats of
        bot_players (seat ids or a bit mask; None: every seat) play the scripted opponent's rule in every playout turn, each
        with probability bot_random_permille / 1000 the agent's move instead (gvec_search_playouts_bot).  The searched seat's
        candidate is played on the first turn either way."""
        for name, v in (("candidates", candidates), ("replicas", replicas), ("depth", depth)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an int >= 1, not {v!r}")
        if rollout not in ("agent", "bot"):
            raise ValueError(f"rollout must be 'agent' or 'bot', not {rollout!r}")
        if isinstance(bot_random_permille, bool) or not isinstance(bot_random_permille, (int, np.integer)) \
                or not 0 <= bot_random_permille <= 1000:
            raise ValueError(f"bot_random_permille must be an int in [0, 1000], not {bot_random_permille!r}")
        if rollout == "agent" and (bot_players is not None or bot_random_permille != 0):
            raise ValueError("bot_players and bot_random_permille need rollout='bot'")
        self.K, self.R, self.D = int(candidates), int(replicas), int(depth)
        self.score = PlayoutScore() if score is None else score
        self.env = env_or_engine if hasattr(env_or_engine, "engine") else None
        self.engine = env_or_engine.engine if self.env is not None else env_or_engine
        e = self.engine
        self.W, self.H, self.num_actions = int(e.max_w), int(e.max_h), 5 * int(e.max_w) * int(e.max_h)
        self._ids = None
        self.rollout, self.bot_random_permille = rollout, int(bot_random_permille)
        self.bot_players = 0 if rollout == "agent" else self._seat_mask(bot_players, int(e.max_p))

    @staticmethod
    def _seat_mask(players, max_p):
        """the bit mask of seats below max_p from None (all of them), an int mask or an iterable of seat ids"""
        if players is None:
            return (1 << max_p) - 1
        if isinstance(players, (int, np.integer)) and not isinstance(players, bool):
            mask = int(players)
        else:
            mask = 0
            for p in players:
                if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= p < max_p:
                    raise ValueError(f"seat {p!r} is not an int below max_players = {max_p}")
                mask |= 1 << int(p)
        if not 0 <= mask < (1 << max_p):
            raise ValueError(f"bot_players {mask:#x} names a seat at or above max_players = {max_p}")
        return mask

    # ---- argument checks (before any library call) ---------------------------------------------------------------------
    def _device(self):
        import torch
        return torch.device("cuda", int(self.engine.device))

    def _check(self, t, name, dtype, shape, device=None):
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
        if t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
            raise ValueError(f"{name} must be {dtype}, not {t.dtype}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} {tuple(t.shape)} is not {tuple(shape)}")
        if device is not None and t.device != device:
            raise ValueError(f"{name} is on {t.device}, the engine on {device}")
        return t

    # ---- the launch ----------------------------------------------------------------------------------------------------
    def evaluate(self, env_ids, players, candidates, seed=0):
        """env_ids int32 [n] (None: envs 0..n-1), players int32 [n], candidates int64 [n, K]: contiguous CUDA tensors on the
        engine's device -> terms int32 [n, K, R, 8] (TERM_NAMES).  One launch on the engine's stream, no host sync."""
        import torch
        dev = self._device()
        cand = self._check(candidates, "candidates", torch.int64, None, dev)
        if cand.dim() != 2 or cand.shape[1] != self.K:
            raise ValueError(f"candidates {tuple(cand.shape)} is not [n, {self.K}]")
        n = int(cand.shape[0])
        self._check(players, "players", torch.int32, (n,), dev)
        if env_ids is not None:
            self._check(env_ids, "env_ids", torch.int32, (n,), dev)
        for name, t in (("candidates", cand), ("players", players), ("env_ids", env_ids)):
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if n * self.K * self.R >= 2 ** 31:
            raise ValueError(f"{n} * {self.K} * {self.R} playouts is not below 2^31")
        terms = torch.empty((n, self.K, self.R, SEARCH_TERMS), dtype=torch.int32, device=dev)
        if n == 0:                      # nothing to play (an empty tensor has no address to hand over)
            return terms
        bot = {} if self.rollout == "agent" else dict(bot_players=self.bot_players, bot_random_permille=self.bot_random_permille)
        self.engine.search_playouts_device(n, cand.data_ptr(), players.data_ptr(), terms.data_ptr(), self.K, self.R, self.D, seed,
                                           None if env_ids is None else env_ids.data_ptr(), **bot)
        return terms

    # ---- reductions (torch, on whatever device holds the terms) ---------------------------------------------------------
    def scores(self, terms):
        """terms int32 [n, K, R, 8] -> (q float32 [n, K]: the mean score over the valid replicas, 0 where there is none;
        valid bool [n, K]: some replica was played)"""
        import torch
        t = _terms_tensor(terms)
        if t.dim() != 4:
            raise ValueError(f"terms {tuple(t.shape)} is not [n, K, R, {SEARCH_TERMS}]")
        ok = t[..., T_VALID] != 0
        s = torch.where(ok, self.score(t), torch.zeros((), dtype=torch.float64, device=t.device))
        cnt = ok.sum(dim=-1)
        q = s.sum(dim=-1) / cnt.clamp(min=1).to(torch.float64)
        return q.to(torch.float32), cnt > 0

    def propose(self, mask, logits=None, seed=0):
        """mask bool / uint8 [n, 5 * H * W] (a row's valid-action mask), logits float [n, 5 * H * W] or None -> candidates
        int64 [n, K]: the K legal actions with the largest logits - with logits None: with the largest keys of a counter
        hash of (seed, row, action), a uniform draw without replacement - in that order, padded with GVEC_SEARCH_NONE where
        fewer than K are legal."""
        import torch
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 2 \
                or mask.shape[1] != self.num_actions:
            raise ValueError(f"mask must be a bool / uint8 tensor [n, {self.num_actions}]")
        legal = mask != 0
        n = int(legal.shape[0])
        if logits is not None:
            if not isinstance(logits, torch.Tensor) or not logits.is_floating_point() or tuple(logits.shape) != tuple(legal.shape):
                raise ValueError(f"logits must be a floating-point tensor {tuple(legal.shape)}")
            if logits.device != legal.device:
                raise ValueError(f"logits is on {logits.device}, mask on {legal.device}")
            keys = logits.detach().to(torch.float64)
        else:
            keys = _uniform_keys(seed, n, self.num_actions, legal.device)
        keys = torch.where(legal, keys, torch.full_like(keys, -float("inf")))
        k = min(self.K, self.num_actions)
        top = torch.topk(keys, k, dim=1)                      # [n, K]-sized output: not the hot path
        cand = torch.where(torch.isinf(top.values) & (top.values < 0), torch.full_like(top.indices, SEARCH_NONE), top.indices)
        if k < self.K:
            cand = torch.cat([cand, torch.full((n, self.K - k), SEARCH_NONE, dtype=torch.int64, device=cand.device)], dim=1)
        return cand.contiguous()

    def _rows_to_ids(self, n, rows):
        """(env_ids int32 [n], players int32 [n]) of the flat (env, column) rows of a gym env (None: all of them)"""
        import torch
        env = self.env
        if env is None:
            raise ValueError("act() on a bare VecEngine has no learner columns: use evaluate(env_ids, players, candidates)")
        ids = env._learner_ids() if hasattr(env, "_learner_ids") else list(getattr(env, "player_ids", [0]))
        L = len(ids)
        dev = self._device()
        if self._ids is None:
            flat = torch.arange(env.num_envs * L, device=dev)
            seats = torch.tensor(ids, dtype=torch.int32, device=dev)
            self._ids = ((flat // L).to(torch.int32), seats[flat % L].contiguous())
        if rows is None:
            if n != env.num_envs * L:
                raise ValueError(f"mask has {n} rows, the env {env.num_envs} x {L}: name the rows")
            return self._ids
        self._check(rows, "rows", (torch.int64, torch.int32), (n,), dev)
        r = rows.to(torch.int64)
        return self._ids[0].index_select(0, r), self._ids[1].index_select(0, r)

    def act(self, mask, logits=None, seed=0, rows=None):
        """mask [n, 5 * H * W] of the rows `rows` (flat (env, column) indices of the gym env, None: all, in order) ->
        (actions int64 [n], info): the candidate with the largest q among the valid ones; 0 for a row without one (the env
        refuses it, as it does for an eliminated learner).  info: candidates [n, K], q [n, K], valid [n, K], terms."""
        import torch
        dev = self._device()
        if isinstance(mask, torch.Tensor) and mask.device != dev:
            raise ValueError(f"mask is on {mask.device}, the engine on {dev}")
        cand = self.propose(mask, logits, seed)
        env_ids, players = self._rows_to_ids(int(cand.shape[0]), rows)
        terms = self.evaluate(env_ids, players, cand, seed)
        q, valid = self.scores(terms)
        best = torch.where(valid, q, torch.full_like(q, -float("inf"))).argmax(dim=1, keepdim=True)
        actions = torch.where(valid.any(dim=1), cand.gather(1, best).squeeze(1), torch.zeros((), dtype=torch.int64, device=dev))
        return actions, {"candidates": cand, "q": q, "valid": valid, "terms": terms}

    def policy_target(self, candidates, q, valid, temperature=1.0):
        """candidates int64 [n, K], q float [n, K], valid bool [n, K] -> float32 [n, 5 * H * W]: softmax(q / temperature)
        over a row's valid candidates at their action indices, zero elsewhere; all zeros for a row without one.  A valid
        candidate that is GVEC_SEARCH_PASS has no action index: it takes part in the softmax and its share is dropped."""
        import torch
        if not (isinstance(temperature, (int, float)) and temperature > 0 and np.isfinite(temperature)):
            raise ValueError(f"temperature must be a finite number > 0, not {temperature!r}")
        self._check(candidates, "candidates", torch.int64, None)
        if candidates.dim() != 2:
            raise ValueError(f"candidates {tuple(candidates.shape)} is not [n, K]")
        if not isinstance(q, torch.Tensor) or not q.is_floating_point() or tuple(q.shape) != tuple(candidates.shape):
            raise ValueError(f"q must be a floating-point tensor {tuple(candidates.shape)}")
        self._check(valid, "valid", torch.bool, tuple(candidates.shape))
        if q.device != candidates.device or valid.device != candidates.device:
            raise ValueError("candidates, q and valid must be on one device")
        z = torch.where(valid, q.to(torch.float64) / float(temperature), torch.full(q.shape, -float("inf"), dtype=torch.float64, device=q.device))
        top = z.max(dim=1, keepdim=True).values
        e = torch.where(valid, torch.exp(z - torch.where(torch.isinf(top), torch.zeros_like(top), top)), torch.zeros_like(z))
        den = e.sum(dim=1, keepdim=True)
        p = e / torch.where(den > 0, den, torch.ones_like(den))
        on_board = valid & (candidates >= 0) & (candidates < self.num_actions)
        out = torch.zeros((candidates.shape[0], self.num_actions), dtype=torch.float64, device=q.device)
        out.scatter_add_(1, torch.where(on_board, candidates, torch.zeros_like(candidates)), torch.where(on_board, p, torch.zeros_like(p)))
        return out.to(torch.float32)


def halving_schedule(candidates, budget):
    """[(K_r, R_r)] of a sequential-halving search over m = candidates slots: K_0 = m, K_{r+1} = ceil(K_r / 2), T = max(1,
    ceil(log2 m)) rounds - the last one's better half is the one survivor - and R_r = max(1, budget // (T * K_r)) playouts per
    column, so that every round spends about budget / T."""
    m, K, out = int(candidates), int(candidates), []
    T = max(1, (m - 1).bit_length())
    for _ in range(T):
        out.append((K, max(1, int(budget) // (T * K))))
        K = (K + 1) // 2
    return out


class HalvingSearch:
    """Sequential halving with Gumbel-top-m candidates and a completed-Q policy target: the root search of Danihelka et al.,
    "Policy improvement by planning with Gumbel" (ICLR 2022), on PlayoutSearch's playouts.

        search = HalvingSearch(env, candidates=16, budget=64, depth=8)       # 16 x 1, 8 x 2, 4 x 4, 2 x 8 playouts per row
        actions, found = search.act(mask, logits=logits, seed=step)          # per round: one playout launch, one gvec_search_halve
        target, v_mix = search.policy_target(logits, mask, found, value)     # softmax(logits + sigma(completed q)) over the legal set
    """

    def __init__(self, env_or_engine, candidates=16, budget=64, depth=8, score=None, rollout="agent", bot_players=None,
                 bot_random_permille=0, c_visit=50.0, c_scale=1.0):
        """candidates m in [1, 64] slots per row, budget >= 1 playouts per row to spread over the rounds (`schedule`; what is
        spent is `playouts_per_row`), depth, score (a PlayoutScore), rollout, bot_players, bot_random_permille as PlayoutSearch
        takes them; c_visit and c_scale: the paper's sigma(q) = (c_visit + max visits) * c_scale * q with q on [0, 1]."""
        from ._lib import SEARCH_MAX_SLOTS
        for name, v in (("candidates", candidates), ("budget", budget), ("depth", depth)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an int >= 1, not {v!r}")
        if candidates > SEARCH_MAX_SLOTS:
            raise ValueError(f"candidates must be at most {SEARCH_MAX_SLOTS}, not {candidates}")
        for name, v in (("c_visit", c_visit), ("c_scale", c_scale)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")
        if score is not None and not isinstance(score, PlayoutScore):
            raise ValueError(f"score must be a PlayoutScore (the kernel takes its four weights), not {type(score).__name__}")
        self.score = PlayoutScore() if score is None else score
        s = self.score
        half = (s.land + s.army) / 2
        self.q_lo = min(s.loss, -half)
        if not max(s.win, half) > self.q_lo:
            raise ValueError("the score has no range: max(win, (land + army) / 2) must exceed min(loss, -(land + army) / 2)")
        self.q_inv_range = 1.0 / (max(s.win, half) - self.q_lo)
        self.m, self.budget, self.D = int(candidates), int(budget), int(depth)
        self.c_visit, self.c_scale = float(c_visit), float(c_scale)
        self.schedule = halving_schedule(self.m, self.budget)
        self.playouts_per_row = sum(K * R for K, R in self.schedule)
        self._rounds = [PlayoutSearch(env_or_engine, candidates=K, replicas=R, depth=depth, score=s, rollout=rollout,
                                      bot_players=bot_players, bot_random_permille=bot_random_permille) for K, R in self.schedule]
        first = self._rounds[0]
        self.env, self.engine, self.num_actions = first.env, first.engine, first.num_actions
        self.rollout, self.bot_players, self.bot_random_permille = first.rollout, first.bot_players, first.bot_random_permille

    @staticmethod
    def round_seed(seed, r):
        """the playout seed of round r of a search called with `seed`"""
        return ((int(seed) & (2 ** 64 - 1)) + (r + 1) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)

    def _stream(self):
        return C.c_void_p(getattr(self.engine, "_stream", None) or 0)        # where the engine's own launches go

    def propose(self, mask, logits=None, seed=0):
        """mask bool / uint8 [n, 5 * H * W], logits float [n, 5 * H * W] or None (0 on every legal action) -> (candidates int64
        [n, m], prior_key float64 [n, m]): Gumbel-top-m, the m legal actions with the largest key = logit + g in that order,
        g = -log(-log u), u = (h + 0.5) / 2^32 with h the counter hash of (seed, row, action) that PlayoutSearch.propose
        draws from - a sample of m actions without replacement from softmax(logits).  Rows with fewer than m legal actions
        are padded with GVEC_SEARCH_NONE (prior_key -inf)."""
        import torch
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 2 \
                or mask.shape[1] != self.num_actions:
            raise ValueError(f"mask must be a bool / uint8 tensor [n, {self.num_actions}]")
        legal = mask != 0
        n = int(legal.shape[0])
        u = _uniform_keys(seed, n, self.num_actions, legal.device) + 0.5 / 4294967296.0      # exact: h has 32 bits
        keys = -torch.log(-torch.log(u))
        if logits is not None:
            if not isinstance(logits, torch.Tensor) or not logits.is_floating_point() or tuple(logits.shape) != tuple(legal.shape):
                raise ValueError(f"logits must be a floating-point tensor {tuple(legal.shape)}")
            if logits.device != legal.device:
                raise ValueError(f"logits is on {logits.device}, mask on {legal.device}")
            keys = logits.detach().to(torch.float64) + keys
        keys = torch.where(legal, keys, torch.full_like(keys, -float("inf")))
        k = min(self.m, self.num_actions)
        top = torch.topk(keys, k, dim=1)
        cand = torch.where(torch.isinf(top.values) & (top.values < 0), torch.full_like(top.indices, SEARCH_NONE), top.indices)
        prior = top.values
        if k < self.m:
            cand = torch.cat([cand, torch.full((n, self.m - k), SEARCH_NONE, dtype=torch.int64, device=cand.device)], dim=1)
            prior = torch.cat([prior, torch.full((n, self.m - k), -float("inf"), dtype=torch.float64, device=cand.device)], dim=1)
        return cand.contiguous(), prior.contiguous()

    def _halve_args(self, n, K, R, k_next, terms, slot, candidates, prior_key, total, count, next_slot, next_candidates):
        from ._lib import SearchHalveArgs
        s = self.score
        return SearchHalveArgs(n=n, m=self.m, k=K, replicas=R, k_next=k_next, reserved=0, terms=terms.data_ptr(),
                               slot=None if slot is None else slot.data_ptr(), candidates0=candidates.data_ptr(),
                               prior_key=prior_key.data_ptr(), win=s.win, loss=s.loss, land=s.land, army=s.army, q_lo=self.q_lo,
                               q_inv_range=self.q_inv_range, c_visit=self.c_visit, c_scale=self.c_scale, sum=total.data_ptr(),
                               count=count.data_ptr(), next_slot=next_slot.data_ptr(), next_candidates=next_candidates.data_ptr())

    def search(self, env_ids, players, candidates, prior_key, seed=0):
        """env_ids int32 [n] (None: envs 0..n-1), players int32 [n], candidates int64 [n, m], prior_key float64 [n, m]:
        contiguous CUDA tensors on the engine's device -> a dict: sum float64 [n, m] and count int32 [n, m] of every slot's
        playout scores, q float32 [n, m] (the mean, 0 where there is no count), valid bool [n, m] (count > 0), slot int32 [n]
        and action int64 [n] (the survivor: its slot and candidates[slot]) and found bool [n] (the survivor has a count).
        Per round one playout launch (PlayoutSearch.evaluate, under round_seed(seed, r)) and one gvec_search_halve, all on
        the engine's stream; no host sync."""
        import torch
        from ._lib import load
        first = self._rounds[0]
        dev = first._device()
        cand0 = first._check(candidates, "candidates", torch.int64, None, dev)
        if cand0.dim() != 2 or cand0.shape[1] != self.m:
            raise ValueError(f"candidates {tuple(cand0.shape)} is not [n, {self.m}]")
        n = int(cand0.shape[0])
        first._check(prior_key, "prior_key", torch.float64, (n, self.m), dev)
        if not prior_key.is_contiguous():
            raise ValueError("prior_key must be contiguous")
        total = torch.zeros((n, self.m), dtype=torch.float64, device=dev)
        count = torch.zeros((n, self.m), dtype=torch.int32, device=dev)
        cand, slot = cand0, None
        for r, (K, R) in enumerate(self.schedule):
            terms = self._rounds[r].evaluate(env_ids, players, cand, self.round_seed(seed, r))
            k_next = (K + 1) // 2
            next_slot = torch.empty((n, k_next), dtype=torch.int32, device=dev)
            next_cand = torch.empty((n, k_next), dtype=torch.int64, device=dev)
            if n:
                a = self._halve_args(n, K, R, k_next, terms, slot, cand0, prior_key, total, count, next_slot, next_cand)
                check(load().gvec_search_halve(dev.index, self._stream(), C.byref(a)), "gvec_search_halve")
            cand, slot = next_cand, next_slot
        valid = count > 0
        q = (total / count.clamp(min=1).to(torch.float64)).to(torch.float32)
        survivor = slot[:, 0]
        found = valid.gather(1, survivor.to(torch.int64)[:, None]).squeeze(1) if n else torch.zeros(0, dtype=torch.bool, device=dev)
        return {"sum": total, "count": count, "q": q, "valid": valid, "slot": survivor, "action": cand[:, 0], "found": found}

    def act(self, mask, logits=None, seed=0, rows=None):
        """PlayoutSearch.act's signature and row conventions -> (actions int64 [n], info): the surviving candidate; 0 for a
        row without one (the env refuses it).  info: candidates and prior_key [n, m], and everything search() returns."""
        import torch
        dev = self._rounds[0]._device()
        if isinstance(mask, torch.Tensor) and mask.device != dev:
            raise ValueError(f"mask is on {mask.device}, the engine on {dev}")
        cand, prior = self.propose(mask, logits, seed)
        env_ids, players = self._rounds[0]._rows_to_ids(int(cand.shape[0]), rows)
        info = self.search(env_ids, players, cand, prior, seed)
        info.update(candidates=cand, prior_key=prior)
        ok = info["found"] & (info["action"] >= 0)
        return torch.where(ok, info["action"], torch.zeros((), dtype=torch.int64, device=dev)), info

    def policy_target(self, logits, mask, info, value=None, out=None):
        """logits float32 [n, A] or None (uniform over the legal set), mask bool / uint8 [n, A], info with candidates, sum and
        count as act() returns them, value float32 [n] or None (the net's value in score units): contiguous CUDA tensors ->
        (target float32 [n, A], v_mix float32 [n]): gvec_search_improved_policy, softmax over the legal set of logits +
        sigma(completed q) - q the playout mean on the visited actions, v_mix elsewhere.  out: a contiguous float32 [n, A]
        tensor that takes the target instead of a new one (SelfPlayRolloutBuffer.policy_target_slot, flattened)."""
        import torch
        from ._lib import SearchPolicyArgs, load
        first = self._rounds[0]
        dev, A = first._device(), self.num_actions
        first._check(mask, "mask", (torch.bool, torch.uint8), None, dev)
        if mask.dim() != 2 or mask.shape[1] != A:
            raise ValueError(f"mask {tuple(mask.shape)} is not [n, {A}]")
        n = int(mask.shape[0])
        if logits is not None:
            first._check(logits, "logits", torch.float32, (n, A), dev)
        if value is not None:
            first._check(value, "value", torch.float32, (n,), dev)
        if not isinstance(info, dict) or not all(k in info for k in ("candidates", "sum", "count")):
            raise ValueError("info must hold candidates, sum and count, as act() returns them")
        first._check(info["candidates"], "info['candidates']", torch.int64, (n, self.m), dev)
        first._check(info["sum"], "info['sum']", torch.float64, (n, self.m), dev)
        first._check(info["count"], "info['count']", torch.int32, (n, self.m), dev)
        for name, t in (("mask", mask), ("logits", logits), ("value", value), ("info['candidates']", info["candidates"]),
                        ("info['sum']", info["sum"]), ("info['count']", info["count"])):
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if out is not None:
            first._check(out, "out", torch.float32, (n, A), dev)
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
        target = torch.empty((n, A), dtype=torch.float32, device=dev) if out is None else out
        v_mix = torch.empty((n,), dtype=torch.float32, device=dev)
        if n == 0:
            return target, v_mix
        legal = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        a = SearchPolicyArgs(n=n, num_actions=A, m=self.m, reserved=0, logits=None if logits is None else logits.data_ptr(),
                             mask=legal.data_ptr(), candidates0=info["candidates"].data_ptr(), sum=info["sum"].data_ptr(),
                             count=info["count"].data_ptr(), value=None if value is None else value.data_ptr(), q_lo=self.q_lo,
                             q_inv_range=self.q_inv_range, c_visit=self.c_visit, c_scale=self.c_scale, target=target.data_ptr(),
                             v_mix=v_mix.data_ptr())
        check(load().gvec_search_improved_policy(dev.index, self._stream(), C.byref(a)), "gvec_search_improved_policy")
        return target, v_mix


def search_expand_device(engine, num_roots, candidates_ptr, root_players_ptr, terms_ptr, num_candidates, replicas, depth, seed=0,
                         root_envs_ptr=None, bot_players=0, bot_random_permille=0, dst=None, child_envs_ptr=None, status_ptr=None):
    """gvec_search_expand on device memory: search_playouts_device's playouts, and replica 0's board after its first turn
    kept as env child_envs[i][k] (None: i * K + k) of the VecEngine `dst` (None: nothing is kept); status int32 [n][K]."""
    a = SearchArgs(num_roots=int(num_roots), num_candidates=int(num_candidates), replicas=int(replicas), depth=int(depth),
                   root_envs=root_envs_ptr, root_players=root_players_ptr, candidates=candidates_ptr, seed=int(seed) & (2 ** 64 - 1),
                   terms=terms_ptr)
    if not 0 <= int(bot_players) < 2 ** 32:
        raise ValueError(f"bot_players must be a mask of seats below 32, not {bot_players!r}")
    check(engine.L.gvec_search_expand(engine.h, C.byref(a), int(bot_players), int(bot_random_permille), None if dst is None else dst.h,
                                      child_envs_ptr, status_ptr), "gvec_search_expand")


class TreeSearch:
    """The search of Danihelka et al. with a tree below the root: sequential halving over the
    Gumbel-top-m root slots, the deterministic argmax(pi' - N / (1 + sum N)) rule at every node below, one node expanded per
    simulation, the values backed up along the path.  Every node's board stays resident in a scratch engine.

        search = TreeSearch(env, candidates=16, simulations=64, depth=8)     # 15 waves of 16, 8, 8, 4 ... columns per row
        actions, found = search.act(mask, logits=logits, seed=step)          # per wave: select, expand, observe, backup, copy
        target, v_mix = search.policy_target(logits, mask, found, value)
        arena = Arena(env, [playout_policy(search, net), bot_policy()])

    Round r of halving_schedule(candidates, simulations) runs R_r waves over its K_r surviving root slots; a wave is
    gvec_tree_select, gvec_search_expand (the parents' node envs as roots, under HalvingSearch.round_seed(seed, wave)),
    the priors of the new nodes (the gym observation of the dense frontier the children were stored in) and
    gvec_tree_backup, then gvec_copy_envs of the children into their node envs - whose range check is the one stream
    synchronisation a wave costs."""

    def __init__(self, env_or_engine, candidates=16, simulations=64, depth=8, replicas=1, children=None, prior_fn=None, value_weight=0.0,
                 score=None, rollout="agent", bot_players=None, bot_random_permille=0, c_visit=50.0, c_scale=1.0):
        """candidates m in [1, 64] root slots, simulations >= 1 expansions per row to spread over the rounds (what is spent is
        `simulations_per_row`), depth and replicas: every expansion is `replicas` playouts of at most `depth` turns from the
        parent; children C in [candidates, 64] slots per node (None: candidates); prior_fn(obs, mask) -> logits [rows, A] or
        (logits, value [rows] in score units) for the new nodes (None: logit 0 on every legal action); value_weight w in [0, 1]
        mixes that value into a node's estimate, (1 - w) * playout mean + w * value; the rest as HalvingSearch takes it."""
        from ._lib import SEARCH_MAX_SLOTS
        for name, v in (("simulations", simulations), ("replicas", replicas)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an int >= 1, not {v!r}")
        self._halving = HalvingSearch(env_or_engine, candidates=candidates, budget=simulations, depth=depth, score=score, rollout=rollout,
                                      bot_players=bot_players, bot_random_permille=bot_random_permille, c_visit=c_visit, c_scale=c_scale)
        if children is None:
            children = candidates
        if isinstance(children, bool) or not isinstance(children, (int, np.integer)) or not candidates <= children <= SEARCH_MAX_SLOTS:
            raise ValueError(f"children must be an int in [candidates = {candidates}, {SEARCH_MAX_SLOTS}], not {children!r}")
        if isinstance(value_weight, bool) or not isinstance(value_weight, (int, float, np.integer, np.floating)) \
                or not 0.0 <= value_weight <= 1.0:
            raise ValueError(f"value_weight must be a number in [0, 1], not {value_weight!r}")
        if prior_fn is not None and not callable(prior_fn):
            raise ValueError("prior_fn must be callable: prior_fn(obs, mask) -> logits or (logits, value)")
        if value_weight > 0 and prior_fn is None:
            raise ValueError("value_weight > 0 needs a prior_fn that returns (logits, value)")
        h = self._halving
        self.m, self.C, self.R, self.D = int(candidates), int(children), int(replicas), int(depth)
        self.simulations, self.prior_fn, self.value_weight = int(simulations), prior_fn, float(value_weight)
        self.score, self.q_lo, self.q_inv_range, self.c_visit, self.c_scale = h.score, h.q_lo, h.q_inv_range, h.c_visit, h.c_scale
        self.env, self.engine, self.num_actions = h.env, h.engine, h.num_actions
        self.rollout, self.bot_players, self.bot_random_permille = h.rollout, h.bot_players, h.bot_random_permille
        self.schedule = h.schedule                             # [(K_r, R_r)]: R_r waves of K_r columns
        self.waves = sum(R for _, R in self.schedule)
        self.simulations_per_row = sum(K * R for K, R in self.schedule)
        self.nodes = 1 + self.simulations_per_row
        self.playouts_per_row = self.simulations_per_row * self.R     # what HalvingSearch calls the same count
        self.max_turns = int(getattr(self.env, "max_turns", 500))
        self._slots = PlayoutSearch(env_or_engine, candidates=self.C, replicas=1, depth=1)      # propose() for a node's slots
        self._tree_engine = self._frontier = None
        self._rows = 0

    round_seed = staticmethod(HalvingSearch.round_seed)

    def propose(self, mask, logits=None, seed=0):
        """HalvingSearch.propose: the root's Gumbel-top-m slots and their prior keys"""
        return self._halving.propose(mask, logits, seed)

    # ---- the scratch engines ---------------------------------------------------------------------------------------------
    def _engines(self, n):
        """(tree engine of n * nodes envs - node j of row r is env j * n + r -, frontier of n * candidates envs): created
        on first use, again when a call brings more rows"""
        if self._tree_engine is None or n > self._rows:
            from .vec_engine import VecEngine
            e = self.engine
            for old in (self._tree_engine, self._frontier):
                if old is not None:
                    old.close()
            kw = dict(fog_of_war=e.fog_of_war, device=e.device, production=e.production, normal_growth_interval=e.normal_growth_interval,
                      stream=getattr(e, "_stream", None), lib=e.L)
            self._tree_engine = VecEngine(n * self.nodes, e.max_w, e.max_h, e.max_p, **kw)
            self._frontier = VecEngine(n * self.m, e.max_w, e.max_h, e.max_p, **kw)
            self._rows = n
        return self._tree_engine, self._frontier

    def close(self):
        for e in (self._tree_engine, self._frontier):
            if e is not None:
                e.close()
        self._tree_engine = self._frontier = None
        self._rows = 0

    def new_tree(self, n, device):
        """the nine node-major tensors of n empty trees (include/generals_vec.h gvec_tree)"""
        import torch
        from ._lib import TREE_NOT_EXPANDED
        N, Cn = self.nodes, self.C
        return {"child_action": torch.full((N, n, Cn), SEARCH_NONE, dtype=torch.int64, device=device),
                "child_logit": torch.zeros((N, n, Cn), dtype=torch.float32, device=device),
                "child_node": torch.full((N, n, Cn), TREE_NOT_EXPANDED, dtype=torch.int32, device=device),
                "child_count": torch.zeros((N, n, Cn), dtype=torch.int32, device=device),
                "child_sum": torch.zeros((N, n, Cn), dtype=torch.float64, device=device),
                "node_value": torch.zeros((N, n), dtype=torch.float64, device=device),
                "node_status": torch.zeros((N, n), dtype=torch.int32, device=device),
                "node_parent": torch.zeros((N, n), dtype=torch.int32, device=device),
                "node_slot": torch.zeros((N, n), dtype=torch.int32, device=device)}

    def _tree_struct(self, tree, n):
        from ._lib import Tree
        return Tree(n=n, nodes=self.nodes, num_slots=self.C, reserved=0, **{k: v.data_ptr() for k, v in tree.items()})

    # ---- the four steps of a wave (the GPU tests drive them one by one) ----------------------------------------------------
    def select(self, tree, slot):
        """slot int32 [n, K] -> (leaf_node, leaf_slot int32 [n, K], leaf_action int64 [n, K], leaf_depth int32 [n, K])"""
        import torch
        from ._lib import TreeSelectArgs, load
        n, K = int(slot.shape[0]), int(slot.shape[1])
        dev = slot.device
        out = [torch.empty((n, K), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64, torch.int32)]
        a = TreeSelectArgs(tree=self._tree_struct(tree, n), k=K, reserved=0, slot=slot.data_ptr(), q_lo=self.q_lo, q_inv_range=self.q_inv_range,
                           c_visit=self.c_visit, c_scale=self.c_scale, leaf_node=out[0].data_ptr(), leaf_slot=out[1].data_ptr(),
                           leaf_action=out[2].data_ptr(), leaf_depth=out[3].data_ptr())
        check(load().gvec_tree_select(dev.index, self._halving._stream(), C.byref(a)), "gvec_tree_select")
        return tuple(out)

    def expand(self, n, players, leaf_node, leaf_action, seed):
        """the playouts of one wave from the parents' node envs, the children stored in the frontier's envs r * K + c ->
        (terms int32 [n, K, R, 8], status int32 [n, K])"""
        import torch
        tree_e, frontier = self._engines(n)
        K, dev = int(leaf_node.shape[1]), leaf_node.device
        rows = torch.arange(n, dtype=torch.int64, device=dev)[:, None]
        root_envs = (leaf_node.to(torch.int64) * n + rows).to(torch.int32).reshape(-1).contiguous()
        seats = players.repeat_interleave(K).contiguous()
        cand = leaf_action.reshape(n * K, 1).contiguous()
        terms = torch.empty((n, K, self.R, SEARCH_TERMS), dtype=torch.int32, device=dev)
        status = torch.empty((n, K), dtype=torch.int32, device=dev)
        search_expand_device(tree_e, n * K, cand.data_ptr(), seats.data_ptr(), terms.data_ptr(), 1, self.R, self.D, seed, root_envs.data_ptr(),
                             self.bot_players, self.bot_random_permille, dst=frontier, status_ptr=status.data_ptr())
        return terms, status

    def observe(self, n, K, players, turn_count):
        """(obs float32 [n * K, 9, stride], mask uint8 [n * K, A]) of the frontier's first n * K envs, each from the seat of
        its row; turn_count int64 [n, K].  The frontier is observed once per seat that searches (gvec_gym_observe)."""
        import torch
        _, frontier = self._engines(n)
        dev, B, stride = players.device, frontier.B, int(frontier.stride)
        turns = torch.zeros((B,), dtype=torch.int64, device=dev)
        turns[:n * K] = turn_count.reshape(-1)
        if self.env is not None:
            seats = [int(p) for p in (self.env._learner_ids() if hasattr(self.env, "_learner_ids") else getattr(self.env, "player_ids", [0]))]
        else:
            seats = list(range(int(self.engine.max_p)))
        seat_of = players.repeat_interleave(K)
        obs = mask = None
        for p in sorted(set(seats)):
            o = torch.empty((B, 9, stride), dtype=torch.float32, device=dev)
            k = torch.empty((B, 5 * stride), dtype=torch.uint8, device=dev)
            check(frontier.L.gvec_gym_observe(frontier.h, p, turns.data_ptr(), self.max_turns, o.data_ptr(), k.data_ptr(), None, None, None),
                  "gvec_gym_observe")
            o, k = o[:n * K], k[:n * K]
            if obs is None:
                obs, mask = o, k
            else:
                mine = seat_of == p
                obs, mask = torch.where(mine[:, None, None], o, obs), torch.where(mine[:, None], k, mask)
        return obs, mask

    def priors(self, obs, mask, seed):
        """-> (slots int64 [rows, C], logits float32 [rows, C], value float32 [rows] or None): a new node's slots are its
        top-C legal actions by prior_fn's logits (PlayoutSearch.propose's hash order under `seed` without a prior_fn)"""
        import torch
        logits = value = None
        if self.prior_fn is not None:
            with torch.no_grad():
                out = self.prior_fn(obs, mask)
            logits, value = (out[0], out[1]) if isinstance(out, (tuple, list)) else (out, None)
            logits = logits.reshape(mask.shape).to(torch.float32)
            if value is not None:
                value = value.reshape(-1).to(torch.float32).contiguous()
        slots = self._slots.propose(mask, logits, seed)
        if logits is None:
            return slots, torch.zeros(slots.shape, dtype=torch.float32, device=slots.device), None
        got = logits.gather(1, slots.clamp(min=0))
        return slots, torch.where(slots >= 0, got, torch.zeros_like(got)).contiguous(), value

    def backup(self, tree, leaf_node, leaf_slot, new_node, terms, status, net_value=None):
        from ._lib import TreeBackupArgs, load
        n, K = int(leaf_node.shape[0]), int(leaf_node.shape[1])
        s = self.score
        use = net_value is not None and self.value_weight > 0
        a = TreeBackupArgs(tree=self._tree_struct(tree, n), k=K, replicas=self.R, leaf_node=leaf_node.data_ptr(), leaf_slot=leaf_slot.data_ptr(),
                           new_node=new_node.data_ptr(), terms=terms.data_ptr(), status=status.data_ptr(),
                           net_value=net_value.data_ptr() if use else None, value_weight=self.value_weight if use else 0.0,
                           win=s.win, loss=s.loss, land=s.land, army=s.army)
        check(load().gvec_tree_backup(leaf_node.device.index, self._halving._stream(), C.byref(a)), "gvec_tree_backup")

    def rank(self, tree, n, K, slot, prior_key, k_next):
        """the round's K columns ranked as gvec_search_halve ranks them from the root's sums and counts (all-zero terms add
        nothing) -> (next_slot int32 [n, k_next], next_candidates int64 [n, k_next])"""
        import torch
        from ._lib import SearchHalveArgs, load
        dev, s = slot.device, self.score
        zeros = torch.zeros((n, K, 1, SEARCH_TERMS), dtype=torch.int32, device=dev)
        next_slot = torch.empty((n, k_next), dtype=torch.int32, device=dev)
        next_cand = torch.empty((n, k_next), dtype=torch.int64, device=dev)
        a = SearchHalveArgs(n=n, m=self.C, k=K, replicas=1, k_next=k_next, reserved=0, terms=zeros.data_ptr(), slot=slot.data_ptr(),
                            candidates0=tree["child_action"][0].data_ptr(), prior_key=prior_key.data_ptr(), win=s.win, loss=s.loss,
                            land=s.land, army=s.army, q_lo=self.q_lo, q_inv_range=self.q_inv_range, c_visit=self.c_visit,
                            c_scale=self.c_scale, sum=tree["child_sum"][0].data_ptr(), count=tree["child_count"][0].data_ptr(),
                            next_slot=next_slot.data_ptr(), next_candidates=next_cand.data_ptr())
        check(load().gvec_search_halve(dev.index, self._halving._stream(), C.byref(a)), "gvec_search_halve")
        return next_slot, next_cand

    def start(self, env_ids, players, candidates, prior_key):
        """the tree of a new search: node 0 a copy of the root envs (which stay read-only), its slots the candidates ->
        (tree, prior key padded to [n, C])"""
        import torch
        n, dev = int(candidates.shape[0]), candidates.device
        tree_e, _ = self._engines(n)
        mix = getattr(self.engine, "agent_mix", None)             # the playouts draw under the root engine's mix, as
        if mix is not None and mix != getattr(tree_e, "agent_mix", None):   # HalvingSearch's do on the root engine itself
            tree_e.set_agent_mix(*mix)
        tree = self.new_tree(n, dev)
        tree["child_action"][0, :, :self.m] = candidates
        tree["node_status"][0] = 1
        key = torch.full((n, self.C), -float("inf"), dtype=torch.float64, device=dev)
        key[:, :self.m] = prior_key
        src = torch.arange(n, dtype=torch.int32, device=dev) if env_ids is None else env_ids
        tree_e.copy_envs(torch.arange(n, dtype=torch.int32, device=dev), src, n=n, src=self.engine)
        return tree, key

    def keep(self, n, new_node):
        """the wave's children, the frontier's envs r * K + c, into their node envs new_node * n + r (gvec_copy_envs)"""
        import torch
        tree_e, frontier = self._engines(n)
        K, dev = int(new_node.shape[1]), new_node.device
        rows = torch.arange(n, dtype=torch.int64, device=dev)[:, None]
        dst = (new_node.to(torch.int64) * n + rows).to(torch.int32).reshape(-1)
        tree_e.copy_envs(dst, torch.arange(n * K, dtype=torch.int32, device=dev), n=n * K, src=frontier)

    def search(self, env_ids, players, candidates, prior_key, seed=0, turn_count=None):
        """HalvingSearch.search's arguments (turn_count int64 [n]: the rows' gym turn counts, for the observations' turn
        plane; None: 0) -> what it returns, from the root's slots, plus nodes_used int32 [n] (the root included) and `tree`,
        the node-major tensors."""
        import torch
        first = self._halving._rounds[0]
        dev = first._device()
        cand0 = first._check(candidates, "candidates", torch.int64, None, dev)
        if cand0.dim() != 2 or cand0.shape[1] != self.m:
            raise ValueError(f"candidates {tuple(cand0.shape)} is not [n, {self.m}]")
        n = int(cand0.shape[0])
        first._check(prior_key, "prior_key", torch.float64, (n, self.m), dev)
        first._check(players, "players", torch.int32, (n,), dev)
        if env_ids is not None:
            first._check(env_ids, "env_ids", torch.int32, (n,), dev)
        if turn_count is not None:
            first._check(turn_count, "turn_count", torch.int64, (n,), dev)
        if n * self.nodes >= 2 ** 31 or n * self.m * self.R >= 2 ** 31:
            raise ValueError(f"{n} rows of {self.nodes} nodes do not fit a scratch engine")
        if n == 0:
            tree = self.new_tree(0, dev)
            empty = torch.zeros((0,), dtype=torch.int32, device=dev)
            return {"sum": tree["child_sum"][0], "count": tree["child_count"][0], "q": torch.zeros((0, self.m), dtype=torch.float32, device=dev),
                    "valid": torch.zeros((0, self.m), dtype=torch.bool, device=dev), "slot": empty, "action": empty.to(torch.int64),
                    "found": empty.to(torch.bool), "nodes_used": empty, "tree": tree}
        tree, key = self.start(env_ids, players, cand0, prior_key)
        turn0 = torch.zeros((n,), dtype=torch.int64, device=dev) if turn_count is None else turn_count
        slot = torch.arange(self.m, dtype=torch.int32, device=dev).repeat(n, 1).contiguous()
        cand, wave, used = cand0, 0, 1
        for K, R in self.schedule:
            for _ in range(R):
                wave_seed = self.round_seed(seed, wave)
                leaf_node, leaf_slot, leaf_action, leaf_depth = self.select(tree, slot)
                terms, status = self.expand(n, players, leaf_node, leaf_action, wave_seed)
                obs, mask = self.observe(n, K, players, turn0[:, None] + leaf_depth.to(torch.int64) + 1)
                slots, logits, value = self.priors(obs, mask, wave_seed)
                new_node = (used + torch.arange(K, dtype=torch.int32, device=dev)).repeat(n, 1).contiguous()
                at = (new_node.to(torch.int64) * n + torch.arange(n, dtype=torch.int64, device=dev)[:, None]).reshape(-1)
                tree["child_action"].view(-1, self.C)[at] = slots
                tree["child_logit"].view(-1, self.C)[at] = logits
                self.backup(tree, leaf_node, leaf_slot, new_node, terms, status, None if value is None else value.reshape(n, K).contiguous())
                self.keep(n, new_node)
                wave, used = wave + 1, used + K
            slot, cand = self.rank(tree, n, K, slot, key, (K + 1) // 2)
        total, count = tree["child_sum"][0, :, :self.m].contiguous(), tree["child_count"][0, :, :self.m].contiguous()
        valid = count > 0
        q = (total / count.clamp(min=1).to(torch.float64)).to(torch.float32)
        survivor = slot[:, 0]
        found = valid.gather(1, survivor.to(torch.int64)[:, None]).squeeze(1)
        return {"sum": total, "count": count, "q": q, "valid": valid, "slot": survivor, "action": cand[:, 0], "found": found,
                "nodes_used": (tree["node_status"] & 1).sum(dim=0).to(torch.int32), "tree": tree}

    def act(self, mask, logits=None, seed=0, rows=None):
        """HalvingSearch.act's signature and row conventions -> (actions int64 [n], info): the surviving root slot's action;
        0 for a row without one.  info: candidates and prior_key [n, m], and everything search() returns."""
        import torch
        first = self._halving._rounds[0]
        dev = first._device()
        if isinstance(mask, torch.Tensor) and mask.device != dev:
            raise ValueError(f"mask is on {mask.device}, the engine on {dev}")
        cand, prior = self.propose(mask, logits, seed)
        env_ids, players = first._rows_to_ids(int(cand.shape[0]), rows)
        turns = getattr(self.env, "_d_turn", None)
        turn_count = None if turns is None else turns.reshape(-1).to(torch.int64).index_select(0, env_ids.to(torch.int64))
        info = self.search(env_ids, players, cand, prior, seed, turn_count)
        info.update(candidates=cand, prior_key=prior)
        ok = info["found"] & (info["action"] >= 0)
        return torch.where(ok, info["action"], torch.zeros((), dtype=torch.int64, device=dev)), info

    def policy_target(self, logits, mask, info, value=None, out=None):
        """HalvingSearch.policy_target on the root's slots (gvec_search_improved_policy)"""
        return self._halving.policy_target(logits, mask, info, value, out)


class _PlayoutPolicy:
    """An Arena entrant: search.act on the rows it is seated at (Arena binds them), the prior from net or uniform."""

    def __init__(self, search, net=None, seed=0):
        self.search, self.net, self.seed, self._calls, self._rows, self._single = search, net, int(seed), 0, None, False

    def bind(self, env, rows):
        if env is not self.search.env:
            raise ValueError("playout_policy: the search was built on another env than the arena's")
        self._rows = rows
        self._single = rows is not None and int(rows.numel()) == env.num_envs * env.num_learners

    def __call__(self, obs, mask):
        import torch
        logits = None
        if self.net is not None:
            with torch.no_grad():
                out = self.net(obs)
            logits = (out[0] if isinstance(out, (tuple, list)) else out).reshape(mask.shape)
        self._calls += 1
        rows = None if self._single or self._rows is None else self._rows
        return self.search.act(mask, logits, seed=(self.seed << 32) + self._calls, rows=rows)[0]


def playout_policy(search, net=None, seed=0):
    """An Arena entrant that plays PlayoutSearch.act: the candidates are the top K legal actions by net(obs)'s logits
    (net returns logits [n, 5 * H * W] or (logits, value)), or a uniform draw of K legal actions when net is None."""
    return _PlayoutPolicy(search, net, seed)
