"""Plain numpy restatement of the scripted opponent (gvec_bot_actions, DESIGN.md section 6 "Scripted opponent").

The rule reads one player's SEEN VIEW only (seen_view): a tile the player does not see carries no owner, army, type or list
entry - the arrays hold poison there and every read goes through the `seen` mask first.  bot_actions() applies the rule to
every selected seat of an OracleBatch-style state dict (read_state / game_state arrays) and mixes in the random agent's
moves the way the kernel does.  TEST INFRASTRUCTURE ONLY."""
from collections import deque

import numpy as np

TILE_NORMAL, TILE_GENERAL, TILE_CITY, TILE_MOUNTAIN = 0, 1, 2, 3
DIRS = ((0, -1), (1, 0), (0, 1), (-1, 0))     # up, right, down, left: the legal mask's order
UNSEEN_OWNER, UNSEEN_ARMY, UNSEEN_TYPE = -128, np.iinfo(np.int32).min, 255
M32 = 0xFFFFFFFF

# the exploration draw: independent of the random agent's own h1 / h2
MIX_C0, MIX_C1, MIX_C2, MIX_C3 = 0x5851F42D, 0x2C1B3C6D, 0x297A2D39, 0x1B873593


def amix(x):
    x &= M32
    x ^= x >> 15
    x = ((x & 0xFFFFFF) * 0xE8A54D) & M32
    x ^= x >> 13
    x = ((x & 0xFFFFFF) * 0xAA34A7) & M32
    x ^= x >> 15
    return x


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def env_key(seed, env):
    """the agent's per-env key (gvec_device.hpp env_key)"""
    lo, hi = seed & M32, (seed >> 32) & M32
    base = (fmix32(lo ^ 0x9E3779B9) + hi * 0x85EBCA77 + 0x27D4EB2F) & M32
    return fmix32(base + env * 0xC2B2AE3D)


def takes_random(seed, env, turn, player, random_permille):
    """True when slot (env, player) plays the random agent's move this turn."""
    ek = env_key(seed, env)
    h = amix(((ek ^ MIX_C0) + turn * MIX_C1 + player * MIX_C2) & M32)
    h = amix(h ^ MIX_C3)
    return (((h & 0xFFFF) * 1000) >> 16) < random_permille


class SeenView:
    """Player p's view of env e: seen[t]; owner / army / type / listed hold poison where the tile is not seen."""

    def __init__(self, st, e, p, fog):
        self.w, self.h = int(st["width"][e]), int(st["height"][e])
        n = self.w * self.h
        self.p, self.players = p, int(st["players"][e])
        self.done, self.alive = bool(st["done"][e]), bool(st["alive"][e][p]) if p < st["alive"].shape[1] else False
        self.fog = bool(fog)
        vis = st["visible"][e, :n].astype(np.int64)
        self.seen = np.ones(n, bool) if not fog else ((vis >> p) & 1).astype(bool)
        s = self.seen
        self.owner = np.where(s, st["owner"][e, :n].astype(np.int64), UNSEEN_OWNER)
        self.army = np.where(s, st["army"][e, :n].astype(np.int64), UNSEEN_ARMY)
        self.type = np.where(s, st["type"][e, :n].astype(np.int64), UNSEEN_TYPE)
        self.listed = np.where(s, st["listed"][e, :n].astype(np.int64), UNSEEN_OWNER)


def _bfs(v, targets):
    """distance to the target set through tiles that are not seen mountains (unseen tiles are passable); -1 = unreachable"""
    w, h = v.w, v.h
    passable = ~(v.seen & (v.type == TILE_MOUNTAIN))
    dist = np.full(w * h, -1, np.int64)
    q = deque()
    for t in np.flatnonzero(targets):
        dist[t] = 0
        q.append(int(t))
    while q:
        t = q.popleft()
        x, y = t % w, t // w
        for dx, dy in DIRS:
            nx, ny = x + dx, y + dy
            if 0 <= nx < w and 0 <= ny < h:
                u = ny * w + nx
                if dist[u] < 0 and passable[u]:
                    dist[u] = dist[t] + 1
                    q.append(u)
    return dist


def bot_move(v):
    """-> (from_x, from_y, to_x, to_y) or None for the view v (the rule of DESIGN.md section 6)."""
    p, w, h = v.p, v.w, v.h
    if v.done or p >= v.players or not v.alive:
        return None
    s_ok = v.seen & (v.owner == p) & (v.listed == p) & (v.army >= 2)   # the legal mask's sources, as far as p sees them
    sources = np.flatnonzero(s_ok)
    if len(sources) == 0:
        return None
    # ---- captures: highest tier, then the larger margin a - b, then the lower source tile, then the direction order
    best = None
    for s in sources:
        x, y = s % w, s // w
        a = int(v.army[s]) - 1
        for d, (dx, dy) in enumerate(DIRS):
            tx, ty = x + dx, y + dy
            if not (0 <= tx < w and 0 <= ty < h):
                continue
            t = ty * w + tx
            if not v.seen[t] or v.type[t] == TILE_MOUNTAIN or v.owner[t] == p:
                continue
            b = int(v.army[t])
            if not a > b:
                continue
            o, ty_ = int(v.owner[t]), int(v.type[t])
            tier = 4 if (ty_ == TILE_GENERAL and o >= 0) else 3 if ty_ == TILE_CITY else 2 if o >= 0 else 1
            key = (tier, a - b, -int(s), -d)
            if best is None or key > best[0]:
                best = (key, (x, y, tx, ty))
    if best is not None:
        return best[1]
    # ---- consolidation towards the target set
    enemy_gen = v.seen & (v.type == TILE_GENERAL) & (v.owner >= 0) & (v.owner != p)
    if enemy_gen.any():
        targets = enemy_gen
    else:
        normal = v.seen & (v.type == TILE_NORMAL) & (v.owner != p)
        if normal.any():
            targets = normal
        elif v.fog and (~v.seen).any():
            targets = ~v.seen
        else:
            return None
    dist = _bfs(v, targets)
    mine = v.seen & (v.owner == p)
    pick = None
    for s in sources:
        ds = int(dist[s])
        if ds < 2:
            continue
        x, y = s % w, s // w
        for dx, dy in DIRS:
            tx, ty = x + dx, y + dy
            if 0 <= tx < w and 0 <= ty < h:
                t = ty * w + tx
                if mine[t] and dist[t] == ds - 1:
                    key = (int(v.army[s]), -int(s))
                    if pick is None or key > pick[0]:
                        pick = (key, (x, y, tx, ty))
                    break
    return None if pick is None else pick[1]


def bot_actions(st, players, fog, seed=0, random_permille=0, agent=None, out=None, max_p=None):
    """The restatement of gvec_bot_actions over a state dict: players = bit mask of seats; agent = the random agent's
    [B][max_p] actions for the same state (needed when random_permille > 0); out = the array whose other slots are kept."""
    from _oracle import ACTION_DTYPE
    B = len(st["turn"])
    max_p = st["alive"].shape[1] if max_p is None else max_p
    acts = np.zeros((B, max_p), ACTION_DTYPE) if out is None else out
    for e in range(B):
        for p in range(max_p):
            if not (players >> p) & 1:
                continue
            if random_permille > 0 and takes_random(seed, e, int(st["turn"][e]), p, random_permille):
                acts[e, p] = agent[e, p]
                continue
            mv = bot_move(SeenView(st, e, p, fog))
            acts[e, p] = (0, 0, 0, 0, 0, (0, 0, 0)) if mv is None else (mv[0], mv[1], mv[2], mv[3], 1, (0, 0, 0))
    return acts
