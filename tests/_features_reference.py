"""The strategic feature planes restated in numpy from their definition (include/generals_vec.h "strategic feature planes",
DESIGN.md section 4.13): a queue breadth-first search per plane, tile by tile.  Written from the definition, not from the
kernel - the kernel's bit-plane layout, level loop and bit-sliced distances appear nowhere here."""
from collections import deque

import numpy as np


NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def distances_one(obs):
    """obs float32 [9, H, W] -> (int64 [4, H, W] path lengths, -1 = impassable or unreachable; bool [H, W] front line)."""
    obs = np.asarray(obs, np.float32)
    assert obs.ndim == 3 and obs.shape[0] == 9
    H, W = obs.shape[1:]
    vis, mine, enemy = obs[0] != 0, obs[1] == np.float32(0.5), obs[1] == np.float32(1.0)
    mtn, city, gen = obs[4] != 0, obs[5] != 0, obs[6] != 0
    passable = ~mtn
    sources = [gen & mine, enemy, city & ~mine, ~vis & passable]
    dist = np.full((4, H, W), -1, np.int64)
    for p, src in enumerate(sources):
        d = dist[p]
        queue = deque()
        for y, x in zip(*np.nonzero(src & passable)):       # a source is an end of the path: it must be passable itself
            d[y, x] = 0
            queue.append((int(y), int(x)))
        while queue:
            y, x = queue.popleft()
            for dy, dx in NEIGHBOURS:
                ny, nx = y + dy, x + dx                      # (y, W - 1) -> (y, W) is off the board, never (y + 1, 0)
                if 0 <= ny < H and 0 <= nx < W and passable[ny, nx] and d[ny, nx] < 0:
                    d[ny, nx] = d[y, x] + 1
                    queue.append((ny, nx))
    front = np.zeros((H, W), bool)
    for y, x in zip(*np.nonzero(mine)):
        front[y, x] = any(0 <= y + dy < H and 0 <= x + dx < W and enemy[y + dy, x + dx] for dy, dx in NEIGHBOURS)
    return dist, front


def apply_cap(dist, front, cap):
    """(distances, front line) of distances_one -> float32 [5, H, W]: min(d, cap) / cap, 1.0 where there is no path."""
    assert cap >= 2 and cap & (cap - 1) == 0
    out = np.empty((5,) + front.shape, np.float32)
    out[:4] = np.where(dist < 0, np.float32(1.0), np.minimum(dist, cap).astype(np.float32) / np.float32(cap))
    out[4] = front
    return out


def features_one(obs, cap=64):
    """obs float32 [9, H, W] -> float32 [5, H, W]."""
    return apply_cap(*distances_one(obs), cap)


def features(obs, cap=64):
    """obs [..., 9, H, W] -> [..., 5, H, W]."""
    obs = np.asarray(obs, np.float32)
    lead = obs.shape[:-3]
    flat = obs.reshape((-1,) + obs.shape[-3:])
    out = np.stack([features_one(o, cap) for o in flat]) if len(flat) else np.empty((0, 5) + obs.shape[-2:], np.float32)
    return out.reshape(lead + (5,) + obs.shape[-2:])


def features_batch(obs, cap=64):
    """features() for the volume of the env tests (hundreds of observations per step): the same definition walked level by
    level over the whole batch with array shifts instead of tile by tile with a queue.  tests/test_features_reference.py pins
    it to features() on random boards; the queue search stays the reference the kernel cases are written against."""
    obs = np.asarray(obs, np.float32)
    lead, (H, W) = obs.shape[:-3], obs.shape[-2:]
    o = obs.reshape((-1, 9, H, W))
    vis, mine, enemy = o[:, 0] != 0, o[:, 1] == np.float32(0.5), o[:, 1] == np.float32(1.0)
    passable, city, gen = ~(o[:, 4] != 0), o[:, 5] != 0, o[:, 6] != 0

    def around(m):                                         # some 4-neighbour is in m: shifts that fall off the board, no wrap
        r = np.zeros_like(m)
        r[..., 1:, :] |= m[..., :-1, :]
        r[..., :-1, :] |= m[..., 1:, :]
        r[..., :, 1:] |= m[..., :, :-1]
        r[..., :, :-1] |= m[..., :, 1:]
        return r

    free = np.repeat(passable[:, None], 4, axis=1)
    frontier = np.stack([gen & mine, enemy, city & ~mine, ~vis], axis=1) & free
    dist = np.where(frontier, 0, -1).astype(np.int64)
    level = 0
    while frontier.any():
        level += 1
        frontier = around(frontier) & free & (dist < 0)
        dist[frontier] = level
    out = np.empty((len(o), 5, H, W), np.float32)
    out[:, :4] = np.where(dist < 0, np.float32(1.0), np.minimum(dist, cap).astype(np.float32) / np.float32(cap))
    out[:, 4] = mine & around(enemy)
    return out.reshape(lead + (5, H, W))


def max_depth(obs):
    """The deepest finite distance of planes 0-3 of one observation (uncapped)."""
    return int(distances_one(obs)[0].max())


def make_obs(H, W, mtn=None, mine=None, enemy=None, city=None, gen=None, vis=None):
    """A hand-written observation from boolean [H, W] maps (None: nowhere; vis None: everywhere)."""
    z = lambda m: np.zeros((H, W), bool) if m is None else np.asarray(m, bool).reshape(H, W)
    obs = np.zeros((9, H, W), np.float32)
    obs[0] = np.ones((H, W), bool) if vis is None else z(vis)
    obs[1] = np.where(z(mine), 0.5, np.where(z(enemy), 1.0, 0.0))
    obs[4], obs[5], obs[6] = z(mtn), z(city), z(gen)
    obs[3] = ~(z(mtn) | z(city) | z(gen))
    return obs


def serpentine(n, vis=True):
    """n x n: mountain rows 1, 3, 5, ..., the gap alternating right and left, own general at the origin.  The one
    path from the origin winds through every open row."""
    mtn = np.zeros((n, n), bool)
    for k, y in enumerate(range(1, n, 2)):
        mtn[y, :] = True
        mtn[y, n - 1 if k % 2 == 0 else 0] = False
    gen = np.zeros((n, n), bool)
    gen[0, 0] = True
    return make_obs(n, n, mtn=mtn, mine=gen, gen=gen, vis=np.full((n, n), vis))


def random_obs(rng, rows, H, W, mountain_share=0.2, visible_share=0.5):
    """Synthetic observations: type one-hot (mountain with `mountain_share`, a few cities and generals), visibility 50 %,
    owner 0 / 0.5 / 1.0 on visible non-mountain tiles; planes 2, 7 and 8 random (they are not read)."""
    obs = np.zeros((rows, 9, H, W), np.float32)
    u = rng.random((rows, H, W))
    mtn = u < mountain_share
    city = ~mtn & (u < mountain_share + 0.04)
    gen = ~mtn & ~city & (u < mountain_share + 0.06)
    vis = rng.random((rows, H, W)) < visible_share
    owner = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(rows, H, W), p=[0.6, 0.25, 0.15])
    for r in range(rows):                                  # every board shows its own general, as every observation of a game does
        y, x = int(rng.integers(H)), int(rng.integers(W))
        mtn[r, y, x], city[r, y, x], gen[r, y, x], vis[r, y, x], owner[r, y, x] = False, False, True, True, 0.5
    obs[:, 0] = vis
    obs[:, 1] = np.where(vis & ~mtn, owner, 0.0)
    obs[:, 2] = rng.random((rows, H, W)) * (obs[:, 1] != 0)
    obs[:, 3], obs[:, 4], obs[:, 5], obs[:, 6] = ~(mtn | city | gen), mtn, city, gen
    obs[:, 7] = rng.random((rows, H, W))
    obs[:, 8] = rng.random((rows, H, W))
    return obs
