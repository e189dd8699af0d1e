"""The fog-of-war memory planes (include/generals_vec.h "fog-of-war memory planes") restated in numpy: what the GPU tests
compare gvec_obs_memory_update with, bit for bit.  tests/test_memory_reference.py pins this file on hand-written planes.

A state is float32 [rows, 4, H, W]: seen, last_owner, last_army, age.  cap is a power of two, so min(k, cap) / cap is an
exact float32 and age * cap an exact integer whatever computes them: there is no tolerance anywhere."""
import numpy as np

SEEN, LAST_OWNER, LAST_ARMY, AGE = range(4)


def blank(rows, H, W):
    m = np.zeros((rows, 4, H, W), np.float32)
    m[:, AGE] = 1.0
    return m


def update(prev, obs, reset=None, cap=64, rows_per_flag=1):
    """One update.  prev [rows, 4, H, W] or None (every row blank); obs [rows, 9, H, W] float32; reset [rows / rows_per_flag]
    (any integer or bool dtype) or None.  Returns a new array; the arguments are left unchanged."""
    obs = np.asarray(obs)
    assert obs.dtype == np.float32 and obs.ndim == 4 and obs.shape[1] == 9
    rows, _, H, W = obs.shape
    base = blank(rows, H, W) if prev is None else np.array(prev, np.float32, copy=True)
    assert base.shape == (rows, 4, H, W)
    if reset is not None:
        flags = np.repeat(np.asarray(reset).reshape(-1) != 0, rows_per_flag)
        assert flags.shape == (rows,)
        base[flags] = blank(int(flags.sum()), H, W)
    vis = obs[:, 0] != 0
    capf = np.float32(cap)
    older = np.minimum(base[:, AGE] * capf + np.float32(1.0), capf) / capf
    out = np.empty_like(base)
    out[:, SEEN] = np.where(vis, np.float32(1.0), base[:, SEEN])
    # owner and army are copied, never computed with: through a uint32 view, so that any bit pattern survives
    for p in (LAST_OWNER, LAST_ARMY):
        out[:, p].view(np.uint32)[...] = np.where(vis, np.ascontiguousarray(obs[:, p]).view(np.uint32),
                                                  np.ascontiguousarray(base[:, p]).view(np.uint32))
    out[:, AGE] = np.where(vis, np.float32(0.0), np.where(base[:, SEEN] != 0, older, np.float32(1.0)))
    return out


def run(obs_seq, reset_seq=None, cap=64, rows_per_flag=1, prev=None):
    """The states after each observation of obs_seq [steps, rows, 9, H, W] -> [steps, rows, 4, H, W]; reset_seq[s] goes with
    obs_seq[s] (None, or None entries: no flags)."""
    out = []
    for s, obs in enumerate(obs_seq):
        prev = update(prev, obs, None if reset_seq is None else reset_seq[s], cap, rows_per_flag)
        out.append(prev)
    return np.stack(out)


def random_sequence(rng, steps, rows, H, W, rows_per_flag=1, p_visible=0.3, p_reset=0.1):
    """(obs [steps, rows, 9, H, W], reset uint8 [steps, rows / rows_per_flag]) as the GPU tests draw them: a tile is visible
    with probability p_visible per step; a visible tile's owner is one of 0, 0.5, 1.0 and its army log(a + 1) / 10, a hidden
    tile's are 0 as the env emits them; planes 3-8, which the update does not read, hold NaN."""
    vis = rng.random((steps, rows, H, W)) < p_visible
    obs = np.full((steps, rows, 9, H, W), np.nan, np.float32)
    obs[:, :, 0] = vis
    owner = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=vis.shape)
    army = (np.log(rng.integers(0, 2000, size=vis.shape).astype(np.float32) + np.float32(1.0)) / np.float32(10.0)).astype(np.float32)
    obs[:, :, 1] = np.where(vis, owner, np.float32(0.0))
    obs[:, :, 2] = np.where(vis, army, np.float32(0.0))
    reset = (rng.random((steps, rows // rows_per_flag)) < p_reset).astype(np.uint8)
    return obs, reset
