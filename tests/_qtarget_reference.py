"""numpy restatement of the masked Q targets (include/generals_vec.h "masked Q targets"): the legal
set of an observation, the scalar (Double) DQN target and the categorical (C51) target.  Written from the definitions, not
from the kernels: what tests/test_hip_qtarget.py holds the device against."""
import numpy as np

DIRS = ((0, -1), (1, 0), (0, 1), (-1, 0))          # up, right, down, left as (dx, dy)


def mask_from_observation(obs):
    """obs float32 [..., 9, H, W] -> bool [..., 5 * H * W]; action (y * W + x) * 5 + d."""
    obs = np.asarray(obs, np.float32)
    H, W = obs.shape[-2:]
    src = (obs[..., 1, :, :] == np.float32(0.5)) & (obs[..., 2, :, :] > np.float32(0.09))
    passable = obs[..., 4, :, :] == 0
    mask = np.zeros(src.shape + (5,), bool)
    for d, (dx, dy) in enumerate(DIRS):
        tgt = np.zeros(src.shape, bool)                # the neighbour in direction d is on the board and passable
        ys, yt = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
        xs, xt = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
        tgt[..., ys, xs] = passable[..., yt, xt]
        mask[..., d] = src & tgt
    mask[..., 4] = mask[..., :4].any(-1)
    return mask.reshape(src.shape[:-2] + (H * W * 5,))


def masked_argmax(values, mask):
    """The rule of both targets per row: over the legal i, the greatest value, the lowest index among equals; a NaN never
    wins; an all -inf legal set picks its lowest index.  values [rows, A], mask bool [rows, A] -> int64 [rows], -1 when
    nothing won."""
    values = np.asarray(values)
    cand = mask & ~np.isnan(values)
    v = np.where(cand, values, -np.inf)
    best = v.max(1) if v.shape[1] else np.full(v.shape[0], -np.inf)
    winners = cand & (v == best[:, None])
    idx = winners.argmax(1).astype(np.int64)
    return np.where(cand.any(1), idx, -1)


def _discount(discount, rows, dtype):
    d = np.asarray(discount, np.float32)               # the C ABI carries float32: gamma is rounded before it is used
    return np.broadcast_to(d, (rows,)).astype(dtype)


def q_target(next_obs, q_eval, reward, discount, done, q_select=None):
    """-> target float32 [rows], next_action int64 [rows], next_value float32 [rows]; float32 throughout: one rounded
    multiply, one rounded add."""
    q_eval = np.asarray(q_eval, np.float32)
    rows = q_eval.shape[0]
    mask = mask_from_observation(next_obs).reshape(rows, -1)
    a = masked_argmax(q_eval if q_select is None else np.asarray(q_select, np.float32), mask)
    boot = (a >= 0) & ~np.asarray(done).astype(bool)
    nv = np.where(boot, q_eval[np.arange(rows), np.maximum(a, 0)], np.float32(0)).astype(np.float32)
    reward = np.asarray(reward, np.float32)
    with np.errstate(all="ignore"):
        prod = (_discount(discount, rows, np.float32) * nv).astype(np.float32)
        target = np.where(boot, (reward + prod).astype(np.float32), reward).astype(np.float32)
    return target, a, nv


def support(num_atoms, v_min, v_max, dtype):
    v_min, v_max = dtype(np.float32(v_min)), dtype(np.float32(v_max))
    delta = (v_max - v_min) / dtype(num_atoms - 1)
    return (v_min + np.arange(num_atoms).astype(dtype) * delta).astype(dtype), v_min, v_max, delta


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def categorical_q(next_obs, logits, v_min, v_max, dtype=np.float64):
    """Q_i = sum_j softmax(logits[i])_j z_j at the legal actions, -inf elsewhere (their logits are not read).
    logits [rows, A, N] -> (Q [rows, A] of dtype, mask)."""
    rows, A, N = logits.shape
    mask = mask_from_observation(next_obs).reshape(rows, A)
    z = support(N, v_min, v_max, dtype)[0]
    q = np.full((rows, A), -np.inf, dtype)
    r, a = np.nonzero(mask)
    if len(r):
        q[r, a] = (_softmax(logits[r, a].astype(dtype)) * z).sum(-1)
    return q, mask


def project(p, reward, discount, v_min, v_max, dtype=np.float64):
    """m_k = sum_j p_j max(0, 1 - |b_j - k|), b_j = (clamp(reward + discount z_j) - v_min) / delta, summed in ascending j.
    p [rows, N], reward and discount [rows]."""
    rows, N = p.shape
    z, lo, hi, delta = support(N, v_min, v_max, dtype)
    tz = np.clip((reward[:, None] + (discount[:, None] * z[None, :]).astype(dtype)).astype(dtype), lo, hi)
    b = np.clip(((tz - lo) / delta).astype(dtype), dtype(0), dtype(N - 1))
    k = np.arange(N).astype(dtype)
    m = np.zeros((rows, N), dtype)
    for j in range(N):
        w = np.maximum(dtype(1) - np.abs(b[:, j:j + 1] - k[None, :]), dtype(0)).astype(dtype)
        m = (m + (p[:, j:j + 1] * w).astype(dtype)).astype(dtype)
    return m


def categorical_target(next_obs, logits_eval, reward, discount, done, v_min, v_max, logits_select=None, dtype=np.float64):
    """-> m dtype [rows, N], next_action int64 [rows] (-1 on done rows and where nothing won).  dtype=np.float32 keeps every
    intermediate in float32."""
    rows, A, N = logits_eval.shape
    q, mask = categorical_q(next_obs, logits_eval if logits_select is None else logits_select, v_min, v_max, dtype)
    a = masked_argmax(q, mask)
    done = np.asarray(done).astype(bool)
    a = np.where(done, -1, a)
    boot = a >= 0
    p = np.zeros((rows, N), dtype)
    p[:, 0] = 1                                        # the point mass: every b_j is the clamped reward's
    if boot.any():
        p[boot] = _softmax(logits_eval[np.nonzero(boot)[0], a[boot]].astype(dtype))
    reward = np.asarray(reward, np.float32).astype(dtype)
    disc = np.where(boot, _discount(discount, rows, dtype), dtype(0)).astype(dtype)
    return project(p, reward, disc, v_min, v_max, dtype), a
