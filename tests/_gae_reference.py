"""numpy float64 restatement of the rollout kernels (gvec_traj_* in include/generals_vec.h): the flag rule of
gvec_traj_record, the GAE recurrence and statistics of gvec_traj_gae, the index list of gvec_traj_compact and the batch of
gvec_traj_gather.  Written from the header's text, with the operations in the order the header gives them."""
import numpy as np

VALID, TERMINAL, CUT = 1, 2, 4


def record_flags(reset, terminated, truncated, alive, alive_state, num_learners):
    """reset / terminated / truncated [B] and alive / alive_state [B * L] (0/1) -> (flags uint8 [B * L], new alive_state)."""
    rs, te, tr = (np.repeat(np.asarray(x).astype(bool), num_learners) for x in (reset, terminated, truncated))
    al, was = np.asarray(alive).astype(bool), np.asarray(alive_state).astype(bool)
    valid = ~rs & was
    terminal = valid & (te | ~al)
    cut = valid & (te | tr | ~al)
    return (valid * VALID + terminal * TERMINAL + cut * CUT).astype(np.uint8), al.astype(np.uint8)


def gae(reward, value, flags, gamma, lam):
    """reward float64 [T, N], value float32 [T + 1, N], flags uint8 [T, N] -> (adv, ret) float64 [T, N], before the one
    rounding to float32."""
    T, N = reward.shape
    value = value.astype(np.float64)
    adv, ret = np.zeros((T, N)), np.zeros((T, N))
    carry = np.zeros(N)
    gl = np.float64(gamma) * np.float64(lam)
    for t in range(T - 1, -1, -1):
        f = flags[t]
        valid, terminal, cut = (f & VALID) != 0, (f & TERMINAL) != 0, (f & CUT) != 0
        delta = (reward[t] + gamma * np.where(terminal, 0.0, value[t + 1])) - value[t]
        a = delta + gl * np.where(cut, 0.0, carry)
        a = np.where(valid, a, 0.0)
        adv[t] = a
        ret[t] = np.where(valid, a + value[t], value[t])
        carry = a
    return adv, ret


def stats(adv32, flags):
    """{valid rows, sum adv, sum adv^2, 0} over the valid rows of adv AS STORED (float32), in float64."""
    x = adv32.astype(np.float64)[(flags & VALID) != 0]
    return np.array([x.size, x.sum(), (x * x).sum(), 0.0])


def stats_abs(adv32, flags):
    """The sums of |x| the tolerance of the statistics is scaled by: (sum |adv|, sum adv^2)."""
    x = adv32.astype(np.float64)[(flags & VALID) != 0]
    return np.abs(x).sum(), (x * x).sum()


def normalise(adv32, st):
    """(adv - mean) / sqrt(var + 1e-8) in float64, from the statistics."""
    c = st[0]
    mean = st[1] / c if c > 0 else 0.0
    var = max(st[2] / c - mean * mean, 0.0) if c > 0 else 0.0
    return (adv32.astype(np.float64) - mean) / np.sqrt(var + 1e-8)


def compact(flags):
    return np.flatnonzero((flags.reshape(-1) & VALID) != 0).astype(np.int64)


def gather(pos, obs, mask, action, logp, value, ret, adv, flags, st=None):
    """obs [T + 1, N, F], mask [T + 1, N, K], the small stores [T(+1), N]; pos int64 [M].  Returns a dict; positions outside
    [0, T * N) give zero rows, and `rejected` counts them."""
    T, N = flags.shape
    ok = (pos >= 0) & (pos < T * N)
    p = np.where(ok, pos, 0)
    flat = lambda x: x.reshape((-1,) + x.shape[2:])
    zero = lambda x: np.where(ok.reshape((-1,) + (1,) * (x.ndim - 1)), x, np.zeros((), x.dtype))
    a = flat(adv)[p]
    out = {"obs": zero(flat(obs)[p]), "mask": zero(flat(mask)[p]), "action": zero(flat(action)[p]), "logp": zero(flat(logp)[p]),
           "value": zero(flat(value)[p]), "ret": zero(flat(ret)[p]),
           "adv": zero(a) if st is None else np.where(ok, normalise(a, st), 0.0),
           "weight": np.where(ok & ((flat(flags)[p] & VALID) != 0), 1.0, 0.0).astype(np.float32), "rejected": int((~ok).sum())}
    return out


def ulp_diff(a32, b32):
    """Distance in float32 units in the last place between two float32 arrays (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a32) - key(b32))


def random_rollout(rng, T, N, p_cut=0.05, p_term=0.5, p_invalid=0.05):
    """Random rewards / values and flag patterns that keep the flags' own invariants (TERMINAL implies CUT implies VALID)."""
    reward = rng.standard_normal((T, N))
    value = rng.standard_normal((T + 1, N)).astype(np.float32)
    valid = rng.random((T, N)) >= p_invalid
    cut = valid & (rng.random((T, N)) < p_cut)
    terminal = cut & (rng.random((T, N)) < p_term)
    flags = (valid * VALID + terminal * TERMINAL + cut * CUT).astype(np.uint8)
    return reward, value, flags
