"""The masked-categorical policy head restated in numpy (float64 from the float32 inputs, the RNG in exact uint32
arithmetic), written from include/generals_vec.h and DESIGN.md sections 4.12 / 6 - not from the kernels.

Also the shared inputs of the CPU and GPU tests: `make_rows` builds one batch that mixes every row kind;
`case_inputs`, SHAPES, SCALES and SAMPLING_SEED name the exact inputs and seed the sampling test draws on."""
import numpy as np

M32 = 0xFFFFFFFF


# ---- the counter RNG ----
def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def row_keys(seed, rows):
    """rows: int64 array of global row numbers (row_base + r)."""
    lo, hi = np.uint64(seed & M32), np.uint64((seed >> 32) & M32)
    base = (fmix32(lo ^ np.uint64(0x9E3779B9)) + hi * np.uint64(0x85EBCA77) + np.uint64(0x27D4EB2F)) & M32
    r = np.asarray(rows, np.int64).astype(np.uint64)
    rlo, rhi = r & M32, r >> np.uint64(32)
    k = fmix32((base + rlo * np.uint64(0xC2B2AE3D)) & M32)
    return fmix32(k ^ ((rhi * np.uint64(0x9E3779B1)) & M32) ^ np.uint64(0x68E31DA4))


def draws24(seed, rows, A):
    """k[r][i]: the top 24 bits of the hash of (seed, row, i)."""
    rk = row_keys(seed, rows)[:, None]
    i = np.arange(A, dtype=np.uint64)[None, :]
    return (fmix32((rk + i * np.uint64(0x9E3779B9)) & M32) >> np.uint64(8)).astype(np.int64)


def gumbel64(k):
    u = (k.astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def gumbel32(k):
    """The same draw carried out in float32: u rounded to float32 once, both logs and their negations in float32."""
    u = ((k.astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)
    u = np.minimum(u, np.float32(1.0 - 2.0 ** -24))          # k + 0.5 does not fit 24 bits at the very top: stay below 1
    return -np.log(-np.log(u, dtype=np.float32), dtype=np.float32)


# ---- the distribution ----
def legal_set(logits, mask):
    return (np.asarray(mask) != 0) & (np.asarray(logits) > -np.inf)


def forward(logits, mask):
    """(logp [R, A] float64 with -inf outside S, p, H [R], dead [R])."""
    l = np.asarray(logits, np.float32).astype(np.float64)
    S = legal_set(l, mask)
    dead = ~S.any(1)
    x = np.where(S, l, -np.inf)
    m = np.where(dead, 0.0, x.max(1, initial=-np.inf))
    e = np.where(S, np.exp(np.where(S, x - m[:, None], 0.0)), 0.0)
    Z = np.where(dead, 1.0, e.sum(1))
    logp = np.where(S, x - m[:, None] - np.log(Z)[:, None], -np.inf)
    p = np.where(S, np.exp(np.where(S, logp, 0.0)), 0.0)
    H = -(p * np.where(S, logp, 0.0)).sum(1)
    H[dead] = 0.0
    return logp, p, H, dead


def evaluate(logits, mask, action):
    """(logp of action [R], H [R], bad [R]): an action outside [0, A) or outside S has logp 0; bad marks those on live rows."""
    logp, _, H, dead = forward(logits, mask)
    R, A = logp.shape
    a = np.asarray(action, np.int64)
    inr = (a >= 0) & (a < A)
    ok = inr & legal_set(logits, mask)[np.arange(R), np.where(inr, a, 0)]
    lp = np.where(ok, logp[np.arange(R), np.where(ok, a, 0)], 0.0)
    return lp, H, ~ok & ~dead


def backward(logits, mask, action, grad_logp=None, grad_entropy=None):
    """grad_logits [R, A] float64: i in S: gl * (1[i == a] - p_i) - ge * p_i * (logp_i + H), otherwise 0."""
    logp, p, H, dead = forward(logits, mask)
    R, A = logp.shape
    S = legal_set(logits, mask)
    a = np.asarray(action, np.int64)
    inr = (a >= 0) & (a < A)
    ok = inr & S[np.arange(R), np.where(inr, a, 0)]
    gl = np.zeros(R) if grad_logp is None else np.asarray(grad_logp, np.float32).astype(np.float64)
    ge = np.zeros(R) if grad_entropy is None else np.asarray(grad_entropy, np.float32).astype(np.float64)
    gl = np.where(ok, gl, 0.0)
    onehot = np.zeros((R, A))
    onehot[np.arange(R)[ok], a[ok]] = 1.0
    g = gl[:, None] * (onehot - p) - ge[:, None] * p * (np.where(S, logp, 0.0) + H[:, None])
    return np.where(S, g, 0.0)


def sample_keys(logits, mask, seed, row_base=0, greedy=False, f32=False):
    """l_i + g_i on S, -inf elsewhere (greedy: l_i) - in float64, or with the draw and the add in float32."""
    l32 = np.asarray(logits, np.float32)
    S = legal_set(l32, mask)
    R, A = l32.shape
    if greedy:
        key = l32.astype(np.float64)
    else:
        k = draws24(seed, row_base + np.arange(R, dtype=np.int64), A)
        if f32:
            with np.errstate(invalid="ignore"):
                key = (np.where(S, l32, np.float32(0)) + gumbel32(k)).astype(np.float64)
        else:
            key = np.where(S, l32.astype(np.float64), 0.0) + gumbel64(k)
    return np.where(S, key, -np.inf)


def sample(logits, mask, seed, row_base=0, greedy=False, f32=False):
    """(action [R] - argmax of the keys, lowest index among equals, 0 on a dead row - and the keys)."""
    key = sample_keys(logits, mask, seed, row_base, greedy, f32)
    return np.where(np.isfinite(key).any(1), key.argmax(1), 0).astype(np.int64), key


def slack_ok(key64, picked):
    """The second route of the sampling check: the pick's float64 key is within 2^-20 * max(1, |best|) of the best."""
    R = key64.shape[0]
    best = key64.max(1)
    dead = ~np.isfinite(best)
    got = key64[np.arange(R), picked]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(got) & (best - got <= 2.0 ** -20 * np.maximum(1.0, np.abs(best)))
    return np.where(dead, picked == 0, ok)


# ---- shared inputs ----
ROW_KINDS = ["all", "sparse", "one", "none", "last", "last_chunk", "legal_all_ninf", "legal_some_ninf", "constant"]


def make_rows(rows, A, scale, seed):
    """(logits float32 [rows, A], mask uint8 [rows, A], kind [rows]): row r is of kind ROW_KINDS[r % 9]."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((rows, A)) * scale).astype(np.float32)
    mask = np.zeros((rows, A), np.uint8)
    kind = np.array([r % len(ROW_KINDS) for r in range(rows)])
    for r in range(rows):
        k = ROW_KINDS[kind[r]]
        if k == "all":
            mask[r] = 1
        elif k == "sparse":                                   # about 2 % legal, at least two
            n = min(A, max(2, int(round(0.02 * A))))
            mask[r, rng.choice(A, n, replace=False)] = rng.integers(1, 256, n)   # any nonzero byte is legal
        elif k == "one":
            mask[r, rng.integers(A)] = 1
        elif k == "none":
            pass
        elif k == "last":
            mask[r, A - 1] = 1
        elif k == "last_chunk":                               # only inside the last partial 64-chunk (the whole row when A < 64)
            lo = (A - 1) // 64 * 64
            mask[r, lo:] = rng.integers(0, 2, A - lo)
            mask[r, A - 1] = 1
        elif k == "legal_all_ninf":
            idx = rng.choice(A, max(1, A // 8), replace=False)
            mask[r, idx] = 1
            logits[r, idx] = -np.inf
        elif k == "legal_some_ninf":
            mask[r] = rng.integers(0, 2, A)
            mask[r, 0] = 1
            legal = np.flatnonzero(mask[r])
            logits[r, legal[::2]] = -np.inf
            if len(legal) == 1:                               # keep one finite legal logit where the row allows it
                logits[r, legal[0]] = np.float32(0.25)
        elif k == "constant":
            mask[r] = rng.integers(0, 2, A)
            mask[r, A // 2] = 1
            logits[r] = np.float32(rng.standard_normal() * scale)
    return logits, mask, kind


SAMPLING_SEED = 0x5EED0000BEEF
SHAPES = [(65, A) for A in (1, 5, 63, 64, 65, 320, 1125, 2000, 5120)] + [(R, 1125) for R in (1, 3, 1000)] + [(3, 5121)]
SCALES = (1.0, 30.0)


def case_inputs(rows, A, scale):
    """The batch of one (rows, A, scale) case - the same on every call."""
    return make_rows(rows, A, scale, seed=rows * 100003 + A * 7 + int(scale))
