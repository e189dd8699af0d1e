"""numpy float64 restatement of gvec_traj_vtrace (include/generals_vec.h), written from the header's text with the
operations in the order the header gives them, and the direct sum of the paper's definition (Espeholt et al., IMPALA, 2018,
eq. 1) it is checked against."""
import numpy as np

import _gae_reference as R

VALID, TERMINAL, CUT = R.VALID, R.TERMINAL, R.CUT


def ratios(logp_target, logp_behaviour, rho_bar, c_bar):
    """(rho, c) float64 [T, N] from the two float32 log-probs."""
    w = np.exp(logp_target.astype(np.float64) - logp_behaviour.astype(np.float64))
    return np.minimum(rho_bar, w), np.minimum(c_bar, w)


def vtrace(reward, value, flags, logp_target, logp_behaviour, gamma, lam, rho_bar, c_bar):
    """reward float64 [T, N], value float32 [T + 1, N], flags uint8 [T, N], the log-probs float32 [T, N] ->
    (vs, pg, rho, M): vs / pg / rho float64 [T, N] before the one rounding to float32, and M float64 [N], per stream the
    maximum over its valid rows of rho * (|r| + |nv| + |nvs| + |V_t|) + |acc_next|: what a row's rounding errors scale with."""
    T, N = reward.shape
    v = value.astype(np.float64)
    rho, c = ratios(logp_target, logp_behaviour, rho_bar, c_bar)
    gl = np.float64(gamma) * np.float64(lam)
    vs, pg, ro = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N))
    M = np.zeros(N)
    acc, vs_next = np.zeros(N), v[T].copy()
    for t in range(T - 1, -1, -1):
        f = flags[t]
        valid, terminal, cut = (f & VALID) != 0, (f & TERMINAL) != 0, (f & CUT) != 0
        nv = np.where(terminal, 0.0, v[t + 1])
        nvs = np.where(terminal, 0.0, np.where(cut, v[t + 1], vs_next))
        delta = rho[t] * ((reward[t] + gamma * nv) - v[t])
        a = delta + (gl * c[t]) * np.where(cut, 0.0, acc)
        p = rho[t] * ((reward[t] + gamma * nvs) - v[t])
        m = rho[t] * (np.abs(reward[t]) + np.abs(nv) + np.abs(nvs) + np.abs(v[t])) + np.abs(acc)
        M = np.maximum(M, np.where(valid, m, 0.0))
        a = np.where(valid, a, 0.0)
        vs[t] = v[t] + a
        pg[t] = np.where(valid, p, 0.0)
        ro[t] = np.where(valid, rho[t], 0.0)
        acc, vs_next = a, vs[t]
    return vs, pg, ro, M


def runs(flags, t, n):
    """The rows t, t+1, ... the correction of row (t, n) sums over: up to the first CUT, or the last row before an invalid one."""
    T = flags.shape[0]
    k = t
    while True:
        yield k
        if (flags[k, n] & CUT) or k + 1 >= T or not (flags[k + 1, n] & VALID):
            return
        k += 1


def direct(reward, value, flags, logp_target, logp_behaviour, gamma, lam, rho_bar, c_bar):
    """vs_t = V_t + sum_k gamma^(k-t) (prod_{i<k} lam c_i) rho_k (r_k + gamma V_{k+1} - V_k), term by term.
    Returns (vs, scale): scale is the sum of the terms' magnitudes."""
    T, N = reward.shape
    v = value.astype(np.float64)
    rho, c = ratios(logp_target, logp_behaviour, rho_bar, c_bar)
    vs, scale = v[:-1].copy(), np.zeros((T, N))
    for t in range(T):
        for n in range(N):
            if not flags[t, n] & VALID:
                continue
            coef, terms = 1.0, []
            for k in runs(flags, t, n):
                nv = 0.0 if flags[k, n] & TERMINAL else v[k + 1, n]
                terms.append(coef * rho[k, n] * (reward[k, n] + gamma * nv - v[k, n]))
                coef *= gamma * lam * c[k, n]
            vs[t, n] = v[t, n] + sum(terms)
            scale[t, n] = abs(v[t, n]) + sum(abs(x) for x in terms)
    return vs, scale


def stats(pg32, rho32, flags):
    """{valid rows, sum pg, sum pg^2, sum rho} over the valid rows of the values AS STORED (float32), in float64."""
    ok = (flags & VALID) != 0
    x, r = pg32.astype(np.float64)[ok], rho32.astype(np.float64)[ok]
    return np.array([x.size, x.sum(), (x * x).sum(), r.sum()])


def random_logps(rng, T, N, spread=0.5):
    """logp_behaviour in [-3, 0], logp_target = logp_behaviour + spread * normal: float32 both."""
    lb = (-3.0 * rng.random((T, N))).astype(np.float32)
    lt = (lb + (spread * rng.standard_normal((T, N))).astype(np.float32)).astype(np.float32)
    return lt, lb
