"""The argument checks of the handle-free entry points (replay ring, PER, n-step, rollouts, policy head).

They run before anything touches a device, so they are pinned here without one: every rejection branch once, with its
return code and the part of gvec_last_error() that tells it from its neighbours, the order in which two failing checks are
reported, and the early GVEC_OK returns that need no device.  No call in this file passes every check: one that did would
launch a kernel on the fake pointers below.
"""
import ctypes as C

import pytest

import generalsreinforcementlearning_amd as g
from generalsreinforcementlearning_amd import _lib as lib

OK, INVALID = 0, -1
P = 256                 # a non-NULL "device pointer", aligned for every check; nothing dereferences it before the device check
ODD = P + 8             # not 16-byte aligned
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def L():
    return g.load()


def _args(cls, scalars, **over):
    """An args struct that passes every check: `scalars` as given, every pointer P; then `over` on top."""
    a = cls()
    for name, ctype in cls._fields_:
        if ctype is C.c_void_p:
            setattr(a, name, P)
    for k, v in {**scalars, **over}.items():
        setattr(a, k, v)
    return a


def _pointers(cls):
    return [name for name, ctype in cls._fields_ if ctype is C.c_void_p]


def _rejected(L, rc, text):
    assert rc == INVALID, rc
    msg = L.gvec_last_error()
    assert text.encode() in msg, msg


def _rejected_silently(L, call):
    """A branch that returns GVEC_E_INVALID without a message of its own: the last message stays."""
    assert L.gvec_per_tree_layout(0, None) == INVALID
    before = L.gvec_last_error()
    assert call() == INVALID
    assert L.gvec_last_error() == before


# ---- gvec_expand_experience_records ----------------------------------------------------------------------------------

def _layout(rd_extra=0, mp=2, fd=4, ns=2, stride=100):
    return (C.c_int32 * 8)(4 + 2 * mp + (8 * mp + 3) * fd + ns * 64 + rd_extra, mp, fd, ns, 2, stride, 0, 0)


def test_expand_experience_records(L):
    p = C.c_void_p(P)
    ok = _layout()
    for i in range(6):   # layout8, records, state, next_state, action_mask, meta
        ptrs = [ok, p, p, p, p, p]
        ptrs[i] = None
        _rejected_silently(L, lambda: L.gvec_expand_experience_records(0, None, ptrs[0], ptrs[1], 4, *ptrs[2:]))
    _rejected_silently(L, lambda: L.gvec_expand_experience_records(0, None, ok, p, -1, p, p, p, p))
    bad = [_layout(rd_extra=-1), _layout(rd_extra=4), _layout(mp=0), _layout(mp=9), _layout(fd=0), _layout(fd=33), _layout(ns=0),
           _layout(ns=17), _layout(stride=0), _layout(fd=32, ns=16, stride=1025), _layout(stride=129), _layout(ns=1, stride=65)]
    for lay in bad:
        _rejected(L, L.gvec_expand_experience_records(0, None, lay, p, 4, p, p, p, p), "gvec_expand_experience_records: layout {")
    _rejected(L, L.gvec_expand_experience_records(0, None, bad[0], p, 0, p, p, p, p), "layout {")   # the layout before n == 0
    assert L.gvec_expand_experience_records(0, None, ok, p, 0, p, p, p, p) == OK
    assert L.gvec_expand_experience_records(0, None, _layout(rd_extra=3), p, 0, p, p, p, p) == OK
    # the kernel moves a record's dwords and a tile's four mask bytes as one dword: 4-byte alignment, which the types do not give
    for off in (1, 2, 3):
        q = C.c_void_p(P + off)
        _rejected(L, L.gvec_expand_experience_records(0, None, ok, p, 4, p, p, q, p), "must be 4-byte aligned (action_mask is not)")
        _rejected(L, L.gvec_expand_experience_records(0, None, ok, q, 4, p, p, p, p), "must be 4-byte aligned (records is not)")
        _rejected(L, L.gvec_expand_experience_records(0, None, ok, p, 0, p, p, q, p), "action_mask is not")   # before n == 0
    assert L.gvec_expand_experience_records(0, None, ok, p, 0, p, p, C.c_void_p(P + 4), p) == OK               # any dword will do
    # order: NULL, layout, alignment
    _rejected_silently(L, lambda: L.gvec_expand_experience_records(0, None, ok, p, 4, None, p, C.c_void_p(P + 1), p))
    _rejected(L, L.gvec_expand_experience_records(0, None, bad[0], p, 4, p, p, C.c_void_p(P + 1), p), "layout {")


# ---- gvec_pool_collect -----------------------------------------------------------------------------------------------

COLLECT = dict(num_envs=4, obs_floats=8, max_steps_per_episode=10, capacity=16, result_capacity=4)


def test_pool_collect(L):
    call = lambda a: L.gvec_pool_collect(0, None, C.byref(a))
    _rejected_silently(L, lambda: L.gvec_pool_collect(0, None, None))
    for over in (dict(num_envs=0), dict(obs_floats=0), dict(max_steps_per_episode=0), dict(result_capacity=-1), dict(capacity=3)):
        _rejected(L, call(_args(lib.CollectArgs, COLLECT, **over)), "a step's transitions must fit: >= num_envs")
    optional = {"needs_reset"}
    for name in _pointers(lib.CollectArgs):
        a = _args(lib.CollectArgs, COLLECT, **{name: None})
        if name in optional:
            a.scratch = ODD   # goes on to the next check
            _rejected(L, call(a), "gvec_pool_collect: scratch must be 16-byte aligned")
        else:
            _rejected(L, call(a), "gvec_pool_collect: a required pointer is NULL (only needs_reset may be)")
    # the episode results are optional as a whole
    a = _args(lib.CollectArgs, COLLECT, result_capacity=0, result_reward=None, result_length=None, result_worker=None, scratch=ODD)
    _rejected(L, call(a), "gvec_pool_collect: scratch must be 16-byte aligned")
    _rejected(L, call(_args(lib.CollectArgs, COLLECT, scratch=ODD)), "gvec_pool_collect: scratch must be 16-byte aligned")
    # order: scalars, pointers, alignment
    _rejected(L, call(_args(lib.CollectArgs, COLLECT, num_envs=0, state=None, scratch=ODD)), "must fit")
    _rejected(L, call(_args(lib.CollectArgs, COLLECT, state=None, scratch=ODD)), "a required pointer is NULL")


# ---- prioritized replay ----------------------------------------------------------------------------------------------

PER_MAX = 1 << 36


def _per_calls(L):
    """Every gvec_per_* launch wrapper as f(tree, capacity), its own arguments valid."""
    return {
        "gvec_per_init": lambda t, c: L.gvec_per_init(0, None, t, c),
        "gvec_per_push": lambda t, c: L.gvec_per_push(0, None, t, c, P, P, 1),
        "gvec_per_update": lambda t, c: L.gvec_per_update(0, None, t, c, P, P, 4, 0.6, 1e-3),
        "gvec_per_sample": lambda t, c: L.gvec_per_sample(0, None, t, c, P, 4, 0.4, None, 1, P, P),
    }


def test_per_tree_checks(L):
    for fn, call in _per_calls(L).items():
        _rejected(L, call(None, 8), fn + ": tree is NULL")
        for cap in (0, -1, PER_MAX + 1):
            _rejected(L, call(P, cap), fn + ": capacity %d outside [1, 2^36]" % cap)
        _rejected(L, call(P + 128, 8), fn + ": tree must be 256-byte aligned")
        # order: NULL, capacity, alignment
        _rejected(L, call(None, 0), fn + ": tree is NULL")
        _rejected(L, call(P + 128, 0), fn + ": capacity 0 outside")


def test_per_tree_checks_come_first(L):
    _rejected(L, L.gvec_per_push(0, None, None, 8, None, None, 0), "gvec_per_push: tree is NULL")
    _rejected(L, L.gvec_per_update(0, None, P, 0, None, None, -1, -1.0, 0.0), "gvec_per_update: capacity 0 outside")
    _rejected(L, L.gvec_per_sample(0, None, P + 128, 8, None, 0, -1.0, None, 1, None, None), "gvec_per_sample: tree must be")


def test_per_push(L):
    text = "gvec_per_push: counters_before / counters_after NULL or max_count"
    _rejected(L, L.gvec_per_push(0, None, P, 8, None, P, 1), text)
    _rejected(L, L.gvec_per_push(0, None, P, 8, P, None, 1), text)
    _rejected(L, L.gvec_per_push(0, None, P, 8, P, P, 0), text + " 0 < 1")


def test_per_update(L):
    text = "gvec_per_update: n %d < 0, alpha"
    _rejected(L, L.gvec_per_update(0, None, P, 8, P, P, -1, 0.6, 1e-3), text % -1)
    for alpha, eps in ((-0.5, 1e-3), (NAN, 1e-3), (0.6, 0.0), (0.6, -1.0), (0.6, NAN)):
        _rejected(L, L.gvec_per_update(0, None, P, 8, P, P, 4, alpha, eps), text % 4)
    assert L.gvec_per_update(0, None, P, 8, None, None, 0, 0.0, 1e-3) == OK          # nothing to update: no device, no arrays
    _rejected(L, L.gvec_per_update(0, None, P, 8, None, None, 0, -1.0, 1e-3), text % 0)   # the scalars before n == 0
    _rejected(L, L.gvec_per_update(0, None, P, 8, None, P, 4, 0.6, 1e-3), "gvec_per_update: idx or td_error is NULL")
    _rejected(L, L.gvec_per_update(0, None, P, 8, P, None, 4, 0.6, 1e-3), "gvec_per_update: idx or td_error is NULL")


def test_per_sample(L):
    text = "gvec_per_sample: k %d < 1 or beta"
    _rejected(L, L.gvec_per_sample(0, None, P, 8, P, 0, 0.4, None, 1, P, P), text % 0)
    for beta in (-0.1, NAN):
        _rejected(L, L.gvec_per_sample(0, None, P, 8, P, 4, beta, None, 1, P, P), text % 4)
    for i in range(3):
        ptrs = [P, P, P]
        ptrs[i] = None
        _rejected(L, L.gvec_per_sample(0, None, P, 8, ptrs[0], 4, 0.4, None, 1, ptrs[1], ptrs[2]),
                  "gvec_per_sample: ring_counters, idx or weight is NULL")
    _rejected(L, L.gvec_per_sample(0, None, P, 8, None, 0, 0.4, None, 1, None, None), text % 0)   # the scalars before the pointers


def test_per_tree_layout_and_bytes(L):
    out = (C.c_int64 * 10)()
    text = "gvec_per_tree_layout: capacity %d outside [1, 2^36] or out is NULL"
    _rejected(L, L.gvec_per_tree_layout(8, None), text % 8)
    for cap in (0, -5, PER_MAX + 1):
        _rejected(L, L.gvec_per_tree_layout(cap, out), text % cap)
        assert L.gvec_per_tree_bytes(cap) == 0
    for cap in (1, 64, 65, 1000, PER_MAX):
        assert L.gvec_per_tree_layout(cap, out) == OK
        levels, total = out[0], out[1]
        assert 1 <= levels <= 6 and total > 0 and L.gvec_per_tree_bytes(cap) == 4 * total
        offs = list(out[2:3 + levels])
        assert offs == sorted(offs) and offs[0] >= lib.PER_HEADER_WORDS and offs[-1] < total
        assert all(o == 0 for o in out[3 + levels:])


# ---- n-step returns --------------------------------------------------------------------------------------------------

def test_nstep_link(L):
    call = lambda a, cb=P, succ=P, last=P: L.gvec_nstep_link(0, None, C.byref(a) if a is not None else None, cb, succ, last)
    good = lambda **over: _args(lib.CollectArgs, COLLECT, **over)
    text = "gvec_nstep_link: args, counters_before, ring_succ or nstep_last is NULL"
    _rejected(L, call(None), text)
    _rejected(L, call(good(), cb=None), text)
    _rejected(L, call(good(), succ=None), text)
    _rejected(L, call(good(), last=None), text)
    for over in (dict(capacity=0), dict(num_envs=0), dict(num_envs=17)):
        _rejected(L, call(good(**over)), "gvec_nstep_link: capacity %d < 1, or num_envs" % over.get("capacity", 16))
    for name in ("ring_counters", "scratch"):
        _rejected(L, call(good(**{name: None})), "gvec_nstep_link: a required pointer of args is NULL (ring_counters, scratch)")
    _rejected(L, call(good(scratch=ODD)), "gvec_nstep_link: scratch must be 16-byte aligned")
    # it reads nothing else of the collect args: the other pointers may be NULL
    others = {n: None for n in _pointers(lib.CollectArgs) if n not in ("ring_counters", "scratch")}
    _rejected(L, call(good(scratch=ODD, obs_floats=0, max_steps_per_episode=0, **others)), "scratch must be 16-byte aligned")
    # order: arguments, scalars, pointers of args, alignment
    _rejected(L, call(good(capacity=0, scratch=None), cb=None), text)
    _rejected(L, call(good(capacity=0, scratch=None)), "outside [1, capacity]")


NSTEP = dict(k=4, capacity=16, n_step=3, obs_floats=8, gamma=0.99)


def test_nstep_gather(L):
    call = lambda a: L.gvec_nstep_gather(0, None, C.byref(a))
    good = lambda **over: _args(lib.NstepGatherArgs, NSTEP, **over)
    _rejected(L, L.gvec_nstep_gather(0, None, None), "gvec_nstep_gather: args is NULL")
    for over in (dict(capacity=0), dict(k=-1), dict(k=(1 << 28) + 1), dict(n_step=0), dict(obs_floats=0)):
        _rejected(L, call(good(**over)), "gvec_nstep_gather: capacity %d < 1, k %d outside [0, 2^28]" % (over.get("capacity", 16), over.get("k", 4)))
    for gamma in (-0.1, INF, NAN):
        _rejected(L, call(good(gamma=gamma)), "must be finite and >= 0")
    _rejected(L, call(good(ring_succ=None)), "gvec_nstep_gather: ring_succ is NULL with n_step 3 > 1")
    everything = {n: None for n in _pointers(lib.NstepGatherArgs)}
    assert call(good(k=0, n_step=1, **everything)) == OK            # nothing to gather: no device, no arrays
    assert call(good(k=0, **{**everything, "ring_succ": P})) == OK
    _rejected(L, call(good(k=0, **everything)), "ring_succ is NULL with n_step")   # ... but the checks above k == 0 hold
    _rejected(L, call(good(k=0, gamma=-1.0)), "must be finite")
    for name in _pointers(lib.NstepGatherArgs):
        if name != "ring_succ":
            _rejected(L, call(good(**{name: None})), "gvec_nstep_gather: a required pointer is NULL (only ring_succ may be, with n_step == 1)")
    _rejected(L, call(good(n_step=1, ring_succ=None, idx=None)), "a required pointer is NULL (only ring_succ may be")
    # order: scalars, gamma, ring_succ, pointers
    _rejected(L, call(good(capacity=0, gamma=-1.0, ring_succ=None, idx=None)), "outside [0, 2^28]")
    _rejected(L, call(good(gamma=-1.0, ring_succ=None, idx=None)), "must be finite")
    _rejected(L, call(good(ring_succ=None, idx=None)), "ring_succ is NULL with n_step")


# ---- on-policy rollouts ----------------------------------------------------------------------------------------------

NULL_TEXT = "%s: args or a required pointer is NULL"
SHAPE_TEXT = "%s: T %d, N %d: both must be >= 1 (and T * N <= 2^40)"


def test_traj_scratch_bytes(L):
    for T, N in ((0, 4), (4, 0), (-1, -1), ((1 << 20) + 1, 1 << 20)):
        assert L.gvec_traj_scratch_bytes(T, N) == 0
        assert (SHAPE_TEXT % ("gvec_traj_scratch_bytes", T, N)).encode() in L.gvec_last_error()
    assert L.gvec_traj_scratch_bytes(1, 1) > 0 and L.gvec_traj_scratch_bytes(1 << 20, 1 << 20) > 0


RECORD = dict(T=8, t=3, num_envs=4, num_learners=2)


def test_traj_record(L):
    fn = "gvec_traj_record"
    call = lambda a: L.gvec_traj_record(0, None, C.byref(a))
    good = lambda **over: _args(lib.TrajRecordArgs, RECORD, **over)
    _rejected(L, L.gvec_traj_record(0, None, None), NULL_TEXT % fn)
    for over in (dict(num_envs=0), dict(num_learners=0)):
        _rejected(L, call(good(**over)), "N = num_envs * num_learners must be >= 1")
    _rejected(L, call(good(T=0)), SHAPE_TEXT % (fn, 0, 8))
    _rejected(L, call(good(T=(1 << 40) // 8 + 1)), SHAPE_TEXT % (fn, (1 << 40) // 8 + 1, 8))
    for t in (-1, 8):
        _rejected(L, call(good(t=t)), "gvec_traj_record: t %d outside [0, T = 8)" % t)
    for name in _pointers(lib.TrajRecordArgs):
        _rejected(L, call(good(**{name: None})), NULL_TEXT % fn)
    # order: learners, shape, t, pointers
    _rejected(L, call(good(num_envs=0, T=0, t=-1, flags=None)), "N = num_envs * num_learners")
    _rejected(L, call(good(T=0, t=-1, flags=None)), "both must be >= 1")
    _rejected(L, call(good(t=-1, flags=None)), "outside [0, T = 8)")


GAE = dict(T=8, N=4, gamma=0.99, lam=0.95)


def test_traj_gae(L):
    fn = "gvec_traj_gae"
    call = lambda a: L.gvec_traj_gae(0, None, C.byref(a))
    good = lambda **over: _args(lib.TrajGaeArgs, GAE, **over)
    _rejected(L, L.gvec_traj_gae(0, None, None), NULL_TEXT % fn)
    for over in (dict(T=0), dict(N=0), dict(T=1 << 21, N=1 << 20)):
        _rejected(L, call(good(**over)), SHAPE_TEXT % (fn, over.get("T", 8), over.get("N", 4)))
    for over in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=NAN), dict(lam=-0.1), dict(lam=1.5), dict(lam=NAN)):
        _rejected(L, call(good(**over)), "gvec_traj_gae: gamma")
        assert b"outside [0, 1]" in L.gvec_last_error()
    for name in _pointers(lib.TrajGaeArgs):
        _rejected(L, call(good(**{name: None})), NULL_TEXT % fn)
    _rejected(L, call(good(scratch=ODD)), "gvec_traj_gae: scratch must be 16-byte aligned")
    # order: shape, discounts, pointers, alignment
    _rejected(L, call(good(T=0, gamma=2.0, adv=None, scratch=ODD)), "both must be >= 1")
    _rejected(L, call(good(gamma=2.0, adv=None, scratch=ODD)), "outside [0, 1]")
    _rejected(L, call(good(adv=None, scratch=ODD)), NULL_TEXT % fn)


def test_traj_compact(L):
    fn = "gvec_traj_compact"
    call = lambda a: L.gvec_traj_compact(0, None, C.byref(a))
    good = lambda **over: _args(lib.TrajCompactArgs, dict(T=8, N=4), **over)
    _rejected(L, L.gvec_traj_compact(0, None, None), NULL_TEXT % fn)
    for over in (dict(T=0), dict(N=-3)):
        _rejected(L, call(good(**over)), SHAPE_TEXT % (fn, over.get("T", 8), over.get("N", 4)))
    for name in _pointers(lib.TrajCompactArgs):
        _rejected(L, call(good(**{name: None})), NULL_TEXT % fn)
    _rejected(L, call(good(scratch=ODD)), "gvec_traj_compact: scratch must be 16-byte aligned")
    _rejected(L, call(good(T=0, idx=None, scratch=ODD)), "both must be >= 1")
    _rejected(L, call(good(idx=None, scratch=ODD)), NULL_TEXT % fn)


GATHER = dict(T=8, N=4, M=16, obs_floats=8, mask_bytes=4)


def test_traj_gather(L):
    fn = "gvec_traj_gather"
    call = lambda a: L.gvec_traj_gather(0, None, C.byref(a))
    good = lambda **over: _args(lib.TrajGatherArgs, GATHER, **over)
    _rejected(L, L.gvec_traj_gather(0, None, None), NULL_TEXT % fn)
    _rejected(L, call(good(T=0)), SHAPE_TEXT % (fn, 0, 4))
    for over in (dict(M=-1), dict(obs_floats=0), dict(mask_bytes=-1)):
        _rejected(L, call(good(**over)), "gvec_traj_gather: M %d < 0, obs_floats" % over.get("M", 16))
    everything = {n: None for n in _pointers(lib.TrajGatherArgs)}
    assert call(good(M=0, **everything)) == OK                       # nothing to gather: no device, no arrays
    _rejected(L, call(good(M=0, T=0)), "both must be >= 1")          # ... but the checks above M == 0 hold
    _rejected(L, call(good(M=0, obs_floats=0)), "obs_floats 0 < 1")
    for name in _pointers(lib.TrajGatherArgs):
        if name != "stats":   # optional
            _rejected(L, call(good(**{name: None})), NULL_TEXT % fn)
    # the masks are required only when they have bytes: without them the check moves on to the next NULL
    _rejected(L, call(good(mask_bytes=0, mask=None, out_mask=None, stats=None, rejected=None)), NULL_TEXT % fn)
    _rejected(L, call(good(T=0, M=-1, pos=None)), "both must be >= 1")
    _rejected(L, call(good(M=-1, pos=None)), "M -1 < 0")


# ---- policy head -----------------------------------------------------------------------------------------------------

POLICY = [
    ("gvec_policy_sample", lib.PolicySampleArgs, dict(rows=5, num_actions=7, greedy=0, seed=1, row_base=0),
     ("logits", "mask", "action", "logp", "entropy")),
    ("gvec_policy_evaluate", lib.PolicyEvaluateArgs, dict(rows=5, num_actions=7), ("logits", "mask", "action", "logp", "entropy")),
    ("gvec_policy_backward", lib.PolicyBackwardArgs, dict(rows=5, num_actions=7), ("logits", "mask", "action", "grad_logits")),
]


@pytest.mark.parametrize("fn,cls,scalars,required", POLICY, ids=[p[0] for p in POLICY])
def test_policy_head(L, fn, cls, scalars, required):
    f = getattr(L, fn)
    call = lambda a: f(0, None, C.byref(a))
    good = lambda **over: _args(cls, scalars, **over)
    _rejected(L, f(0, None, None), NULL_TEXT % fn)
    for over in (dict(rows=-1), dict(rows=1 << 31), dict(num_actions=0)):
        _rejected(L, call(good(**over)), "%s: rows %d outside [0, 2^31) or num_actions" % (fn, over.get("rows", 5)))
    for name in required:
        _rejected(L, call(good(**{name: None})), fn + ": a required pointer is NULL")
    assert call(good(rows=0)) == OK                                               # no rows: no device
    assert call(good(rows=0, **{n: None for n in _pointers(cls) if n not in required})) == OK
    _rejected(L, call(good(rows=0, logits=None)), fn + ": a required pointer is NULL")   # ... but the pointers before rows == 0
    _rejected(L, call(good(rows=-1, logits=None)), "outside [0, 2^31)")
