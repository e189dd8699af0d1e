"""gvec_bot_actions (bot_kernel) against the numpy restatement of the scripted opponent's rule (tests/_bot_reference.py),
slot for slot, and the vector env's opponent="bot" against its manual composition."""
import numpy as np
import pytest

import _bot_reference as R
import _harness as H
import _state_forms as F
from test_bot_reference import hand_state, STRENGTH_FLOOR, STRENGTH_TURNS

pytestmark = pytest.mark.gpu


def _g():
    import generalsreinforcementlearning_amd as g
    return g


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))


def assert_actions_equal(hip, ref, ctx):
    h, r = _bytes(hip), _bytes(ref)
    if not np.array_equal(h, r):
        e, p = np.argwhere((h != r).any(axis=-1))[0]
        raise AssertionError(f"{ctx}: {int((h != r).any(axis=-1).sum())} slot(s) differ; first env {e} player {p}: "
                             f"hip={hip[e, p]} restatement={ref[e, p]}")


def check_engine(eng, ctx, masks=None, seed=0, permille=0):
    """every mask in `masks` (default: all seats, then each seat alone, then a pattern) against the restatement"""
    st = eng.game_state()
    full = (1 << eng.max_p) - 1
    masks = masks or [full] + [1 << p for p in range(eng.max_p)] + [full & 0x55]
    agent = eng.agent_actions(seed) if permille else None
    for m in masks:
        hip = eng.bot_actions(m, seed, permille)
        ref = R.bot_actions(st, m, eng.fog_of_war, seed, permille, agent=agent, max_p=eng.max_p)
        assert_actions_equal(hip, ref, f"{ctx} players {m:#x}")
    return st


def engine_from(sizes, mw, mh, maxp, fog, seed, auto_reset=False):
    g = _g()
    army, owner, typ, w, h, p = H.gen_boards(seed, sizes, mw, mh)
    eng = g.VecEngine(len(sizes), mw, mh, maxp, fog_of_war=fog, auto_reset=auto_reset)
    eng.reset(army, owner, typ, w, h, p)
    return eng


@pytest.mark.parametrize("fog", [True, False])
def test_fresh_and_played_boards(fog):
    sizes = [(15, 15, 2), (20, 20, 4), (13, 9, 3), (20, 17, 4), (6, 6, 2)] * 8 + [(20, 20, 4)] * 3   # 43 envs: a padded wave
    eng = engine_from(sizes, 20, 20, 4, fog, 21)
    done = 0
    for turns in (0, 50, 500):
        eng.rollout(turns - done, 77, 0, fused=False, want_stats=False)
        done = turns
        check_engine(eng, f"fog={fog} turn {turns}")
    eng.close()


@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS))
def test_every_layout(maxp, slots, parity):
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, 10)
    eng = engine_from(sizes, mw, mh, maxp, True, 5 + slots)
    check_engine(eng, f"<{maxp},{slots},{parity}> fresh", masks=[(1 << maxp) - 1])
    eng.rollout(60, 3, 40, fused=False, want_stats=False)        # invalid moves: lists out of step with ownership
    check_engine(eng, f"<{maxp},{slots},{parity}> turn 60", masks=[(1 << maxp) - 1, 0b10])
    eng.close()


@pytest.mark.parametrize("w,h,P,fog", [(20, 20, 4, True), (15, 15, 2, False)])
def test_aged_batches(w, h, P, fog):
    B = 48
    eng = engine_from([(w, h, P)] * B, w, h, P, fog, 8)
    eng.rollout(8, 12, 80, fused=False, want_stats=False)
    F.age_batch(eng, 12)
    wide = ldiff = 0
    for k in range(6):
        st = check_engine(eng, f"aged step {k}", masks=[(1 << P) - 1])
        F.check_flag_invariants(eng, st, f"aged step {k}")
        wide += int(F.wide_envs(st).sum())
        ldiff += int(F.desynced_envs(st).sum())
        eng.rollout(1 + 20 * k, 13, 30, fused=False, want_stats=False)
    assert wide > 0 and ldiff > 0, "the run must hold wide-army and HF_LDIFF envs"
    eng.close()


def test_done_envs_dead_players_and_empty_seats():
    sizes = [(6, 6, 2), (7, 6, 3), (8, 8, 4), (6, 7, 3)] * 12
    eng = engine_from(sizes, 8, 8, 4, True, 4)
    seen_done = seen_dead = False
    for k in range(8):
        eng.rollout(150, 30 + k, 0, fused=False, want_stats=False)
        st = check_engine(eng, f"round {k}")
        seen_done |= bool(st["done"].any())
        dead = ~st["alive"].astype(bool) & (np.arange(4)[None, :] < st["players"][:, None]) & (st["done"] == 0)[:, None]
        seen_dead |= bool(dead.any())
    assert seen_done and seen_dead
    eng.close()


def test_hand_built_boards():
    g = _g()
    boards = [["N0=9 G1=3 C-=1 N1=1", "G0=2 . . ."],
              ["N1=1 N0=9 C-=5 .", ". N0=9 . G1=1", "G0=1 . . ."],
              ["N0=9 N-=7 . N0=4", "G0=1 # # #", "# # # G1=1"],
              [". N0=4 .", "# G0=1 G1=1"],
              ["N0=3 N1=2 .", "G0=1 # G1=1"],
              [f"N0={10 ** 8} N1={10 ** 8 - 5} . N0={10 ** 8 - 10}", f"G0=1 # # N1={10 ** 8 - 12}", "# # # G1=1"],
              ["N0=2 N0=6 N0=5 N0=1 N1=1 .", "G0=1 # # # # G1=1"],
              ["N0=1 N0=1 G1=1", "N0=7 N0=1 N0=1", "G0=1 # #"],
              ["N0=5 N0=1 . . . . .", "G0=1 # # # # # G1=1"],
              ["N0=5 N0=1 C-=40 . .", "# G0=1 # . .", "# # # . G1=1"],
              ["N0=5 N0=1 # . .", "# G0=1 # . .", "# # # . G1=1"]]     # every player holds a general: alive
    for fog in (False, True):
        states = [hand_state(b) for b in boards]
        mw, mh = 8, 8
        eng = g.VecEngine(len(boards), mw, mh, 2, fog_of_war=fog)
        army = np.zeros((len(boards), mw * mh), np.int32)
        owner = np.full((len(boards), mw * mh), -1, np.int8)
        typ = np.zeros((len(boards), mw * mh), np.uint8)
        for i, s in enumerate(states):
            n = s["army"].shape[1]
            army[i, :n], owner[i, :n], typ[i, :n] = s["army"][0], s["owner"][0], s["type"][0]
        eng.reset(army, owner, typ, [s["width"][0] for s in states], [s["height"][0] for s in states], [2] * len(boards))
        check_engine(eng, f"hand-built fog={fog}")
        eng.close()


def test_sharded_handle_and_refusals():
    g = _g()
    sizes = [(15, 15, 2), (20, 20, 4), (9, 11, 3)] * 10
    army, owner, typ, w, h, p = H.gen_boards(2, sizes, 20, 20)
    plain = g.VecEngine(len(sizes), 20, 20, 4)
    many = g.VecEngine(len(sizes), 20, 20, 4, devices=[0, 0, 0])
    for e in (plain, many):
        e.reset(army, owner, typ, w, h, p)
        e.rollout(40, 9, 0, fused=False, want_stats=False)
    for m, seed, pm in ((0b1111, 0, 0), (0b0101, 3, 250)):
        assert_actions_equal(many.bot_actions(m, seed, pm), plain.bot_actions(m, seed, pm), f"sharded players {m:#x}")
    check_engine(plain, "plain", masks=[0b1111])
    import torch
    buf = torch.zeros((len(sizes), 4, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(g.GvecError):
        many.bot_actions_device(0b1, 0, 0, buf.data_ptr())     # sharded handles: host memory only
    for bad in (-1, 1001):
        with pytest.raises(g.GvecError):
            plain.bot_actions(0b1, 0, bad)
    with pytest.raises(g.GvecError):
        plain.bot_actions(1 << 4)                              # a seat at max_players
    plain.close()
    many.close()


def test_untouched_slots_host_and_device():
    import torch
    g = _g()
    sizes = [(15, 15, 2), (20, 20, 4), (12, 12, 3)] * 7
    eng = engine_from(sizes, 20, 20, 4, True, 6)
    eng.rollout(30, 1, 0, fused=False, want_stats=False)
    st = eng.game_state()
    rng = np.random.default_rng(0)
    junk = rng.integers(0, 256, (len(sizes), 4, 8), dtype=np.uint8)
    ref = R.bot_actions(st, 0b0110, True, max_p=4)
    host = junk.copy().view(g.ACTION_DTYPE).reshape(len(sizes), 4)
    out = eng.bot_actions([1, 2], actions=host)
    assert out is host
    hb = _bytes(host)
    assert np.array_equal(hb[:, [0, 3]], junk[:, [0, 3]]), "host memory: a slot outside `players` changed"
    assert np.array_equal(hb[:, [1, 2]], _bytes(ref)[:, [1, 2]])
    dev = torch.as_tensor(junk).cuda()
    eng.bot_actions_device(0b0110, 0, 0, dev.data_ptr())
    torch.cuda.synchronize()
    db = dev.cpu().numpy()
    assert np.array_equal(db[:, [0, 3]], junk[:, [0, 3]]), "device memory: a slot outside `players` changed"
    assert np.array_equal(db[:, [1, 2]], _bytes(ref)[:, [1, 2]])
    eng.close()


def test_random_permille_mix():
    sizes = [(15, 15, 2), (20, 20, 4), (10, 10, 3)] * 30
    eng = engine_from(sizes, 20, 20, 4, True, 17)
    eng.rollout(25, 4, 0, fused=False, want_stats=False)
    for mix in ((6554, 19661), (0, 0)):
        eng.set_agent_mix(*mix)
        for seed in (0, 5, 2 ** 40 + 3):
            assert_actions_equal(eng.bot_actions(0b1111, seed, 1000), eng.agent_actions(seed), f"permille 1000 mix {mix} seed {seed}")
    eng.set_agent_mix()
    st = check_engine(eng, "permille 300", masks=[0b1111, 0b0010], seed=9, permille=300)
    n = sum(R.takes_random(9, e, int(st["turn"][e]), p, 300) for e in range(len(sizes)) for p in range(4))
    assert 0.2 < n / (4 * len(sizes)) < 0.4
    eng.close()


def test_bot_beats_the_random_agent_on_the_device():
    """4,096 boards 15x15 2P, every call on device memory: the bot in seat 0, then seat 1, against the random agent."""
    import torch
    g = _g()
    B = 4096
    for seat in (0, 1):
        eng = g.VecEngine(B, 15, 15, 2)
        eng.reset_generated(100 + seat)
        acts = torch.zeros((B, 2, 8), dtype=torch.uint8, device="cuda")
        for k in range(STRENGTH_TURNS):
            g._lib.check(eng.L.gvec_agent_actions(eng.h, 500 + k, 0, acts.data_ptr(), g.vec_engine.MEM_DEVICE), "gvec_agent_actions")
            eng.bot_actions_device(1 << seat, 0, 0, acts.data_ptr())
            eng.step_device(acts.data_ptr())
            if k % 100 == 99 and eng.game_state(fields=("done",))["done"].all():
                break
        st = eng.game_state(fields=("done", "winner"))
        wins = int(((st["done"] == 1) & (st["winner"] == seat)).sum())
        assert wins >= STRENGTH_FLOOR * B, f"seat {seat}: {wins} / {B} wins within {k + 1} turns"
        eng.close()


def _learner_actions(mask, gen):
    import torch
    m = mask.reshape(mask.shape[0], -1).float() + 1e-6
    return torch.multinomial(m, 1, generator=gen).reshape(-1)


@pytest.mark.parametrize("permille", [0, 150])
def test_vector_env_bot_equals_manual_composition(permille):
    import torch
    g = _g()
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    B, P, seed = 512, 2, 3
    bot = GeneralsVecEnv(B, 15, 15, P, seed=seed, device_outputs=True, opponent="bot", opponent_random_permille=permille, max_turns=120)
    man = GeneralsVecEnv(B, 15, 15, P, seed=seed, device_outputs=True, max_turns=120)
    o1, i1 = bot.reset()
    o2, i2 = man.reset()
    buf = torch.zeros((B, P, 8), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    finished = 0
    for k in range(200):
        a = _learner_actions(i1["valid_actions_mask"], gen)
        man.engine.bot_actions_device(0b10, seed + 1000 * k + 1, permille, buf.data_ptr())
        r1 = bot.step(a)
        r2 = man.step(a, other_actions=buf)
        for x, y, name in zip(r1[:4], r2[:4], ("obs", "reward", "terminated", "truncated")):
            assert torch.equal(x, y), f"step {k}: {name} differs"
        for key in ("turn", "valid_actions_mask", "invalid_action", "winner", "reset"):
            assert torch.equal(r1[4][key], r2[4][key]), f"step {k}: info[{key}] differs"
        i1 = r1[4]
        finished += int((r1[2] | r1[3]).sum())
    assert finished > 0
    bot.close()
    man.close()


def test_vector_env_random_opponent_unchanged():
    import torch
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    B = 256
    a = GeneralsVecEnv(B, 15, 15, 2, seed=4, device_outputs=True, opponent="random")
    b = GeneralsVecEnv(B, 15, 15, 2, seed=4, device_outputs=True)
    _, ia = a.reset()
    b.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    for k in range(100):
        act = _learner_actions(ia["valid_actions_mask"], gen)
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra[:4], rb[:4]):
            assert torch.equal(x, y), f"step {k}"
        ia = ra[4]
    with pytest.raises(ValueError):
        GeneralsVecEnv(4, 8, 8, 2, opponent="league")
    a.close()
    b.close()
