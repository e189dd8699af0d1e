"""The observation and mask writers on every store path their selectors can pick (tests/_store_paths.py), on the GPU.

For each compiled <players, slots, parity> variant: a ragged batch of nine envs is played for about thirty turns, armies
above 1,000 and above 65,535 are planted, the state is saved on the device, and every entry point that writes into a
caller's device buffer is launched once per placement - the buffer a few bytes off a 256-byte boundary, inside one
allocation with guard bands (tests/_slab.py).  What a launch must have written comes from the kernels' own references,
computed from the state read back AFTER the launch: tests/_gym_reference.py for the gym kernels, the oracle for gvec_observe
and the packed masks, experience.decode_records for the expansion.  Every output is compared bit for bit, every input and
every byte between the buffers must be what was uploaded, and the path each launch took - computed from its real pointers -
must be the one tests/test_store_paths.py promised from the placements alone.

Boards smaller than the handle's limits: no reference has padding, so the expectation is what the header says of a slot -
the env's own [9][H][W] (mask: [H*W*5]) at the start, index y*W + x, zeros behind it - and, from gym_emit's own words, the
turn plane filled over the whole stride ("the whole plane, like obs[7, :, :] = ...").  Every path must write these same bytes.

Run with -s to see (site, path, sh, windows) of every launch."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import _gym_reference as G
import _harness as H
import _oracle as O
import _store_paths as SP
from _slab import Slab

pytestmark = pytest.mark.gpu
B, MAX_TURNS = SP.B, SP.MAX_TURNS
TURN_IN = np.array([0, 5, 63, 64, 100, 7, 31, 9, 10], np.int64)      # the turn plane: below, at and beyond max_turns


class _Case:
    """One engine, its saved twin, the oracle that mirrors read-back states, and the tally of paths taken."""

    def __init__(self, maxp, slots, parity):
        import torch
        import generalsreinforcementlearning_amd as g
        from generalsreinforcementlearning_amd._lib import check
        g.load()
        self.t, self.check, self.maxp, self.key = torch, check, maxp, (maxp, slots, parity)
        self.mw, self.mh, self.sizes = H.variant_batch(maxp, slots, parity, B)
        self.stride = self.mw * self.mh
        self.tiles = [w * h for w, h, _ in self.sizes]
        seed = 900 + slots
        mk = lambda: g.VecEngine(B, self.mw, self.mh, maxp, fog_of_war=True, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream)
        self.eng, self.saved = mk(), mk()
        self.ora = O.OracleBatch(B, self.mw, self.mh, maxp, fog=True)
        for target in (self.eng, self.ora):
            SP.deal(target, maxp, slots, parity, seed)
            SP.prepare(target, seed)
        st = self.eng.game_state()
        H.assert_states_equal(st, self.ora.read_state(), "the prepared state")      # what the CPU test checked is what runs here
        SP.check_prepared(st, maxp, slots, parity)
        self.saved.copy_envs(n=B, src=self.eng)                                      # the on-device save of env_state.py
        self.took = {site: set() for site in SP.SELECTORS}
        self.cache = {}
        self.seen = {"planes": set(), "legal": 0, "mid": set(), "wide": set(), "slots": set(), "launches": 0}

    def restore(self):
        self.eng.copy_envs(n=B, src=self.saved)

    def state(self):
        self.t.cuda.synchronize()
        st = self.eng.game_state()
        return st, hashlib.blake2b(b"".join(st[k].tobytes() for k in sorted(st)), digest_size=16).digest()

    def slab(self, sizes, groups, shift):
        return Slab(sizes, groups, shift, align=256)

    def note(self, name, placement, paths, promised):
        assert paths == promised, (name, placement, sorted(paths ^ promised, key=str)[:6])
        for e in paths:
            self.took[e[0]].add(e)
        self.seen["launches"] += 1
        print(f"{name} {placement}:", *sorted(paths, key=str))

    # ---- the gym reference on a read-back state ---------------------------------------------------------------------
    def gym_expected(self, st, digest, players, turn):
        """obs [B][L][9][stride] float32, mask [B][L][stride * 5] uint8 of the learners `players` at turn counts `turn`"""
        key = ("gym", digest, tuple(players), turn.tobytes())
        if key in self.cache:
            return self.cache[key]
        obs = np.zeros((B, len(players), 9, self.stride), np.float32)
        mask = np.zeros((B, len(players), self.stride * 5), np.uint8)
        for j, p in enumerate(players):
            vis, fog = self.eng.compute_player_visibility(p)
            view = G.proto_view(st["owner"], st["army"], st["type"], vis, fog)
            for e in range(B):
                w, h = int(st["width"][e]), int(st["height"][e])
                n = w * h
                sub = {k: v[e:e + 1] for k, v in view.items()}
                o = G.build_observation(sub, p, turn[e:e + 1], MAX_TURNS, w, h).reshape(9, n)
                obs[e, j, :, :n] = o
                obs[e, j, 7, :] = o[7, 0]
                mask[e, j, :n * 5] = G.valid_actions_mask(sub, p, w, h)[0]
                self._tally(e, p, o, n, st)
            self.seen["legal"] += int(mask[:, j].sum())
        self.cache[key] = (obs, mask)
        return obs, mask

    def _tally(self, e, p, o, n, st):
        """what keeps the comparison from being one of zeros"""
        for c in range(7):
            if len(np.unique(o[c])) >= 2:
                self.seen["planes"].add(c)
        if (o[1] == 0.5).any() and (o[1] == 1.0).any():
            self.seen["planes"].add("both owners")
        top = float(o[2].max())
        if e == SP.MID_ENV and np.log(1001.0) / 10 <= top <= np.log(65536.0) / 10:
            self.seen["mid"].add(p)
        if e == SP.WIDE_ENV:
            if top > np.log(65537.0) / 10:
                self.seen["wide"].add(p)
            self.seen["slots"] |= {s for s in range((n + 63) // 64) if o[2][64 * s:64 * s + 64].any()}

    def check_not_vacuous(self):
        s = self.seen
        assert set(range(7)) <= s["planes"] and "both owners" in s["planes"], s["planes"]
        assert s["legal"] > 0
        last = self.sizes[SP.WIDE_ENV][2] - 1
        assert {0, last} <= s["wide"] and {0, last} <= s["mid"], (s["wide"], s["mid"])   # in the sight of seat 0 and of the last seat
        assert s["slots"] == set(range((self.stride + 63) // 64)), s["slots"]

    # ---- launches -----------------------------------------------------------------------------------------------------
    def full_moves(self, st, digest, players):
        """[B][L] one full move per learner from its reference mask (action 0 where it has none) and [B][L] whether it has one"""
        _, mask = self.gym_expected(st, digest, players, TURN_IN)
        m = mask.reshape(B, len(players), self.stride, 5)[..., :4].reshape(B, len(players), -1).astype(bool)
        has = m.any(-1)
        first = m.argmax(-1)
        return np.where(has, (first // 4) * 5 + first % 4, 0).astype(np.int64), has

    def gym(self, name, players, placement, run, steps, turn_exp=None):
        """One gym launch: obs / mask placed, turn_count and the inputs beside them.  run(ptr) makes the call; ptr(name)
        is a buffer's address."""
        t, L = self.t, len(players)
        sizes = {"turn": 8 * B, "obs": B * L * 36 * self.stride, "mask": B * L * 5 * self.stride}
        inputs = dict(steps or {})
        sizes.update({k: np.asarray(v).nbytes for k, v in inputs.items()})
        slab = self.slab(sizes, [("turn",)] + [(k,) for k in inputs] + [("obs",), ("mask",)], {"obs": placement[0], "mask": placement[1]})
        slab.put("turn", TURN_IN)
        for k, v in inputs.items():
            slab.put(k, v)
        slab.upload(t, "cuda")
        ptr = lambda k: slab.at(k).data_ptr()
        assert ptr("obs") % 256 == placement[0] and ptr("mask") % 256 == placement[1]
        run(ptr)
        st, digest = self.state()
        turn = TURN_IN if turn_exp is None else turn_exp
        obs, mask = self.gym_expected(st, digest, players, turn)
        slab.check({"obs": obs.view(np.uint32), "mask": mask, "turn": turn}, f"{name} {self.key} at {placement}")
        self.note(name, placement, SP.gym_launch(ptr("obs"), ptr("mask"), self.stride, B * L),
                  SP.gym_launch(SP.BASE + placement[0], SP.BASE + placement[1], self.stride, B * L))


def _gym_launches(c):
    eng, L, maxp = c.eng, c.eng.L, c.maxp
    everyone, bits = list(range(maxp)), (1 << maxp) - 1
    c.restore()
    st0, d0 = c.state()
    zeros = np.zeros(B, np.uint8)
    for i, place in enumerate(SP.GYM_PLACEMENTS):
        p = 0 if i % 2 == 0 else maxp - 1                     # the single-learner kernels: seat 0 and the last seat in turn
        c.gym("gvec_gym_observe", [p], place, lambda ptr: c.check(
            L.gvec_gym_observe(eng.h, p, ptr("turn"), MAX_TURNS, ptr("obs"), ptr("mask"), None, None, None), "gvec_gym_observe"), None)
        c.gym("gvec_gym_observe_players", everyone, place, lambda ptr: c.check(
            L.gvec_gym_observe_players(eng.h, bits, ptr("turn"), MAX_TURNS, ptr("obs"), ptr("mask"), None, None, None), "gvec_gym_observe_players"), None)
        # the three that play a turn, each from the saved state
        acts, has = c.full_moves(st0, d0, [p])
        c.restore()
        c.gym("gvec_gym_step", [p], place, lambda ptr: c.check(
            L.gvec_gym_step(eng.h, p, 31 + i, ptr("actions"), ptr("resetting"), ptr("turn"), MAX_TURNS, ptr("obs"), ptr("mask"),
                            None, None, None, None, None, None, None, None, None), "gvec_gym_step"),
            {"actions": acts[:, 0], "resetting": zeros}, TURN_IN + has[:, 0])
        c.restore()
        t = c.t
        d_acts = t.zeros((B, maxp, 8), dtype=t.uint8, device="cuda")
        d_played = t.zeros(B, dtype=t.uint8, device="cuda")
        d_gym = t.from_numpy(acts[:, 0].copy()).cuda()
        d_mask = t.from_numpy(c.gym_expected(st0, d0, [p], TURN_IN)[1][:, 0].copy()).cuda()
        d_rs = t.zeros(B, dtype=t.uint8, device="cuda")
        c.check(L.gvec_agent_actions(eng.h, 31 + i, 0, d_acts.data_ptr(), 1), "gvec_agent_actions")
        c.check(L.gvec_gym_actions(eng.h, p, d_gym.data_ptr(), d_mask.data_ptr(), d_rs.data_ptr(), d_acts.data_ptr(), d_played.data_ptr(), None, None),
                "gvec_gym_actions")
        eng.step_device(d_acts.data_ptr())
        assert np.array_equal(d_played.cpu().numpy().astype(bool), has[:, 0])
        c.gym("gvec_gym_finish_step", [p], place, lambda ptr: c.check(
            L.gvec_gym_finish_step(eng.h, p, ptr("turn"), MAX_TURNS, ptr("resetting"), ptr("played"), ptr("obs"), ptr("mask"),
                                   None, None, None, None, None, None), "gvec_gym_finish_step"),
            {"resetting": zeros, "played": has[:, 0].astype(np.uint8)}, TURN_IN + has[:, 0])
        acts, _ = c.full_moves(st0, d0, everyone)
        c.restore()
        c.gym("gvec_gym_step_players", everyone, place, lambda ptr: c.check(
            L.gvec_gym_step_players(eng.h, bits, 31 + i, ptr("actions"), ptr("resetting"), ptr("turn"), MAX_TURNS, ptr("obs"), ptr("mask"),
                                    None, None, None, None, None, None, None, None, None), "gvec_gym_step_players"),
            {"actions": acts, "resetting": zeros}, TURN_IN + 1)


def _mirror(c):
    """the oracle on the state read back from the engine"""
    st, _ = c.state()
    c.ora.write_state(st)
    return st


def _observe_launches(c):
    eng, maxp, stride = c.eng, c.maxp, c.stride
    c.restore()
    for i, (off,) in enumerate(SP.OBSERVE_PLACEMENTS):
        for player in (0 if i % 2 == 0 else maxp - 1, -1):
            per_env = maxp if player < 0 else 1
            slab = c.slab({"out": B * per_env * 36 * stride}, [("out",)], {"out": off}).upload(c.t, "cuda")
            ptr = slab.at("out").data_ptr()
            assert ptr % 256 == off
            c.check(eng.L.gvec_observe(eng.h, player, ptr, 1), "gvec_observe")
            _mirror(c)
            want = np.stack([c.ora.observe(p) for p in range(maxp)], 1) if player < 0 else c.ora.observe(player)
            if player >= 0:      # armies beyond the tensor's clamp, in the player's sight
                assert all((want[e].reshape(9, stride)[0] == 1.0).any() for e in (SP.WIDE_ENV, SP.MID_ENV) if player < c.sizes[e][2])
            slab.check({"out": want.view(np.uint32)}, f"gvec_observe({player}) {c.key} at +{off}")
            c.note(f"gvec_observe({player})", (off,), SP.observe_launch(ptr, stride, c.tiles, per_env),
                   SP.observe_launch(SP.BASE + off, stride, c.tiles, per_env))


def _expand_launches(c):
    from generalsreinforcementlearning_amd.experience import decode_records
    eng, t, stride = c.eng, c.t, c.stride
    c.restore()
    lay = eng.experience_record_layout()
    mp, rd = lay["mp"], lay["record_dw"]
    rec_dev = t.zeros(B * rd, dtype=t.int32, device="cuda")
    eng.experience_begin()
    acts = eng.agent_actions(77)
    eng.step(acts)
    eng.experience_records(rec_dev.data_ptr(), actions=acts, env_id_base=1000)
    eng.synchronize()
    recs = rec_dev.cpu().numpy().view(np.uint32).reshape(B, rd)
    dec = decode_records(recs, lay)
    want = {"state": np.zeros((B, mp, 9 * stride), np.float32), "next_state": np.zeros((B, mp, 9 * stride), np.float32),
            "action_mask": np.zeros((B, mp, 4 * stride), np.uint8), "meta": np.zeros((B, mp, 8), np.int32)}
    want["meta"][:, :, 2] = np.arange(mp)
    acting = []
    for i in range(len(dec["env"])):
        r, p, w, h = int(dec["env"][i]) - 1000, int(dec["player_id"][i]), int(dec["width"][i]), int(dec["height"][i])
        n = w * h
        want["state"][r, p, :9 * n] = np.asarray(dec["state"][i]).reshape(-1)
        want["next_state"][r, p, :9 * n] = np.asarray(dec["next_state"][i]).reshape(-1)
        want["action_mask"][r, p, :4 * n] = dec["action_mask"][i]
        want["meta"][r, p] = [1, 1000 + r, p, dec["turn"][i], dec["action"][i], int(dec["reward"][i:i + 1].view(np.int32)[0]), int(dec["done"][i]), w | h << 8]
        acting.append((r, p, n))
    # not vacuous: every env's transition is there, seats of a small and of a full board, clamped armies, legal moves
    assert {r for r, _, _ in acting} == set(range(B)) and {n for _, _, n in acting} == set(c.tiles)
    assert {0, c.sizes[SP.WIDE_ENV][2] - 1} <= {p for r, p, _ in acting if r == SP.WIDE_ENV}
    assert (want["state"][SP.WIDE_ENV, 0, :stride] == 1.0).any() and want["action_mask"].any()
    assert set(acting) <= {(r, p, c.tiles[r]) for r in range(B) for p in range(c.sizes[r][2])}
    sizes = {"records": recs.nbytes, **{k: v.nbytes for k, v in want.items()}}
    lay8 = (C.c_int32 * 8)(rd, mp, lay["fd"], lay["ns"], lay["max_players"], stride, 0, 0)
    for place in SP.EXPAND_PLACEMENTS:
        shift = dict(zip(("state", "next_state", "action_mask"), place))
        slab = c.slab(sizes, [("records",), ("meta",), ("state",), ("next_state",), ("action_mask",)], shift)
        slab.put("records", recs)
        slab.upload(t, "cuda")
        ptr = lambda k: slab.at(k).data_ptr()
        assert all(ptr(k) % 256 == off for k, off in shift.items())
        c.check(eng.L.gvec_expand_experience_records(0, C.c_void_p(t.cuda.current_stream().cuda_stream), lay8, C.c_void_p(ptr("records")), B,
                                                     C.c_void_p(ptr("state")), C.c_void_p(ptr("next_state")), C.c_void_p(ptr("action_mask")),
                                                     C.c_void_p(ptr("meta"))), "gvec_expand_experience_records")
        t.cuda.synchronize()
        slab.check({"state": want["state"].view(np.uint32), "next_state": want["next_state"].view(np.uint32), "action_mask": want["action_mask"],
                    "meta": want["meta"]}, f"gvec_expand_experience_records {c.key} at {place}")
        c.note("gvec_expand_experience_records", place, SP.expand_launch(ptr("state"), ptr("next_state"), ptr("action_mask"), stride, mp, acting),
               SP.expand_launch(*(SP.BASE + o for o in place), stride, mp, acting))
    return acting


def _mask_launches(c):
    eng, maxp = c.eng, c.maxp
    nbytes = B * maxp * eng.mask_bytes
    assert eng.device_buffer(3) % 16 == 0          # where store_masks_staged writes, whatever the caller's pointer is
    acts = None
    for (off,) in SP.MASK_PLACEMENTS:
        c.restore()
        acts = eng.agent_actions(55) if acts is None else acts
        slab = c.slab({"actions": acts.nbytes, "legal": nbytes}, [("actions",), ("legal",)], {"legal": off})
        slab.put("actions", acts)
        slab.upload(c.t, "cuda")
        assert slab.at("legal").data_ptr() % 256 == off
        eng.step_device(slab.at("actions").data_ptr(), None, slab.at("legal").data_ptr())
        _mirror(c)
        want = c.ora.legal_mask()
        assert want.any()
        slab.check({"legal": want}, f"gvec_step {c.key} masks at +{off}")
        c.note("gvec_step", (off,), SP.masks_launch("store_masks", eng.device_buffer(3)), SP.masks_launch("store_masks", SP.BASE))
        slab = c.slab({"bits": nbytes}, [("bits",)], {"bits": off}).upload(c.t, "cuda")
        c.check(eng.L.gvec_serializer_mask(eng.h, slab.at("bits").data_ptr(), 1), "gvec_serializer_mask")
        want = c.ora.serializer_mask()                # of the state the step above left: the oracle mirrors it already
        assert want.any()
        slab.check({"bits": want}, f"gvec_serializer_mask {c.key} at +{off}")
        c.note("gvec_serializer_mask", (off,), SP.masks_launch("query_masks", slab.at("bits").data_ptr()), SP.masks_launch("query_masks", SP.BASE + off))


@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_every_store_path_writes_the_reference(maxp, slots, parity):
    c = _Case(maxp, slots, parity)
    _gym_launches(c)
    c.check_not_vacuous()
    _observe_launches(c)
    acting = _expand_launches(c)
    _mask_launches(c)
    # the paths taken, from the real pointers, are the promised ones - and they are every path there is
    assert c.took == SP.promised(maxp, slots, parity, learners=maxp, acting=acting)
    SP.assert_coverage(c.took, c.stride, c.tiles)
    assert c.seen["launches"] == 5 * len(SP.GYM_PLACEMENTS) + 2 * len(SP.OBSERVE_PLACEMENTS) + len(SP.EXPAND_PLACEMENTS) + 2 * len(SP.MASK_PLACEMENTS)
    c.eng.close()
    c.saved.close()


def test_serializer_mask_refuses_a_device_array_off_its_dwords():
    """gvec_serializer_mask stores dwords into a device array the header declares as bytes: one that is not 4-byte aligned
    is refused before any launch, and nothing is written."""
    import torch
    import generalsreinforcementlearning_amd as g
    g.load()
    eng = g.VecEngine(4, 8, 8, 2)
    eng.reset_generated(3)
    raw = torch.full((4 * 2 * eng.mask_bytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3):
        assert eng.L.gvec_serializer_mask(eng.h, raw.data_ptr() + off, 1) == -1
        assert b"gvec_serializer_mask: a device bits array must be 4-byte aligned" in eng.L.gvec_last_error()
    torch.cuda.synchronize()
    assert bool((raw == 0xA5).all())
    assert eng.L.gvec_serializer_mask(eng.h, raw.data_ptr() + 4, 1) == 0
    torch.cuda.synchronize()
    got = raw[4:4 + 4 * 2 * eng.mask_bytes].cpu().numpy().reshape(4, 2, -1)
    assert np.array_equal(got, eng.serializer_mask_bits()) and bool((raw[:4] == 0xA5).all()) and bool((raw[-12:] == 0xA5).all())
    eng.close()
