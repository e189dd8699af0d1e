"""TEST INFRASTRUCTURE - what tests/golden/make_gym_env_fixtures.py (the recorder) and tests/test_gym_env_fixtures.py (the
consumers) share about tests/golden/gym_env_fixtures.json: the lossless JSON form of an observation, the coverage
conditions the fixture has to meet, and the 67-env batches the recorded games are replayed in.

Floats are `float.hex()` strings (lossless for float64; every float32 is exactly a float64).  An observation is stored as
bitmaps for its 0/1 channels, two bitmaps for the ownership channel (0.5 = own, 1.0 = other), {value: [tiles]} for the
army channel and one value for the turn channel; channel 8 is all zero in the reference and asserted so."""
import numpy as np

import _harness as H

NUM_ENVS = 67                       # every replay batch; recorded games sit at their "env" index, the rest is filler
BIT_CHANNELS = (("vis", 0), ("normal", 3), ("mountain", 4), ("city", 5), ("general", 6))
DIRS = ((0, -1), (1, 0), (0, 1), (-1, 0))


def _bits_hex(b):
    return np.packbits(np.asarray(b, bool).ravel()).tobytes().hex()


def _hex_bits(s, n):
    return np.unpackbits(np.frombuffer(bytes.fromhex(s), np.uint8))[:n].astype(bool)


def encode_obs(obs):
    """float32 [9, H, W] -> JSON-able dict; asserts the observation has the form the dict can hold."""
    assert obs.dtype == np.float32 and obs.ndim == 3 and obs.shape[0] == 9
    o = obs.reshape(9, -1)
    d = {}
    for name, c in BIT_CHANNELS:
        assert np.isin(o[c], (0.0, 1.0)).all(), name
        d[name] = _bits_hex(o[c] == 1.0)
    assert np.isin(o[1], (0.0, 0.5, 1.0)).all()
    d["own"], d["other"] = _bits_hex(o[1] == 0.5), _bits_hex(o[1] == 1.0)
    army = {}
    for i in np.flatnonzero(o[2]):
        army.setdefault(float(o[2, i]).hex(), []).append(int(i))
    d["army"] = army
    assert (o[7] == o[7, 0]).all() and not o[8].any()
    d["turn"] = float(o[7, 0]).hex()
    return d


def decode_obs(d, w, h):
    n = w * h
    o = np.zeros((9, n), np.float32)
    for name, c in BIT_CHANNELS:
        o[c] = _hex_bits(d[name], n)
    o[1] = np.where(_hex_bits(d["own"], n), 0.5, np.where(_hex_bits(d["other"], n), 1.0, 0.0))
    for v, idx in d["army"].items():
        o[2, idx] = np.float32(float.fromhex(v))
    o[7] = np.float32(float.fromhex(d["turn"]))
    return o.reshape(9, h, w)


def decode_mask(idx, w, h):
    m = np.zeros(w * h * 5, bool)
    m[np.asarray(idx, np.int64)] = True
    return m


def encode_info(info):
    """keys + each value with its Python type; the mask travels on its own, game_id by type, error by presence."""
    out = {"keys": sorted(info)}
    for k, v in info.items():
        if k in ("valid_actions_mask", "error"):
            continue
        out[k] = [None if k == "game_id" else v, type(v).__name__]
    return out


def planes(game):
    return np.array(game["army"], np.int32), np.array(game["owner"], np.int8), np.array(game["type"], np.uint8)


def first_inboard_dir(t, w, h):
    x, y = t % w, t // w
    for d, (dx, dy) in enumerate(DIRS):
        if 0 <= x + dx < w and 0 <= y + dy < h:
            return d
    return 3


def refusal(step):
    keys = step["info"]["keys"]
    return "invalid" if keys == ["invalid_action"] else "error" if keys == ["error"] else None


# ---- coverage conditions (the issue's list): asserted by the recorder and re-asserted from the JSON by the CPU test ----
def coverage(fx):
    """-> {condition: True / False}, from the episodes of kind (a) and (b) alone."""
    c = {k: False for k in ("win", "loss", "truncation", "terminated_and_truncated", "mask_refused_odd", "mask_refused_even",
                            "half_out_of_mask", "half_accepted", "half_accepted_not_up", "negative_tile_delta", "fog_off",
                            "fogged_city_or_mountain", "hidden_as_normal", "army_1000")}
    server_refused = 0
    big = float(np.float32(np.log(1001.0) / 10.0))
    for g in fx["episodes"]:
        w, h, n = g["w"], g["h"], g["w"] * g["h"]
        c["fog_off"] |= not g["fog"]
        prev_tiles = g["reset"]["stats"][0]
        for s in [g["reset"]] + g["steps"]:
            o = decode_obs(s["obs"], w, h).reshape(9, n)
            quiet = (o[0] == 0) & (o[1] == 0) & (o[2] == 0)
            c["fogged_city_or_mountain"] |= bool((quiet & ((o[4] == 1) | (o[5] == 1))).any())
            c["hidden_as_normal"] |= bool((quiet & (o[3] == 1)).any())
            c["army_1000"] |= bool((o[2] >= big).any())
        for s in g["steps"]:
            r, a = float.fromhex(s["reward"]), s["action"]
            info, ref = s["info"], refusal(s)
            if ref == "invalid":
                c["mask_refused_odd" if n % 2 else "mask_refused_even"] = True
                c["half_out_of_mask"] |= a % 5 == 4
            server_refused += ref == "error" and a % 5 == 4
            if ref is None:
                if a % 5 == 4 and s["sent"][4]:
                    c["half_accepted"] = True
                    c["half_accepted_not_up"] |= first_inboard_dir(a // 5, w, h) != 0
                c["win"] |= s["terminated"] and r == 100.0 and info["winner"] == [0, "int"]
                c["loss"] |= s["terminated"] and r == -100.0
                c["truncation"] |= s["truncated"] and not s["terminated"] and g["max_turns"] <= 10
                c["terminated_and_truncated"] |= s["terminated"] and s["truncated"]
                c["negative_tile_delta"] |= s["stats"][0] < prev_tiles
                prev_tiles = s["stats"][0]
    c["two_server_refused_half_moves"] = server_refused >= 2
    return c


# ---- the replay batches --------------------------------------------------------------------------------------------------
def groups(fx):
    """The recorded episodes by (w, h, fog, max_turns): one GeneralsVecEnv / NumpyReferenceVecEnv batch each."""
    out = {}
    for g in fx["episodes"]:
        out.setdefault((g["w"], g["h"], bool(g["fog"]), g["max_turns"]), []).append(g)
    return out


def place(games):
    """{env index: game}: every game at its recorded index; a kind-(a) game recorded at index 0 (its replay does not depend
    on the index) also at the last index when that is free, so first, middle and last are all compared."""
    at = {g["env"]: g for g in games}
    assert len(at) == len(games)
    if 0 in at and at[0]["kind"] == "a":
        at.setdefault(NUM_ENVS - 1, at[0])
    return at


def batch_planes(games, w, h, players=2, filler_seed=11):
    """Planes of the 67 envs: generated filler boards with the recorded games put at their indices."""
    army, owner, typ, ws, hs, ps = H.gen_boards(filler_seed, [(w, h, players)] * NUM_ENVS, w, h)
    at = place(games)
    for e, g in at.items():
        army[e], owner[e], typ[e] = planes(g)
    return army, owner, typ, ws, hs, ps, at


def opponent_actions(dtype, base, at, k, max_players):
    """[67][max_players] actions of step k: `base` (the fillers' moves; None = nobody moves) with the recorded opponent move
    of every recorded env in seat 1 and nothing in its other seats."""
    a = np.zeros((NUM_ENVS, max_players), dtype) if base is None else np.array(base, dtype).reshape(NUM_ENVS, max_players)
    for e, g in at.items():
        a[e] = np.zeros(max_players, dtype)
        if k < len(g["steps"]) and g["steps"][k]["opponent"] is not None:
            fx_, fy, tx, ty, half = g["steps"][k]["opponent"]
            a[e, 1] = (fx_, fy, tx, ty, 1 | (2 if half else 0), (0, 0, 0))
    return a


def learner_actions(mask, at, k, rng):
    """[67] action indices of step k: the recorded one in a recorded env (0 once its episode is over), a seeded masked-random
    choice in a filler env."""
    acts = np.array([int(rng.choice(np.flatnonzero(m))) if m.any() else 0 for m in np.asarray(mask, bool)], np.int64)
    for e, g in at.items():
        acts[e] = g["steps"][k]["action"] if k < len(g["steps"]) else 0
    return acts
