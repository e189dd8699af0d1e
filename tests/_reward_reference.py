"""numpy float32 restatement of the reference's configurable reward - TEST INFRASTRUCTURE ONLY.

Written from internal/experience/rewards.go (CalculateRewardWithConfig :45-85, countCityChanges :110-129,
countGeneralChanges :132-151, calculateArmyAdvantage :153-175, NormalizeReward :215-223) and internal/game/state.go
(IsGameOver :73-82, GetWinner :84-100), not from the kernel.  On top of the Go function it states the three rules of
gvec_experience_rewards_config (include/generals_vec.h): the clip, the zero of a row without a predecessor, invalid_action.

States are dicts of the state-view planes (VecEngine.game_state / OracleBatch.read_state): owner [B][S] int8, army [B][S]
int32, type [B][S] uint8, alive [B][P], players / width / height / turn [B].
"""
import numpy as np

TILE_GENERAL, TILE_CITY = 1, 2      # core/board.go:20-26 as the state view encodes them
F = np.float32
TERMS = ("d_territory", "d_army", "cities_gained", "cities_lost", "generals_gained", "generals_lost", "outcome", "army_advantage_bits")


def normalize_reward(r):
    """NormalizeReward (:215-223)"""
    r = np.asarray(r, F)
    return np.where(r > F(1.0), F(1.0), np.where(r < F(-1.0), F(-1.0), r)).astype(F)


def shaped_terms(prev, cur, p):
    """The integer counts and the float32 army advantage CalculateRewardWithConfig reads for player p, per env."""
    po, co = prev["owner"].astype(np.int64), cur["owner"].astype(np.int64)
    pa, ca = prev["army"].astype(np.int64), cur["army"].astype(np.int64)
    mine_p, mine_c = po == p, co == p
    d_terr = mine_c.sum(1) - mine_p.sum(1)                                       # :59-61
    d_arm = (ca * mine_c).sum(1) - (pa * mine_p).sum(1)                          # :65-67
    city, gen = cur["type"] == TILE_CITY, cur["type"] == TILE_GENERAL            # the CURRENT tile's type decides (:112, :134)
    c_gain = (city & ~mine_p & mine_c).sum(1)                                    # :119-121
    c_lost = (city & mine_p & ~mine_c).sum(1)                                    # :124-126
    g_gain = (gen & ~mine_p & (po >= 0) & mine_c).sum(1)                         # :141-143
    g_lost = (gen & mine_p & ~mine_c).sum(1)                                     # :146-148
    player = (ca * mine_c).sum(1)                                                # :158-164
    enemy = (ca * ((co >= 0) & ~mine_c)).sum(1)
    total = player + enemy
    with np.errstate(divide="ignore", invalid="ignore"):
        adv = np.where(total == 0, F(0.0), (player - enemy).astype(F) / total.astype(F)).astype(F)   # :167-174
    return d_terr, d_arm, c_gain, c_lost, g_gain, g_lost, adv


def recombine(terms, cfg):
    """terms [..., 8] int32 -> the Go-side float32 value before clip / zero / invalid_action: the definition's order of additions."""
    t = np.asarray(terms, np.int32)
    adv = np.ascontiguousarray(t[..., 7]).view(F)
    r = np.zeros(t.shape[:-1], F)
    r = r + t[..., 0].astype(F) * F(cfg.territory_gained)
    r = r + t[..., 1].astype(F) * F(cfg.army_gained)
    r = r + t[..., 2].astype(F) * F(cfg.capture_city)
    r = r + t[..., 3].astype(F) * F(cfg.lose_city)
    r = r + t[..., 4].astype(F) * F(cfg.capture_general)
    r = r + t[..., 5].astype(F) * F(cfg.lose_general)
    r = r + adv * F(cfg.army_advantage)
    r = np.where(t[..., 6] > 0, F(cfg.win_game), np.where(t[..., 6] < 0, F(cfg.lose_game), r))
    return r.astype(F)


def comparable_rows(prev, cur):
    """an env re-dealt (or not stepped) since the snapshot has no predecessor"""
    return (prev["width"] == cur["width"]) & (prev["height"] == cur["height"]) & (cur["turn"] > prev["turn"])


def reward_reference(prev, cur, cfg, players=None, invalid=None):
    """-> rewards float32 [B][K], terms int32 [B][K][8], done bool [B]; players: seat ids (None: all), columns ascending."""
    B, P = cur["alive"].shape
    ids = list(range(P)) if players is None else sorted(int(p) for p in players)
    seats = np.arange(P)[None, :] < cur["players"][:, None]
    alive = (cur["alive"] != 0) & seats
    n_alive = alive.sum(1)
    over = n_alive <= 1                                                          # IsGameOver
    winner = np.where(n_alive == 1, alive.argmax(1), -1)                         # GetWinner
    comparable = comparable_rows(prev, cur)
    rewards, terms = np.zeros((B, len(ids)), F), np.zeros((B, len(ids), 8), np.int32)
    for k, p in enumerate(ids):
        d_terr, d_arm, c_gain, c_lost, g_gain, g_lost, adv = shaped_terms(prev, cur, p)
        r = np.zeros(B, F)                                                       # :46
        r = r + d_terr.astype(F) * F(cfg.territory_gained)                       # :62 (TerritoryLost is never read)
        r = r + d_arm.astype(F) * F(cfg.army_gained)                             # :68 (ArmyLost is never read)
        r = r + c_gain.astype(F) * F(cfg.capture_city)                           # :72
        r = r + c_lost.astype(F) * F(cfg.lose_city)                              # :73
        r = r + g_gain.astype(F) * F(cfg.capture_general)                        # :77
        r = r + g_lost.astype(F) * F(cfg.lose_general)                           # :78
        r = r + adv * F(cfg.army_advantage)                                      # :82
        won, lost = over & (winner == p), over & (winner != -1) & (winner != p)
        r = np.where(won, F(cfg.win_game), np.where(lost, F(cfg.lose_game), r)).astype(F)   # :49-56
        if cfg.clip:
            r = normalize_reward(r)
        live = comparable & (p < cur["players"])
        r = np.where(live, r, F(0.0)).astype(F)
        t = np.stack([d_terr, d_arm, c_gain, c_lost, g_gain, g_lost, won.astype(np.int64) - lost.astype(np.int64),
                      adv.view(np.int32).astype(np.int64)], axis=1).astype(np.int32)
        terms[:, k] = np.where(live[:, None], t, 0)
        if invalid is not None:
            inv = np.asarray(invalid).reshape(B, len(ids))[:, k] != 0
            r = np.where(inv, r + F(cfg.invalid_action), r).astype(F)
        rewards[:, k] = r
    return rewards, terms, over
