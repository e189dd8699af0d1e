"""Rule-derived hazard scenarios, written in ROLES instead of coordinates, so that one derivation runs on every board,
placement, seat map and army scale (tests/test_hazard_matrix.py on the oracle, tests/test_hip_hazard_matrix.py on the device).

Every expected value below is derived in a comment from the reference's Go rules (paths relative to the reference's
internal/game/, cited file:line as tests/test_scenarios.py does) - never from the oracle or the device.  The rules used:

  ORDER   moves are applied in player-id order (processor/action_processor.go:39-41); a player moves iff it was alive when the
          turn started (:57 - Alive changes only in engine.go:140 and stats.go:54,135, all after the moves)
  MOVE    move-all takes army-1, a half move army/2 (core/movement.go:40-49); the source gives them up (:54); onto an own
          tile they are added (:62-66); else they capture iff moved > defender, leaving moved - defender (:69-72), or are
          subtracted (:85).  The move is validated when it is APPLIED (:25, core/action.go:82-89)
  FIRST   a failing move is skipped, the first error is kept and the later moves are still applied
          (processor/action_processor.go:66-77)
  ORDERS  one elimination order per victim, the first captor of its general tile, in capture order; the previous owner of a
          GENERAL tile counts as victim whoever it is (core/movement.go:104-116)
  TURNOVER  per order: the victim's OwnedTiles - its list as of the last stats pass - that it still owns go to the captor
          and join C and V; then Alive = false (engine.go:130-141)
  PASS1   a turn with an order runs a stats pass at once (engine.go:104-108)
  ABORT   an error is returned after that (engine.go:111-113); ProcessTurn then skips production, the end-of-turn pass and
          the game-over check (turn_processor.go:55-57); Turn stays incremented (:125)
  PROD    alive players, every tile of their list: general +1, city +1, normal +1 on turn % 25 == 0; producers join C
          (production_manager.go:27,39-62)
  STATS   nothing to do if C is empty (stats.go:10-14); |C| > N/5 -> full pass: list = ownership (:20-21,33-49); else
          incremental: a player keeps its listed tiles it still owns and gains the tiles of C it owns (:90-130);
          Alive = has a listed general (:54,135); ArmyCount sums the list
  OVER    the game ends when at most one player is alive, who wins (rules/win_conditions.go:40-49), checked at the end of a
          turn that was not aborted (turn_processor.go:176-177)
  FOG     Turn++, then the fog update from last turn's V and the CURRENT lists, then C and V are cleared
          (turn_processor.go:124-135); |V| > N/10 -> every bit cleared and re-lit from the lists of alive players
          (visibility_optimized.go:22-24,33-48), else the 3x3 around every tile of V is cleared and the alive players owning a
          tile within two steps of one are re-lit from their lists (:68-94)

Timeline of a case: reset (turn 0, full passes), pokes of `turn` and `listed`, one warm-up empty turn, the forced turns
(t = 0, 1, ..) and empty turns after them, TURNS in all.  Armies are written as they stand when the forced turn starts: the
builder takes the warm-up's production (PROD: +1 on every owned general and owned listed city) off what it plants.

Army scales (K.a is added to every attacker, K.x to one general that produces in the first turn that is not aborted):
  base   a = 0, x = 0
  cross  a = 60,000: combat near the top of u16; x = 65,533: that general stands at 65,535 and PROD takes it to 65,536 - the env
         is narrow at the load and wide at the store of that turn (a capture can only shrink an army: moved - defender);
         m = 6,000 is added to the army S3 merges into its own tile: there the MOVE phase stores the first wide army
  wide   a = 1,000,000: the env is wide from the reset on
"""
import collections

import numpy as np

import _harness as H
import _oracle as O
import _ordinary_turn as OT
import _state_forms as F
from generalsreinforcementlearning_amd.vec_engine import unpack_legal_bits

N_, G_, C_ = 0, 1, 2
TURNS = 6            # the forced turn and five after it
NOT_OWNED = 3        # core.ErrNotOwned as the C ABI reports it
Scale = collections.namedtuple("Scale", "name a x m")
SCALES = (Scale("base", 0, 0, 0), Scale("cross", 60000, 65533, 6000), Scale("wide", 10 ** 6, 0, 0))
TURN_OFFSETS = (0, 30, 52)     # turn before the warm-up: the eight turns played from each stay off multiples of 25
# increasing seat tuples: the roles of a scenario are numbered in processing order (ORDER), so these relabel it
SEAT_MAPS = {2: {2: [(0, 1)]},
             4: {2: [(0, 1), (1, 3), (2, 3)], 3: [(0, 1, 2), (0, 2, 3), (1, 2, 3)], 4: [(0, 1, 2, 3)]},
             8: {2: [(0, 1), (3, 6), (6, 7)], 3: [(0, 1, 2), (2, 6, 7), (1, 4, 7)], 4: [(0, 1, 2, 3), (1, 3, 6, 7), (4, 5, 6, 7)]}}
PLACEMENTS = ("corner", "edges", "cross_h", "cross_v", "transposed", "small")


class Tl:
    """a role tile: owner role (None: nobody), army when the forced turn starts (int or function of the Scale), type"""

    def __init__(self, role, army, type=N_):
        self.role, self.army, self.type = role, army, type


class Scenario:
    """groups: lists of (name, u, v) - u steps along the placement's direction, v across; groups[0] starts with the
    capturing move's source (0, 0) and target (1, 0).  fillers(N, regime) -> how many army-1 land tiles `filler_role` lists.
    turns: per forced turn a list of (role, source, target, move_all).  regimes: names of the threshold regimes, [None] if
    no fact depends on one; regime_of(N, n_fill) names the regime a board with that many fillers is in.  reward_sign: role ->
    the derived gym reward of the forced turn (a number or a function of the Scale), of which the sign is checked."""
    roles = 2
    groups = ()
    tiles = {}
    unlisted = ()
    turns = ()
    regimes = (None,)
    filler_role = None
    turn0 = None
    single_mover = False
    half_move = False

    def fillers(self, N, regime):
        return 0

    def regime_of(self, N, n_fill):
        return None

    def facts(self, t, v):
        raise NotImplementedError


def line(*names):
    return [(n, i, 0) for i, n in enumerate(names)]


def att(base):
    return lambda K: base + K.a


def gx(base):
    return lambda K: base + K.x


# ---- the nine scenarios of tests/test_scenarios.py --------------------------------------------------------------------
class S1(Scenario):
    """a neutral city captured this turn gets no production this turn"""
    name, single_mover = "s1_capture_no_production", True
    groups = [line("g0", "city"), line("g1")]
    tiles = {"g0": Tl(0, att(5), G_), "city": Tl(None, 2, C_), "g1": Tl(1, gx(2), G_)}
    turns = [[(0, "g0", "city", True)]]

    # reward_sign: the sign of the gym reward of the forced turn (the reference's python/generals_gym/generals_env.py:499-561:
    # +-100 once the game is over, else listed-tile delta + 0.01 * army delta + 50 per opponent that died), per role
    reward_sign = {0: +1, 1: -1}    # role 0: +1 tile, army 5+a -> 2 + 2+a: +0.99.  Role 1: +0.01, -0.1 for sending no move

    def facts(self, t, v):
        a, x = v.K.a, v.K.x
        if t == 0:
            v.eq("err", v.err, 0)
            # MOVE: 4+a move, 4+a > 2 -> capture with 2+a; g0 keeps 1, PROD +1 = 2; the city is not in role 0's list yet
            # (PROD walks the lists of the last pass): still 2+a.  g1: 2+x +1
            v.eq("city", (v.owner("city"), v.army("city")), (0, 2 + a))
            v.eq("generals", (v.army("g0"), v.army("g1")), (2, 3 + x))
            v.eq("listed city", v.listed("city"), 0)      # in C (MOVE), owned by role 0: STATS lists it in either regime
        if t == 1:
            v.eq("city t1", (v.army("city"), v.army("g0")), (3 + a, 3))


class S2(Scenario):
    """a captured city still produces through the loser's stale list"""
    name, single_mover = "s2_stale_list_production", True
    groups = [line("A", "city"), line("g0"), line("g1")]
    tiles = {"A": Tl(0, att(4)), "city": Tl(1, 1, C_), "g0": Tl(0, gx(2), G_), "g1": Tl(1, 2, G_)}
    turns = [[(0, "A", "city", True)]]
    reward_sign = {0: +1, 1: -1}    # role 0: +1 tile, +1 army.  Role 1: a tile less

    def facts(self, t, v):
        if t == 0:
            # MOVE: 3+a vs 1 -> 2+a; PROD: role 1 is alive and still lists the city, the owner is not re-checked: +1
            v.eq("city", (v.owner("city"), v.army("city")), (0, 3 + v.K.a))
            v.eq("listed", v.listed("city"), 0)
            v.eq("g0", v.army("g0"), 3 + v.K.x)


class S3(Scenario):
    """aborted turn (the source was captured earlier in the turn) and the list desync that follows"""
    name = "s3_abort_and_desync"
    groups = [[("A", 0, 0), ("B", 1, 0), ("n", 2, 0), ("A2", 1, 1)], line("g0"), line("g1")]
    # cross scale: B 60,006 + A2's 6,004 = 66,010 - narrow at the load of t = 2, wide at its store, in the move phase
    tiles = {"A": Tl(0, att(10)), "B": Tl(1, 3), "n": Tl(None, 0), "A2": Tl(0, lambda K: 5 + K.m), "g0": Tl(0, 2, G_), "g1": Tl(1, 2, G_)}
    turns = [[(0, "A", "B", True), (1, "B", "n", True)], [], [(0, "A2", "B", True)]]
    reward_sign = {0: 0, 1: 0}      # ABORT without an order: no pass, the counts the reward reads stand still

    def facts(self, t, v):
        a, x, m = v.K.a, 0, v.K.m
        healed = 2 > v.N // 5   # STATS of t = 1: C = the two generals (PROD); a full pass re-lists B for its owner
        if t == 0:
            v.eq("err", v.err, NOT_OWNED)      # role 1 moves from B, which is role 0's by then (MOVE, validated when applied)
            v.eq("turn", v.turn, v.turn_forced)                                   # ABORT: Turn stays incremented
            v.eq("B", (v.owner("B"), v.army("B"), v.army("A")), (0, 6 + a, 1))    # 9+a vs 3
            v.eq("no production", (v.army("g0"), v.army("g1")), (2 + x, 2))       # ABORT
            v.eq("V kept", v.st["vis_changed"][v.e, v.idx("B")], 1)
            v.eq("listed B", v.listed("B"), 1)                                    # no pass: still in role 1's list
            v.eq("n", v.owner("n"), -1)                                           # role 1's move did not happen
        if t == 1:
            v.eq("err", v.err, 0)
            # incremental STATS: B is not in C -> role 1 drops it (not the owner), role 0 does not gain it
            v.eq("listed B", (v.listed("B"), v.owner("B")), (0 if healed else -1, 0))
            # the stats rule: counts follow the list.  g0 3+x, A 1, A2 5; B's 6+a only if listed
            v.eq("counts", (v.tile_count(0), v.army_count(0)), (4, 15 + m + a) if healed else (3, 9 + m))
            v.eq("mask B", any(v.legal_from(0, "B")), healed)                     # rules/legal_moves.go:37 walks the list
            v.eq("mask A2->B", v.legal(0, "A2", "B"), True)
        if t == 2:
            # MOVE onto an own tile: B joins C -> listed again; 6+a + 4
            v.eq("B", (v.listed("B"), v.army("B"), v.army("A2"), v.tile_count(0)), (0, 10 + a + m, 1, 4))
            v.eq("mask B->n", v.legal(0, "B", "n"), True)


class S3b(Scenario):
    """after an aborted turn a captured city produces through the loser's list, which re-lists it for its owner"""
    name = "s3b_stale_city_heals"
    groups = [line("A", "B", "n"), line("g0"), line("g1")]
    tiles = {"A": Tl(0, att(10)), "B": Tl(1, 3, C_), "n": Tl(None, 0), "g0": Tl(0, gx(2), G_), "g1": Tl(1, 2, G_)}
    turns = [[(0, "A", "B", True), (1, "B", "n", True)]]
    reward_sign = {0: 0, 1: 0}      # as S3

    def facts(self, t, v):
        if t == 0:
            v.eq("abort", (v.err, v.army("B")), (NOT_OWNED, 6 + v.K.a))
        if t == 1:
            # PROD through role 1's stale list: +1, B joins C; STATS (either regime) lists it for role 0
            v.eq("B", (v.army("B"), v.owner("B"), v.listed("B")), (7 + v.K.a, 0, 0))


class S5(Scenario):
    """what a victim captures in the turn of its elimination stays with the dead player and never produces"""
    name, roles = "s5_victim_capture", 3
    groups = [line("A", "g1"), line("S", "city"), line("g0"), line("g2")]
    tiles = {"A": Tl(0, att(10)), "g1": Tl(1, 1, G_), "S": Tl(1, att(6)), "city": Tl(None, 2, C_), "g0": Tl(0, 2, G_),
             "g2": Tl(2, gx(2), G_)}
    turns = [[(0, "A", "g1", True), (1, "S", "city", True)]]
    reward_sign = {0: +1, 1: -1, 2: +1}   # role 0: +2 tiles, +50.  Role 1 (the game goes on): 1 tile for 2, 3+a armies for 7+a.  Role 2: +50

    def facts(self, t, v):
        a = v.K.a
        if t == 0:
            v.eq("err", v.err, 0)
            v.eq("alive", (v.alive(0), v.alive(1), v.alive(2), v.done), (1, 0, 1, 0))
            v.eq("g1", (v.owner("g1"), v.army("g1")), (0, 9 + a))     # 9+a vs 1, PASS1 lists it for role 0, PROD +1
            v.eq("S", v.owner("S"), 0)                                # TURNOVER: role 1's listed land
            # ORDER: role 1 still moves; 5+a vs 2.  The city is not in role 1's pre-turn list: TURNOVER leaves it; a dead
            # player's list does not produce
            v.eq("city", (v.owner("city"), v.army("city"), v.listed("city")), (1, 3 + a, 1))
            v.eq("g2", v.army("g2"), 3 + v.K.x)
        if 1 <= t <= 3:
            v.eq("dead city", v.army("city"), 3 + a)


class S6(Scenario):
    """chain elimination, the head of the chain moving first: the middle player comes back to life"""
    name, roles = "s6_chain_head_first", 3
    groups = [line("A", "g1"), line("S", "g2"), line("g0"), line("l1"), line("l2")]
    tiles = {"A": Tl(0, att(10)), "g1": Tl(1, 1, G_), "S": Tl(1, att(10)), "g2": Tl(2, 1, G_), "g0": Tl(0, gx(2), G_),
             "l1": Tl(1, 3), "l2": Tl(2, 4)}
    turns = [[(0, "A", "g1", True), (1, "S", "g2", True)]]
    # only role 2 ends the turn dead: +50 for the others.  Role 0 +3 tiles; role 1 3 -> 2 tiles, 14+a -> 13+a armies: +48.99; role 2 lists nothing
    reward_sign = {0: +1, 1: +1, 2: -1}

    def facts(self, t, v):
        a = v.K.a
        if t == 0:
            # ORDERS [1 -> 0, 2 -> 1].  TURNOVER 1: S, l1 -> role 0 (g1 is role 0's already).  TURNOVER 2: l2 -> role 1.  PASS1: g2 and
            # l2 are in C and role 1's: listed, a general among them -> alive (STATS); role 2 lists nothing
            v.eq("alive", (v.alive(0), v.alive(1), v.alive(2), v.done, v.winner), (1, 1, 0, 0, -1))
            v.eq("S", (v.owner("S"), v.army("S")), (0, 1))
            v.eq("l1", (v.owner("l1"), v.army("l1")), (0, 3))
            v.eq("l2", (v.owner("l2"), v.army("l2")), (1, 4))
            v.eq("g1", (v.owner("g1"), v.army("g1")), (0, 9 + a))     # 9+a vs 1 -> 8+a, PROD +1
            v.eq("g2", (v.owner("g2"), v.army("g2")), (1, 9 + a))     # role 1 is alive again when PROD runs
            v.eq("g0", v.army("g0"), 3 + v.K.x)
            v.eq("general_idx", (v.general(1), v.general(2)), ("g2", None))
            assert v.general(0) in ("g0", "g1"), v.ctx("general_idx of role 0")   # two generals: Go map order


class S7(Scenario):
    """the fog lags one turn behind ownership"""
    name, single_mover = "s7_fog_lag", True
    groups = [line("A", "B", "Cc"), line("g0"), line("g1"), line("l1")]
    tiles = {"A": Tl(0, att(5)), "B": Tl(None, 0), "Cc": Tl(None, 0), "g0": Tl(0, gx(2), G_), "g1": Tl(1, 2, G_), "l1": Tl(1, 3)}
    turns = [[(0, "A", "B", True)]]
    reward_sign = {0: +1, 1: -1}    # +1 tile (an empty one), +1 army from g0.  Role 1: +0.01, -0.1 for sending no move

    def facts(self, t, v):
        beyond = [v.idx("Cc")] + v.across("Cc", 0, ("B",))     # the column that only a tile at B lights
        if t == -1:
            v.eq("before", (v.vis_at(v.idx("B"), 0), [v.vis_at(i, 0) for i in beyond]), (True, [False] * len(beyond)))
        if t == 0:
            # FOG ran before the move, from the lists of the turn before
            v.eq("owner B", v.owner("B"), 0)
            v.eq("not lit yet", [v.vis_at(i, 0) for i in beyond], [False] * len(beyond))
        if t == 1:
            # V = {B}; role 0 lists B since STATS of t = 0: lit from it by the incremental and by the full update alike
            v.eq("lit", [v.vis_at(i, 0) for i in beyond], [True] * len(beyond))
            v.eq("role 1 never near", v.vis_at(v.idx("B"), 1), False)


class S7b(Scenario):
    """the loser of a tile keeps seeing around it until the next turn's fog update"""
    name, single_mover = "s7b_loser_sees_one_more_turn", True
    groups = [line("A", "B", "Cc"), line("g0"), line("g1")]
    tiles = {"A": Tl(0, att(9)), "B": Tl(1, 1), "Cc": Tl(None, 0), "g0": Tl(0, gx(2), G_), "g1": Tl(1, 2, G_)}
    turns = [[(0, "A", "B", True)]]
    reward_sign = {0: +1, 1: -1}    # +1 tile; armies 9+a + 2 -> 1 + 7+a + 3: unchanged.  Role 1: a tile less

    def facts(self, t, v):
        if t in (-1, 0):
            v.eq("loser sees", v.vis_at(v.idx("Cc"), 1), True)
        if t == 1:
            # V = {B}: cleared around B; role 1 lists nothing in range any more (pairs are kept apart), role 0 lists B
            v.eq("after", (v.vis_at(v.idx("Cc"), 1), v.vis_at(v.idx("Cc"), 0)), (False, True))


class Thresholds(Scenario):
    """|C| > N/5 forces a full pass: a growth turn heals a desynced tile nobody touched - or does not"""
    name, regimes, filler_role, turn0 = "full_update_thresholds", ("incremental", "full"), 0, 21
    groups = S3.groups
    tiles = S3.tiles
    turns = S3.turns[:1]
    reward_sign = S3.reward_sign

    # growth turn (t = 2, turn 25): C = what PROD touched = role 0's listed A, A2 and fillers, g0, g1 (B is listed by nobody
    # since t = 1: it does not produce) -> |C| = 4 + fillers
    def fillers(self, N, regime):
        return max(0, N // 5 - 3) if regime == "full" else 0

    def regime_of(self, N, n_fill):
        return "full" if 4 + n_fill > N // 5 else "incremental"

    def facts(self, t, v):
        if t == 0:
            v.eq("abort", v.err, NOT_OWNED)
        if t == 1 and 2 <= v.N // 5:
            v.eq("dropped", v.listed("B"), -1)     # S3, t = 1
        if t == 2:
            v.eq("turn", v.turn, 25)
            v.eq("B", (v.listed("B"), v.army("B")), (0 if v.regime == "full" else -1, 6 + v.K.a))   # unlisted: did not grow
            v.eq("filler grew", [v.st["army"][v.e, i] for i in v.case.filler_idx], [2] * len(v.case.filler_idx))


# ---- new scenarios ----------------------------------------------------------------------------------------------------
class S6Mid(Scenario):
    """S6 in the other processing order: roles M(0), H(1), T(2) - the middle player's seat is below its captor's, so it
    captures the tail's general BEFORE its own falls"""
    name, roles = "s6_chain_middle_first", 3
    groups = [line("aM", "gT"), line("aH", "gM"), line("gH"), line("lM"), line("lT")]
    tiles = {"aM": Tl(0, att(10)), "gT": Tl(2, 1, G_), "aH": Tl(1, att(10)), "gM": Tl(0, 1, G_), "gH": Tl(1, gx(2), G_),
             "lM": Tl(0, 3), "lT": Tl(2, 4)}
    turns = [[(0, "aM", "gT", True), (1, "aH", "gM", True)]]
    reward_sign = {0: +1, 1: +1, 2: -1}   # as S6: M +50 -1 tile -0.01, H +50 +3 tiles, T lists nothing

    def facts(self, t, v):
        a = v.K.a
        if t == 0:
            # captures in order: gT by M (9+a vs 1), gM by H (9+a vs 1) -> ORDERS [T -> M, M -> H].  TURNOVER 1: T's list {gT, lT}: gT
            # is M's already, lT -> M.  TURNOVER 2: M's PRE-TURN list {gM, aM, lM}: gM is H's, aM and lM -> H; gT and lT are M's
            # but not in that list: they stay.  PASS1: M keeps nothing of its list and gains gT, lT from C: a general -> alive
            v.eq("alive M H T", (v.alive(0), v.alive(1), v.alive(2), v.done, v.winner), (1, 1, 0, 0, -1))
            v.eq("gT", (v.owner("gT"), v.army("gT"), v.listed("gT")), (0, 9 + a, 0))    # 8+a, PROD +1: M alive at PROD
            v.eq("lT", (v.owner("lT"), v.army("lT"), v.listed("lT")), (0, 4, 0))
            v.eq("gM", (v.owner("gM"), v.army("gM")), (1, 9 + a))
            v.eq("aM", (v.owner("aM"), v.army("aM")), (1, 1))
            v.eq("lM", (v.owner("lM"), v.army("lM")), (1, 3))
            v.eq("gH", v.army("gH"), 3 + v.K.x)
            v.eq("general_idx", (v.general(0), v.general(2)), ("gT", None))
            v.eq("counts M", (v.tile_count(0), v.army_count(0)), (2, 13 + a))
        if t == 1:
            v.eq("gT t1", v.army("gT"), 10 + a)


class Chain3(Scenario):
    """a three-link chain: 0 takes 1's general, 1 takes 2's, 2 takes 3's, all in one turn"""
    name, roles = "chain_three_links", 4
    groups = [line("a0", "g1"), line("a1", "g2"), line("a2", "g3"), line("g0"), line("l1"), line("l3")]
    tiles = {"a0": Tl(0, att(10)), "g1": Tl(1, 1, G_), "a1": Tl(1, att(10)), "g2": Tl(2, 1, G_), "a2": Tl(2, att(10)),
             "g3": Tl(3, 1, G_), "g0": Tl(0, gx(2), G_), "l1": Tl(1, 3), "l3": Tl(3, 4)}
    turns = [[(0, "a0", "g1", True), (1, "a1", "g2", True), (2, "a2", "g3", True)]]
    # only role 3 ends the turn dead: +50 for the others.  Role 0 +3 tiles; role 1 3 -> 2 tiles, 14+a -> 10+a: +48.96; role 2 2 -> 2 tiles,
    # 11+a -> 13+a: +50.02; role 3 lists nothing, -0.1 for sending no move
    reward_sign = {0: +1, 1: +1, 2: +1, 3: -1}

    def facts(self, t, v):
        a = v.K.a
        if t == 0:
            # ORDERS [1 -> 0, 2 -> 1, 3 -> 2].  TURNOVER 1: role 1's list {g1, a1, l1}: g1 is role 0's; a1, l1 -> 0.  TURNOVER 2: role 2's
            # list {g2, a2}: g2 is role 1's; a2 -> role 1 (after role 1's own turnover: it stays).  TURNOVER 3: role 3's list
            # {g3, l3}: g3 is role 2's; l3 -> 2.  PASS1 from C: role 1 gains g2, a2; role 2 gains g3, l3: both hold a general
            v.eq("alive", [v.alive(r) for r in range(4)] + [v.done, v.winner], [1, 1, 1, 0, 0, -1])
            v.eq("g1", (v.owner("g1"), v.army("g1")), (0, 9 + a))
            v.eq("g2", (v.owner("g2"), v.army("g2")), (1, 9 + a))
            v.eq("g3", (v.owner("g3"), v.army("g3")), (2, 9 + a))
            v.eq("a1 l1", (v.owner("a1"), v.army("a1"), v.owner("l1")), (0, 1, 0))
            v.eq("a2", (v.owner("a2"), v.army("a2")), (1, 1))
            v.eq("l3", (v.owner("l3"), v.army("l3")), (2, 4))
            v.eq("a0 g0", (v.owner("a0"), v.army("a0"), v.army("g0")), (0, 1, 3 + v.K.x))
            v.eq("general_idx", [v.general(r) for r in (1, 2, 3)], ["g2", "g3", None])
            v.eq("counts", [(v.tile_count(r), v.army_count(r)) for r in range(4)],
                 [(5, 3 + v.K.x + 1 + 9 + a + 1 + 3), (2, 10 + a), (2, 13 + a), (0, 0)])


class Mutual(Scenario):
    """two players take each other's general in one turn: they swap seats of power and both live"""
    name = "mutual_capture"
    groups = [line("a0", "g1"), line("a1", "g0")]
    tiles = {"a0": Tl(0, att(10)), "g1": Tl(1, 2, G_), "a1": Tl(1, att(12)), "g0": Tl(0, 3, G_)}
    turns = [[(0, "a0", "g1", True), (1, "a1", "g0", True)]]
    reward_sign = {0: -1, 1: -1}    # nobody died, 2 tiles each before and after; armies 13+a -> 9+a and 14+a -> 10+a: -0.04 each
    bystander = None

    def facts(self, t, v):
        a, x = v.K.a, v.K.x
        if t == 0:
            # ORDER: both were alive at the start, both move.  a0: 9+a vs 2 -> 7+a.  a1: 11+a vs 3 -> 8+a.  ORDERS [1 -> 0, 0 -> 1].
            # TURNOVER 1: role 1's list {g1, a1}: g1 is role 0's, a1 -> 0.  TURNOVER 2: role 0's pre-turn list {g0, a0}: g0 is role
            # 1's, a0 -> 1 (g1, a1 are not in that list: they stay role 0's).  PASS1: role 0 gains g1, a1 from C, role 1 gains
            # g0, a0: each lists a general -> both alive (STATS), nobody is out, the game goes on (OVER)
            v.eq("alive", (v.alive(0), v.alive(1), v.done, v.winner), (1, 1, 0, -1))
            v.eq("g1", (v.owner("g1"), v.army("g1"), v.listed("g1")), (0, 8 + a, 0))     # PROD +1
            v.eq("g0", (v.owner("g0"), v.army("g0"), v.listed("g0")), (1, 9 + a, 1))
            v.eq("a0", (v.owner("a0"), v.army("a0")), (1, 1))
            v.eq("a1", (v.owner("a1"), v.army("a1")), (0, 1))
            v.eq("general_idx", (v.general(0), v.general(1)), ("g1", "g0"))
            if self.bystander:
                v.eq("bystander", (v.alive(2), v.army(self.bystander)), (1, 3 + x))
        if t == 1:
            v.eq("t1", (v.army("g1"), v.army("g0"), v.done), (9 + a, 10 + a, 0))


class Mutual3(Mutual):
    name, roles, bystander = "mutual_capture_3p", 3, "g2"
    reward_sign = {0: -1, 1: -1, 2: -1}   # the bystander: +0.01 for its general, -0.1 for sending no move
    groups = Mutual.groups + [line("g2")]
    tiles = dict(Mutual.tiles, g2=Tl(2, gx(2), G_))


class TwoOnOne(Scenario):
    """two players attack the same general in one turn: the first captor is eliminated by the second"""
    name, roles = "two_attackers_one_general", 3
    groups = [[("a0", 0, 0), ("gV", 1, 0), ("a1", 2, 0)], line("g0"), line("g1"), line("lV")]
    tiles = {"a0": Tl(0, att(10)), "gV": Tl(2, 1, G_), "a1": Tl(1, att(12)), "g0": Tl(0, 2, G_), "g1": Tl(1, gx(2), G_), "lV": Tl(2, 3)}
    turns = [[(0, "a0", "gV", True), (1, "a1", "gV", True)]]
    reward_sign = {0: -1, 1: +1, 2: -1}   # over: +100 for the winner, -100 for the others
    over = True

    def facts(self, t, v):
        a = v.K.a
        if t == 0:
            # a0: 9+a vs 1 -> gV is role 0's with 8+a.  a1: 11+a vs 8+a -> role 1's with 3.  Both captures are of a GENERAL tile with a
            # previous owner other than the captor: ORDERS [V -> 0, 0 -> 1].  TURNOVER 1: V's list {gV, lV}: gV is role 1's; lV -> 0.
            # TURNOVER 2: role 0's pre-turn list {g0, a0} -> role 1; lV is not in it: it stays role 0's.  PASS1: role 0 keeps nothing
            # and gains lV from C: no general -> dead.  Role 1 lists g1, a1, gV, g0, a0
            v.eq("alive 0 1 V", (v.alive(0), v.alive(1), v.alive(2)), (0, 1, 0))
            v.eq("gV", (v.owner("gV"), v.army("gV")), (1, 4))                     # PROD +1
            v.eq("g0", (v.owner("g0"), v.army("g0"), v.listed("g0")), (1, 3, 1))  # listed by role 1 since PASS1: PROD +1
            v.eq("a0", (v.owner("a0"), v.army("a0")), (1, 1))
            v.eq("lV", (v.owner("lV"), v.army("lV"), v.listed("lV")), (0, 3, 0))
            v.eq("g1", v.army("g1"), 3 + v.K.x)
            v.eq("counts 0", (v.tile_count(0), v.army_count(0), v.general(0)), (1, 3, None))
            # OVER: one player alive - unless a bystander lives
            v.eq("over", (v.done, v.winner), (1, 1) if self.over else (0, -1))
        if t == 1 and not self.over:
            v.eq("dead land", (v.army("lV"), v.army("gV"), v.army("g0")), (3, 5, 4))


class TwoOnOne4(TwoOnOne):
    name, roles, over = "two_attackers_one_general_4p", 4, False
    # the game goes on: role 0 +50 (V died) -1 tile, armies 12+a -> 3; role 1 +100 +3 tiles, armies 14+a+x -> 12+x (its attackers
    # are spent in the two combats); V +50 (role 0 died) -2 tiles -4 armies, -0.1 for sending no move.  Values, of which the sign counts
    reward_sign = {0: lambda K: 49 - 0.01 * (9 + K.a), 1: lambda K: 103 - 0.01 * (2 + K.a), 2: 50 - 2 - 0.04 - 0.1,
                   3: 50 + 50 + 0.01 - 0.1}      # the bystander: two deaths, its general's army, no move sent
    groups = TwoOnOne.groups + [line("g3")]
    tiles = dict(TwoOnOne.tiles, g3=Tl(3, 2, G_))


class Turnover(Scenario):
    """a general falls to a player the game goes on for; the turnover puts the victim's land into C - below and above N/5"""
    name, roles, single_mover = "capture_game_goes_on", 3, True
    regimes, filler_role = ("below", "above"), 1
    groups = [line("a0", "g1"), line("g0"), line("g2"), line("U")]
    tiles = {"a0": Tl(0, att(10)), "g1": Tl(1, 1, G_), "g0": Tl(0, 2, G_), "g2": Tl(2, gx(2), G_), "U": Tl(1, 3)}
    unlisted = ("U",)       # role 1 owns U without listing it (the state S3 leaves behind)
    turns = [[(0, "a0", "g1", True)]]
    reward_sign = {0: +1, 1: -1, 2: +1}   # role 0: +50 and the victim's land.  Role 1: its list is gone.  Role 2: +50

    # the warm-up's and every later empty turn's C is the three generals (PROD): incremental needs 3 <= N/5 (regime_of checks
    # it), so U stays unlisted up to the forced turn.  There C = {a0, g1} + the fillers TURNOVER hands over: PASS1 sees 2 + F,
    # the end-of-turn pass 4 + F (g0, g2 produced)
    def fillers(self, N, regime):
        return N // 5 if regime == "above" else 1

    def regime_of(self, N, n_fill):
        if N // 5 < 3:
            return "unseatable"
        return "above" if 2 + n_fill > N // 5 else "below" if 4 + n_fill <= N // 5 else "mixed"

    def facts(self, t, v):
        a = v.K.a
        F_ = len(v.case.filler_idx)
        above, has_u = v.regime == "above", "U" in self.tiles
        if t == -1 and has_u:
            v.eq("U before", (v.owner("U"), v.listed("U")), (1, -1))
        if t == 0:
            v.eq("alive", (v.alive(0), v.alive(1), v.alive(2), v.done, v.winner, v.err), (1, 0, 1, 0, -1, 0))
            v.eq("g1", (v.owner("g1"), v.army("g1"), v.listed("g1")), (0, 9 + a, 0))
            v.eq("fillers", sorted(set((int(v.st["owner"][v.e, i]), int(v.st["listed"][v.e, i]), int(v.st["army"][v.e, i]))
                                       for i in v.case.filler_idx)), [(v.seat(0), v.seat(0), 1)])
            # U is not in role 1's list: TURNOVER leaves it.  Incremental passes never see it (not in C); a full pass lists it for its
            # owner, the dead role 1, whose counts then follow its list (the stats rule)
            if has_u:
                v.eq("U", (v.owner("U"), v.army("U"), v.listed("U")), (1, 3, 1 if above else -1))
            v.eq("counts 1", (v.tile_count(1), v.army_count(1), v.general(1)), (1, 3, None) if above and has_u else (0, 0, None))
            v.eq("counts 0", (v.tile_count(0), v.army_count(0)), (3 + F_, 3 + 1 + 9 + a + F_))
            v.eq("g2", v.army("g2"), 3 + v.K.x)
        if t >= 1:
            # later turns: C = the living generals g0, g1, g2 -> incremental (3 <= N/5): nothing changes for U
            if has_u:
                v.eq("U later", (v.owner("U"), v.army("U"), v.listed("U")), (1, 3, 1 if above else -1))
            v.eq("g1 later", v.army("g1"), 9 + a + t)


class TurnoverListed(Turnover):
    """the same capture with lists equal to ownership: every fact is the same in both regimes, and a narrow env may enter the
    forced turn - with its turnover below or above N/5 - on the ordinary path (an unlisted tile bars it: HF_LDIFF)"""
    name = "capture_game_goes_on_lists_match"
    groups = Turnover.groups[:-1]
    tiles = {n: tl for n, tl in Turnover.tiles.items() if n != "U"}
    unlisted = ()


class AbortAfterFall(Scenario):
    """a move fails later in a turn in which a general has already fallen: the elimination stands, the turn's rest is skipped
    - the game-over check included"""
    name = "abort_after_general_fell"
    groups = [line("a0", "g1", "n"), line("g0"), line("l1")]
    # g1 holds 2: a move from it is legal when the turn starts (an env that takes action indices refuses any other)
    tiles = {"a0": Tl(0, att(10)), "g1": Tl(1, 2, G_), "n": Tl(None, 0), "g0": Tl(0, gx(2), G_), "l1": Tl(1, 3)}
    turns = [[(0, "a0", "g1", True), (1, "g1", "n", True)]]
    reward_sign = {0: +1, 1: -1}    # the game is not over (ABORT): role 0 +2 tiles +50, role 1 lists nothing any more

    def facts(self, t, v):
        a, x = v.K.a, v.K.x
        if t == 0:
            # a0: 9+a vs 2 -> g1 is role 0's, 7+a.  Role 1 (alive at the start, ORDER) moves from g1: not its tile any more -> ErrNotOwned,
            # skipped (FIRST).  ORDERS [1 -> 0], TURNOVER: l1 -> 0, role 1 dead, PASS1 lists g1 and l1 for role 0.  ABORT: no PROD, no
            # end-of-turn pass, NO game-over check: one player alive and the game not over
            v.eq("err", v.err, NOT_OWNED)
            v.eq("alive", (v.alive(0), v.alive(1), v.done, v.winner), (1, 0, 0, -1))
            v.eq("g1", (v.owner("g1"), v.army("g1"), v.listed("g1")), (0, 7 + a, 0))
            v.eq("l1", (v.owner("l1"), v.listed("l1")), (0, 0))
            v.eq("no production", v.army("g0"), 2 + x)
            v.eq("n", v.owner("n"), -1)
            v.eq("counts", (v.tile_count(0), v.army_count(0), v.tile_count(1)), (4, 2 + x + 1 + 7 + a + 3, 0))
            v.eq("turn", v.turn, v.turn_forced)
        if t == 1:
            # the next turn is played (the game is not over): PROD g0, g1 +1, then OVER: role 0 wins
            v.eq("t1", (v.err, v.army("g0"), v.army("g1"), v.done, v.winner), (0, 3 + x, 8 + a, 1, 0))


class LaterMovesApply(Scenario):
    """a move whose source changed owner earlier in the turn fails - and the moves after it are still applied"""
    name, roles, half_move = "source_changed_owner", 3, True
    groups = [line("h", "m"), line("A", "B", "n"), line("g0"), line("g1"), line("g2")]     # the half move is the placed one
    tiles = {"A": Tl(0, att(10)), "B": Tl(1, 3), "n": Tl(None, 0), "h": Tl(2, att(7)), "m": Tl(None, 0),
             "g0": Tl(0, gx(2), G_), "g1": Tl(1, 2, G_), "g2": Tl(2, 2, G_)}
    turns = [[(0, "A", "B", True), (1, "B", "n", True), (2, "h", "m", False)]]
    reward_sign = {0: 0, 1: 0, 2: 0}      # ABORT without an order: no pass, the counts stand still

    def facts(self, t, v):
        a = v.K.a
        if t == 0:
            # role 0: 9+a vs 3 -> B is its with 6+a.  Role 1 from B: ErrNotOwned, kept as the turn's error, the loop goes on (FIRST).
            # Role 2's half move: (7+a)/2 = 3 + a/2 (a even) leave, 4 + a/2 stay; 3 + a/2 > 0 -> m captured.  ABORT: no PROD, no pass
            v.eq("err", v.err, NOT_OWNED)
            v.eq("B", (v.owner("B"), v.army("B"), v.listed("B")), (0, 6 + a, 1))
            v.eq("n", v.owner("n"), -1)
            v.eq("h m", (v.army("h"), v.owner("m"), v.army("m"), v.listed("m")), (4 + a // 2, 2, 3 + a // 2, -1))
            v.eq("no production", (v.army("g0"), v.army("g1"), v.army("g2")), (2 + v.K.x, 2, 2))
        if t == 1 and 3 <= v.N // 5:
            # C = the three generals: incremental: B dropped by role 1, m still listed by nobody
            v.eq("t1", (v.listed("B"), v.listed("m"), v.army("g0")), (-1, -1, 3 + v.K.x))


SCENARIOS = [S1(), S2(), S3(), S3b(), S5(), S6(), S7(), S7b(), Thresholds(), S6Mid(), Chain3(), Mutual(), Mutual3(), TwoOnOne(),
             TwoOnOne4(), Turnover(), AbortAfterFall(), LaterMovesApply(), TurnoverListed()]
BY_NAME = {s.name: s for s in SCENARIOS}


# ---- placement ----------------------------------------------------------------------------------------------------------
def _group_cells(group, ax, ay, d, side=1):
    dx, dy = d
    px, py = (0, side) if dy == 0 else (side, 0)      # across the line, towards growing (side 1) or falling coordinates
    return {n: (ax + u * dx + v * px, ay + u * dy + v * py) for n, u, v in group}


def _fits(cells, w, h, taken, sep=2):
    for x, y in cells.values():
        if not (0 <= x < w and 0 <= y < h):
            return False
        for tx, ty in taken:
            if max(abs(tx - x), abs(ty - y)) < sep:
                return False
    return len(set(cells.values())) == len(cells)


def _first_anchor(kind, group, w, h):
    """candidate (x, y, direction) for the capturing group under a placement kind: the move is group[0] -> group[1]"""
    n = w * h
    if kind in ("corner", "small"):
        return [(0, 0, (1, 0)), (0, 0, (0, 1))]
    if kind == "transposed":
        return [(0, 0, (0, 1))] if w != h else []
    if kind == "edges":
        return [(w - 2, h - 1, (1, 0)), (w - 1, h - 1, (-1, 0))]     # on the last row, into or out of the last corner
    out = []
    for k in range(1, (n + 63) // 64):
        b = 64 * k
        if kind == "cross_h" and b % w != 0 and b < n:
            out += [((b - 1) % w, (b - 1) // w, (1, 0)), (b % w, b // w, (-1, 0))]
        if kind == "cross_v":
            for t in range(b - 1, max(b - w, 0) - 1, -1):      # t < 64k <= t + w
                if t + w < n:
                    out += [(t % w, t // w, (0, 1)), (t % w, t // w + 1, (0, -1))]
                    break
    return out


def place(sc, kind, w, h, n_fill):
    """name -> (x, y) and the filler tiles, or None if the scenario does not fit the board this way"""
    for ax, ay, d, side in [c + (s,) for c in _first_anchor(kind, sc.groups[0], w, h) for s in (1, -1)]:
        cells = _group_cells(sc.groups[0], ax, ay, d, side)
        if not _fits(cells, w, h, []):
            continue
        placed, taken, ok = dict(cells), list(cells.values()), True
        dirs = [(0, 1), (1, 0)] if kind == "transposed" else [(1, 0), (0, 1)]
        for gi, grp in enumerate(sc.groups[1:]):
            found = None
            if kind == "edges" and gi == 0:      # the second group on the last column
                cand = [(w - 1, 0, (0, 1))]
            else:
                cand = []
            cand += [(x, y, dd) for y in range(h) for x in range(w) for dd in (dirs if len(grp) > 1 else dirs[:1])]
            for x, y, dd in cand:
                c = _group_cells(grp, x, y, dd)
                if _fits(c, w, h, taken):
                    found = c
                    break
            if found is None:
                ok = False
                break
            placed.update(found)
            taken += list(found.values())
        if not ok:
            continue
        fill = []
        for t in range(w * h - 1, -1, -1):
            if len(fill) == n_fill:
                break
            if _fits({"f": (t % w, t // w)}, w, h, taken):
                fill.append((t % w, t // w))
        if len(fill) == n_fill:
            return placed, fill
    return None


def crossing(case):
    """'h' / 'v' if the capturing move joins tiles 64k-1.. and 64k.. of two register rows, else None"""
    s, t = (case.idx(n) for n in (case.sc.groups[0][0][0], case.sc.groups[0][1][0]))
    if s // 64 == t // 64:
        return None
    return "h" if abs(s - t) == 1 else "v"


# ---- cases and batches --------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, sc, kind, w, h, seats, K, regime, turn0, cells, fill):
        self.sc, self.kind, self.w, self.h, self.seats, self.K, self.regime, self.cells = sc, kind, w, h, seats, K, regime, cells
        self.players = max(seats) + 1
        self.turn0 = sc.turn0 if sc.turn0 is not None else turn0
        self.filler_idx = [y * w + x for x, y in fill]
        self.id = f"{sc.name}/{kind}/{w}x{h}/seats{''.join(map(str, seats))}/{K.name}" + (f"/{regime}" if regime else "")

    def idx(self, name):
        x, y = self.cells[name]
        return y * self.w + x

    def planes(self, stride):
        army, owner, typ = np.zeros(stride, np.int32), np.full(stride, -1, np.int8), np.zeros(stride, np.uint8)
        for name, tl in self.sc.tiles.items():
            i = self.idx(name)
            a = tl.army(self.K) if callable(tl.army) else tl.army
            if tl.role is not None and tl.type in (G_, C_) and name not in self.sc.unlisted:
                a -= 1      # the warm-up turn's production
            assert a >= 0
            army[i], typ[i] = a, tl.type
            owner[i] = -1 if tl.role is None else self.seats[tl.role]
        for i in self.filler_idx:
            army[i], owner[i] = 1, self.seats[self.sc.filler_role]
        return army, owner, typ

    def actions(self, t, max_p):
        row = np.zeros(max_p, O.ACTION_DTYPE)
        if t < len(self.sc.turns):
            for role, s, d, move_all in self.sc.turns[t]:
                (fx, fy), (tx, ty) = self.cells[s], self.cells[d]
                row[self.seats[role]] = (fx, fy, tx, ty, 1 | (0 if move_all else 2), (0, 0, 0))
        return row


class View:
    """the state of one case after turn t (t = -1: after the warm-up), in roles and tile names"""

    def __init__(self, case, e, st, err, bits, t):
        self.case, self.e, self.st, self.err, self.bits, self.t = case, e, st, None if err is None else int(err[e]), bits, t
        self.K, self.N, self.regime = case.K, case.w * case.h, case.regime
        self.role_of = {s: r for r, s in enumerate(case.seats)}
        self.turn = int(st["turn"][e])
        self.turn_forced = case.turn0 + 2
        self.done, self.fails = int(st["done"][e]), []

    def ctx(self, what):
        return f"{self.case.id} t={self.t}: {what}"

    def eq(self, what, got, want):
        norm = lambda z: [norm(i) for i in z] if isinstance(z, (tuple, list)) else (z if z is None or isinstance(z, str) else int(z))
        if norm(got) != norm(want):
            self.fails.append(f"{what}: got {norm(got)}, derived {norm(want)}")

    def idx(self, name):
        return self.case.idx(name)

    def seat(self, role):
        return self.case.seats[role]

    def _role(self, s):
        s = int(s)
        return -1 if s < 0 else self.role_of.get(s, 100 + s)

    def army(self, name):
        return int(self.st["army"][self.e, self.idx(name)])

    def owner(self, name):
        return self._role(self.st["owner"][self.e, self.idx(name)])

    def listed(self, name):
        return self._role(self.st["listed"][self.e, self.idx(name)])

    def alive(self, role):
        return int(self.st["alive"][self.e, self.seat(role)])

    @property
    def winner(self):
        return self._role(self.st["winner"][self.e])

    def tile_count(self, role):
        return int(self.st["tile_count"][self.e, self.seat(role)])

    def army_count(self, role):
        return int(self.st["army_count"][self.e, self.seat(role)])

    def general(self, role):
        g = int(self.st["general_idx"][self.e, self.seat(role)])
        if g < 0:
            return None
        names = [n for n in self.case.cells if self.case.idx(n) == g]
        return names[0] if names else g

    def vis_at(self, i, role):
        return bool(int(self.st["visible"][self.e, i]) >> self.seat(role) & 1)

    def across(self, name, role, but):
        """the in-board tiles beside `name`, across the direction of its group's line, that no tile planted for `role` lights
        (the 3x3 of FOG) - `but` apart"""
        grp = next(g for g in self.case.sc.groups if any(n == name for n, _, _ in g))
        (x0, y0), (x1, y1) = self.case.cells[grp[0][0]], self.case.cells[grp[1][0]]
        px, py = (0, 1) if y0 == y1 else (1, 0)
        x, y = self.case.cells[name]
        mine = [self.case.cells[n] for n, tl in self.case.sc.tiles.items() if tl.role == role and n not in but]
        out = [(x + s * px, y + s * py) for s in (-1, 1) if 0 <= x + s * px < self.case.w and 0 <= y + s * py < self.case.h]
        return [cy * self.case.w + cx for cx, cy in out if all(max(abs(cx - mx), abs(cy - my)) > 1 for mx, my in mine)]

    def _mask(self, role):
        return unpack_legal_bits(self.bits[self.e, self.seat(role)], self.case.w, self.case.h)

    def legal_from(self, role, name):
        i = self.idx(name)
        return [bool(b) for b in self._mask(role)[4 * i:4 * i + 4]]

    def legal(self, role, s, d):
        (fx, fy), (tx, ty) = self.case.cells[s], self.case.cells[d]
        k = {(0, -1): 0, (1, 0): 1, (0, 1): 2, (-1, 0): 3}[(tx - fx, ty - fy)]
        return self.legal_from(role, s)[k]


def small_dims(mw, mh):
    return max(3, mw - 3), max(3, mh - 2)     # tests/_harness.py variant_batch's ragged board


def variant_cases(maxp, slots, parity, mover_on_seat_0=False):
    """mover_on_seat_0: the matrix of the single-mover scenarios alone, for a kernel that takes one learner seat: full-size
    boards, seat maps that begin with seat 0.  Else every case of the <maxp, slots, parity> handle: each scenario its roles can be seated for, under every placement that
    fits; seat maps, army scales, regimes and turn offsets are dealt round so that the matrix as a whole uses all of them"""
    mw, mh = H.VARIANT_DIMS[(slots, parity)]
    vi = sorted(H.VARIANT_DIMS).index((slots, parity)) + {2: 0, 4: 1, 8: 2}[maxp]
    cases = []
    for si, sc in enumerate(SCENARIOS):
        maps = SEAT_MAPS[maxp].get(sc.roles)
        if mover_on_seat_0:
            maps = [m for m in maps or [] if m[0] == 0] if sc.single_mover else None
        if not maps:
            continue
        for ki, kind in enumerate(PLACEMENTS):
            w, h = small_dims(mw, mh) if kind == "small" else (mw, mh)
            if kind == "small" and ((w, h) == (mw, mh) or mover_on_seat_0):
                continue
            k = si + ki + vi
            regime = sc.regimes[k % len(sc.regimes)]
            n_fill = sc.fillers(w * h, regime)
            if sc.regime_of(w * h, n_fill) != regime:
                regime = sc.regimes[(k + 1) % len(sc.regimes)]
                n_fill = sc.fillers(w * h, regime)
                if sc.regime_of(w * h, n_fill) != regime:
                    continue
            got = place(sc, kind, w, h, n_fill)
            if got is None:
                continue
            cases.append(Case(sc, kind, w, h, maps[k % len(maps)], SCALES[(k + ki) % 3], regime, TURN_OFFSETS[(k // 3) % 3], *got))
    return mw, mh, cases


N_GENERATED = 3      # generated boards played by the oracle's agent beside the cases


class Batch:
    """the cases of one handle and a few generated envs, as planes and per-turn action arrays"""

    def __init__(self, maxp, slots, parity, only=None, mover_on_seat_0=False):
        mw, mh, cases = variant_cases(maxp, slots, parity, mover_on_seat_0)
        _, _, sizes = H.variant_batch(maxp, slots, parity, N_GENERATED + 1)
        self.fill(maxp, (maxp, slots, parity), mw, mh, [c for c in cases if only is None or only(c)], sizes[1:], 900 + slots)

    @classmethod
    def of_cases(cls, maxp, key, mw, mh, cases):
        """a batch of the given cases alone on a handle of mw x mh"""
        self = cls.__new__(cls)
        self.fill(maxp, key, mw, mh, cases, [], 0)
        return self

    def fill(self, maxp, key, mw, mh, cases, sizes, seed):
        """sizes: (w, h, players) of the generated boards beside the cases"""
        self.maxp, self.key, self.mw, self.mh, self.cases = maxp, key, mw, mh, cases
        n, stride = len(self.cases), self.mw * self.mh
        self.B = n + len(sizes)
        ga, go, gt, gw, gh, gp = H.gen_boards(seed, sizes, self.mw, self.mh)
        self.army = np.concatenate([np.zeros((n, stride), np.int32), ga])
        self.owner = np.concatenate([np.full((n, stride), -1, np.int8), go])
        self.typ = np.concatenate([np.zeros((n, stride), np.uint8), gt])
        self.w = np.concatenate([np.array([c.w for c in self.cases], np.int32), gw])
        self.h = np.concatenate([np.array([c.h for c in self.cases], np.int32), gh])
        self.p = np.concatenate([np.array([c.players for c in self.cases], np.int32), gp])
        for e, c in enumerate(self.cases):
            self.army[e, :c.w * c.h], self.owner[e, :c.w * c.h], self.typ[e, :c.w * c.h] = c.planes(c.w * c.h)
        self.turn = np.concatenate([np.array([c.turn0 for c in self.cases], np.int32), np.zeros(len(sizes), np.int32)]).astype(np.int32)

    def pokes(self, st):
        """write_state arrays from the state after the reset: turn offsets and the tiles a role owns without listing"""
        listed = st["listed"].copy()
        for e, c in enumerate(self.cases):
            for name in c.sc.unlisted:
                listed[e, c.idx(name)] = -1
        return {"turn": self.turn, "listed": listed}

    def actions(self, t, ora, seed=11):
        acts = ora.agent_actions(seed) if t is not None else np.zeros((self.B, self.maxp), O.ACTION_DTYPE)
        for e, c in enumerate(self.cases):
            acts[e] = c.actions(t, self.maxp) if t is not None else 0
        return acts

    def check_facts(self, t, st, err, bits):
        fails = []
        for e, c in enumerate(self.cases):
            v = View(c, e, st, err, bits, t)
            if t > 0 and v.turn < v.turn_forced + t:
                continue      # the game ended on an earlier turn: a frozen or a re-dealt env
            if t <= 0:
                v.eq("turn", v.turn, v.turn_forced + t)
            c.sc.facts(t, v)
            fails += [v.ctx(f) for f in v.fails]
        assert not fails, f"{len(fails)} derived fact(s) fail on <{self.key}>:\n  " + "\n  ".join(fails[:20])


def play(batch, eng=None, after_launch=None):
    """reset, pokes, warm-up, the forced turn and the turns after it, on the oracle and - if given - the engine in lock-step:
    after every turn the derived facts, and on the engine the error codes, the packed masks and the full state against the
    oracle's.  Returns which envs entered the forced turn on the ordinary path: (by the flag model, by the device's flags)."""
    b = batch
    ora = O.OracleBatch(b.B, b.mw, b.mh, b.maxp, fog=True)
    both = (ora,) if eng is None else (ora, eng)
    for x in both:
        x.reset(b.army, b.owner, b.typ, b.w, b.h, b.p)
    if eng is not None and after_launch is not None:
        after_launch(eng, eng.game_state(), f"hazards <{b.key}> reset")
    poke = b.pokes(ora.read_state())
    for x in both:
        x.write_state(poke)
    if eng is not None and after_launch is not None:
        after_launch(eng, eng.game_state(), f"hazards <{b.key}> write_state")
    model = OT.FlagModel(ora.read_state())
    model.imported()
    ctx = f"hazards <{b.key}>"
    ordinary = None
    for t in [-1] + list(range(TURNS)):
        if t == 0:
            ordinary = (OT.ordinary(model.flags(), model.prev), None if eng is None else OT.ordinary(F.header_flags(eng), model.prev))
        acts = b.actions(None if t < 0 else t, ora)
        oerr, obits = ora.step(acts, want_mask=True)
        st = ora.read_state()
        if eng is not None:
            herr, hbits = eng.step(acts, want_mask=True)
            hst = eng.game_state()
            if after_launch is not None:
                after_launch(eng, hst, f"{ctx} t={t}")
            b.check_facts(t, hst, herr, hbits)
            assert np.array_equal(herr, oerr), f"{ctx} t={t}: err differs in envs {np.flatnonzero(herr != oerr)[:8]}: hip={herr[herr != oerr][:8]} ora={oerr[herr != oerr][:8]}"
            assert np.array_equal(hbits, obits), f"{ctx} t={t}: legal mask differs in envs {np.unique(np.argwhere(hbits != obits)[:, 0])[:8]}"
            H.assert_states_equal(hst, st, f"{ctx} t={t}")
        else:
            b.check_facts(t, st, oerr, obits)
        model.step(oerr, st)
    return ordinary
