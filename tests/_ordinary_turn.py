"""The per-turn step kernel's ORDINARY turn (GVEC_ORDTURN, gvec_device.hpp; PBoard::ordinary_turn, gvec_packed.hpp),
restated once in Python: the envs whose next turn the kernel plays on its straight-line instantiation.

    live, armies in narrow form, lists equal to ownership           not HF_DONE, not HF_WIDE, not HF_LDIFF
    stats in sync, V at most a tile per player, few special tiles   HF_SYNC, HF_VSMALL, HF_FEWSPECIAL
    the turn about to be played is not turn 0                       turn >= 0 before the increment
    V stays below the fog's threshold                               P <= N / 10
    not a growth turn (GVEC_ORDTURN bit 4)                          (turn + 1) % interval != 0
    no production rate that takes a narrow army past 24 bits        max rate <= 0xFFFFFF - 8 * 65,535 (KF_BIGRATE, gvec_api.hip)

`ordinary(flags, state)` takes the header flags of a device batch (tests/_state_forms.py header_flags) or the ones
`FlagModel` keeps for an oracle batch.  The first three flags and HF_FEWSPECIAL are functions of the state
(tests/_state_forms.py states them); HF_SYNC and HF_VSMALL are the turn engine's own bookkeeping and no part of the exported
state, so the model follows them from turn to turn by the rules gvec_packed.hpp gives:

    HF_VSMALL  set by every turn that is played, cleared by a turn with an elimination (tile turnover: a general was captured)
    HF_SYNC    set by every stats pass; cleared by an aborted turn without an elimination (armies moved, no pass followed); a
               turn that changed no tile runs no pass and leaves it as it was
    both       set by the initial setup of a reset; a re-dealt env takes its pool board's (set, like a reset's)
"""
import numpy as np

import _state_forms as F

HF_VSMALL = 32
NEED = F.HF_SYNC | HF_VSMALL | F.HF_FEWSPECIAL
BAR = F.HF_DONE | F.HF_WIDE | F.HF_LDIFF
NOGROW = True   # GVEC_ORDTURN bit 4 of the shipped default
BIG_RATE = 0xFFFFFF - 8 * 65535   # above it the engine plays no ordinary turn: the stats pass sums armies with 24-bit multiplies


def ordinary(flags, st, interval=25, nogrow=NOGROW, prod=(1, 1, 1)):
    """bool[n]: the envs whose NEXT per-turn launch takes the ordinary path.  flags: header flags (H_DIMS >> 24);
    st: game_state / read_state with turn, players, width, height; interval, prod: the engine's production config."""
    flags = np.asarray(flags, np.int64)
    turn = st["turn"].astype(np.int64)
    n = st["width"].astype(np.int64) * st["height"]
    o = ((flags & (NEED | BAR)) == NEED) & (turn >= 0) & (10 * st["players"].astype(np.int64) <= n)
    if nogrow:
        o &= (turn + 1) % interval != 0
    if max(prod) > BIG_RATE:
        o &= False
    return o


def state_flags(st):
    """The header flags that are functions of the exported state: HF_DONE, HF_WIDE, HF_LDIFF, HF_FEWSPECIAL."""
    typ = st["type"]
    special = ((typ == 1) | (typ == 2)).sum(axis=1)
    few = 2 * st["players"].astype(np.int64) + special <= (st["width"].astype(np.int64) * st["height"]) // 5
    return (np.where(st["done"].astype(bool), F.HF_DONE, 0) | np.where(F.wide_envs(st), F.HF_WIDE, 0)
            | np.where(F.desynced_envs(st), F.HF_LDIFF, 0) | np.where(few, F.HF_FEWSPECIAL, 0)).astype(np.int64)


class FlagModel:
    """HF_SYNC and HF_VSMALL of a batch that was reset (initial setup done) and is then stepped one turn at a time."""

    def __init__(self, st):
        self.book = np.full(len(st["turn"]), F.HF_SYNC | HF_VSMALL, np.int64)
        self.prev = st
        self.err = None   # the error codes of the last turn

    def imported(self, envs=slice(None)):
        """write_state: "nothing is known" (Board::static_flags)"""
        self.book[envs] = 0

    def flags(self):
        return state_flags(self.prev) | self.book

    def step(self, err, st, auto_reset=False):
        """err, st: what the turn returned and left"""
        was_done = self.prev["done"].astype(bool)
        played = ~was_done
        # an elimination order: a player's general was captured.  Fewer players alive shows most of them, not all: two players
        # who take each other's general in one turn are both turned over and both alive again after the stats pass
        taken = ((self.prev["type"] == 1) & (self.prev["owner"] >= 0) & (st["owner"] != self.prev["owner"])).any(axis=1)
        elim = taken | (st["alive"].astype(np.int64).sum(axis=1) < self.prev["alive"].astype(np.int64).sum(axis=1))
        aborted = np.asarray(err) != 0
        touched = st["changed"].astype(bool).any(axis=1)
        sync = (self.book & F.HF_SYNC) != 0
        sync = np.where(aborted, elim, sync | touched)
        book = np.where(sync, F.HF_SYNC, 0) | np.where(elim, 0, HF_VSMALL)
        self.book = np.where(played, book, (F.HF_SYNC | HF_VSMALL) if auto_reset else self.book)
        self.prev = st
        self.err = np.asarray(err)
