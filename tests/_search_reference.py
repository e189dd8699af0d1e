"""TEST INFRASTRUCTURE - what gvec_search_playouts must return, computed on the CPU oracle.

Playout v = (i * K + k) * R + j is env v of ONE OracleBatch of V = n * K * R envs that all start from their root's state:
turn 0 plays the oracle agent's moves of (seed, env v) with the seat's slot replaced by the candidate, then
rollout(depth - 1, seed).  Agent draws are keyed by (seed, env index, turn, player), so env v of the big batch draws what
playout v must: the kernel has to equal behaviour the engine tests already pin, bit for bit.  The candidate is decoded by
a numpy restatement of gym_decode (gvec_turn.hpp), and the rows the definition calls invalid are decided here in numpy."""
import numpy as np

import _oracle as O

PASS, NONE = -1, -2                      # GVEC_SEARCH_PASS, GVEC_SEARCH_NONE
TERMS = ("valid", "turns", "alive", "won", "land", "army", "land_others", "army_others")
ACT_VALID, ACT_HALF, ACT_SKIP_ENV = 1, 2, 4
_DIRS = ((0, -1), (1, 0), (0, 1), (-1, 0))   # up, right, down, left
IMPORTED = ("army", "owner", "type", "visible", "listed", "changed", "vis_changed", "turn", "done", "width", "height", "players", "alive",
            "army_count", "general_idx")


def decode_candidate(st, e, player, a, stride, fog):
    """gym_decode for seat `player` of env e of the state dict st: None when the action is not accepted, else
    (from_x, from_y, to_x, to_y, half).  The valid-action mask is generals_env.py's: a source is a tile the proto shows as
    the seat's (owned, and visible to it under fog) with army > 1; a direction is open when the neighbour is on the env's own
    board and no mountain; index 4, the half move, is valid when any direction is, and takes the first of up / right / down /
    left whose target is on the board, which must then be open too."""
    W, H = int(st["width"][e]), int(st["height"][e])
    if not 0 <= a < 5 * stride:
        return None
    frm, info = divmod(int(a), 5)
    if frm >= W * H:                     # a tile index beyond the env's own board has no mask bit
        return None
    fx, fy = frm % W, frm // W
    seen = (not fog) or ((int(st["visible"][e, frm]) >> player) & 1)
    if not (st["owner"][e, frm] == player and seen and st["army"][e, frm] > 1):
        return None
    on_board = [0 <= fx + dx < W and 0 <= fy + dy < H for dx, dy in _DIRS]
    open_ = [on_board[d] and st["type"][e, (fy + _DIRS[d][1]) * W + fx + _DIRS[d][0]] != 3 for d in range(4)]
    half = info == 4
    if half:
        if not any(open_):
            return None
        d = on_board.index(True)
    else:
        d = info
    if not open_[d]:
        return None
    return fx, fy, fx + _DIRS[d][0], fy + _DIRS[d][1], half


def repeat_state(st, rows):
    return {k: np.ascontiguousarray(v[rows]) for k, v in st.items()}


class Plan:
    """Which root, seat and move every playout v < V = n * K * R starts with, and which rows are invalid - all decided in
    numpy from the roots' state dict.  src [V]: the root env of playout v (env 0 stands in for an id outside the batch);
    seat [V]; valid [V]; move [V]: None (a pass, or an invalid row) or (from_x, from_y, to_x, to_y, half)."""

    def __init__(self, roots, root_envs, players, candidates, replicas, max_w, max_h, max_p, fog):
        cand = np.asarray(candidates, np.int64)
        self.n, self.K = cand.shape
        self.R = int(replicas)
        n, K, R = self.n, self.K, self.R
        N = len(roots["turn"])
        envs = np.arange(n) if root_envs is None else np.asarray(root_envs, np.int64)
        players = np.asarray(players, np.int64)
        self.V = V = n * K * R
        vi = np.arange(V) // (K * R)
        vk = (np.arange(V) // R) % K
        in_range = (envs >= 0) & (envs < N)
        self.src = np.where(in_range, envs, 0)[vi]
        self.seat = np.clip(players[vi], 0, max_p - 1)
        self.valid = np.zeros(V, bool)
        self.move = [None] * V
        for v in range(V):
            i, e, pl = vi[v], int(self.src[v]), int(players[vi[v]])
            a = int(cand[i, vk[v]])
            ok = (bool(in_range[i]) and not roots["done"][e] and 0 <= pl < max_p and pl < roots["players"][e]
                  and bool(roots["alive"][e, pl]))
            if ok and a != PASS:
                self.move[v] = decode_candidate(roots, e, pl, a, max_w * max_h, fog)
                ok = self.move[v] is not None
            self.valid[v] = ok

    def override(self, acts):
        """acts [V][max_p]: the agent's moves of turn 0 -> the same with every valid playout's seat slot replaced by its
        candidate, and GVEC_ACT_SKIP_ENV on the invalid ones (they sit turn 0 out; what follows for them is discarded)"""
        for v in range(self.V):
            pl = int(self.seat[v])
            if not self.valid[v]:
                first = acts[v, 0]
                first["flags"] |= np.uint8(ACT_SKIP_ENV)
                acts[v, 0] = first
            elif self.move[v] is None:
                acts[v, pl] = np.zeros((), O.ACTION_DTYPE)     # the pass: no move in the seat's slot
            else:
                mv = self.move[v]
                acts[v, pl] = (mv[0], mv[1], mv[2], mv[3], ACT_VALID | (ACT_HALF if mv[4] else 0), (0, 0, 0))
        return acts

    def terms(self, turn0, st):
        """turn0 [V]: the roots' turn counters; st: the state dict of the V envs after the playouts -> int32 [n, K, R, 8]"""
        t = np.zeros((self.V, 8), np.int64)
        rows, pl = np.arange(self.V), self.seat
        t[:, 0] = 1
        t[:, 1] = st["turn"].astype(np.int64) - turn0
        t[:, 2] = st["alive"][rows, pl]
        t[:, 3] = (st["done"] != 0) & (st["winner"] == pl)
        t[:, 4] = st["tile_count"][rows, pl]
        t[:, 5] = st["army_count"][rows, pl]
        t[:, 6] = st["tile_count"].astype(np.int64).sum(axis=1) - t[:, 4]
        t[:, 7] = st["army_count"].astype(np.int64).sum(axis=1) - t[:, 5]
        t[~self.valid] = 0
        return t.astype(np.int32).reshape(self.n, self.K, self.R, 8)


def reference_terms(roots, root_envs, players, candidates, replicas, depth, seed, max_w, max_h, max_p, fog=True, mix=(6554, 19661),
                    prod=(1, 1, 1), interval=25):
    """roots: the full read_state / game_state dict of the engine's envs.  root_envs [n] (None: 0..n-1; ids outside the dict
    give invalid rows), players [n], candidates [n][K] -> terms int32 [n, K, R, 8]."""
    plan = Plan(roots, root_envs, players, candidates, replicas, max_w, max_h, max_p, fog)
    st0 = repeat_state(roots, plan.src)
    ora = O.OracleBatch(plan.V, max_w, max_h, max_p, fog=fog, prod=prod, interval=interval)
    ora.set_agent_mix(*mix)
    ora.reset(st0["army"], st0["owner"], st0["type"], st0["width"], st0["height"], st0["players"])
    ora.write_state({k: st0[k] for k in IMPORTED})
    back = ora.read_state()
    for k, want in st0.items():
        assert np.array_equal(back[k], want), f"the oracle did not take the root state: field {k}"
    ora.step(plan.override(ora.agent_actions(seed)))
    if depth > 1:
        ora.rollout(int(depth) - 1, seed, 0)
    return plan.terms(st0["turn"], ora.read_state())


# ---- the coverage roots: 5x5 two-player games old enough to end inside a playout -------------------------------------------
COVER_W, COVER_H, COVER_P, COVER_B = 5, 5, 2, 32
COVER_BOARD_SEED, COVER_PLAY_SEED, COVER_SEARCH_SEED = 3, 5, 9
COVER_K, COVER_R, COVER_D = 6, 4, 8
_cover_cache = {}


def coverage_roots(fog):
    """(state dict of 2 * COVER_B roots, players [n], candidates [n, 6]): COVER_B generated 5x5 2P games after 60 random-agent
    turns at mix (0, 0), and the same games after 100.  Seats alternate.  Candidates: up to three accepted full moves of the
    seat (first, middle, last of its list), a half move from the first one's tile, an index the mask refuses, the pass;
    a seat without a move gets padding in their place.  Computed once per fog setting; callers must not change it."""
    import _harness as H
    if fog in _cover_cache:
        return _cover_cache[fog]
    ora = O.OracleBatch(COVER_B, COVER_W, COVER_H, COVER_P, fog=fog)
    ora.reset(*H.gen_boards(COVER_BOARD_SEED, [(COVER_W, COVER_H, COVER_P)] * COVER_B, COVER_W, COVER_H))
    ora.set_agent_mix(0, 0)
    ora.rollout(60, COVER_PLAY_SEED, 0)
    young = ora.read_state()
    ora.rollout(40, COVER_PLAY_SEED + 1, 0)
    old = ora.read_state()
    st = {k: np.concatenate([young[k], old[k]]) for k in young}
    n = 2 * COVER_B
    players = (np.arange(n) % COVER_P).astype(np.int32)
    stride = COVER_W * COVER_H
    cand = np.full((n, COVER_K), NONE, np.int64)
    for i in range(n):
        legal = legal_gym_actions(st, i, int(players[i]), stride, fog)
        if legal:
            cand[i, :3] = [legal[0], legal[len(legal) // 2], legal[-1]]
            cand[i, 3] = legal[0] // 5 * 5 + 4
        refused = [a for a in range(stride * 5) if decode_candidate(st, i, int(players[i]), a, stride, fog) is None]
        cand[i, 4] = refused[i % len(refused)]
        cand[i, 5] = PASS
    _cover_cache[fog] = (st, players, cand)
    return _cover_cache[fog]


def legal_gym_actions(st, e, player, stride, fog, limit=None):
    """the seat's accepted full-move gym indices of env e, ascending (at most `limit`)"""
    out = []
    W, H = int(st["width"][e]), int(st["height"][e])
    for t in range(W * H):
        if st["owner"][e, t] != player:
            continue
        for d in range(4):
            if decode_candidate(st, e, player, t * 5 + d, stride, fog) is not None:
                out.append(t * 5 + d)
                if limit is not None and len(out) == limit:
                    return out
    return out
