"""TEST INFRASTRUCTURE - the two walks of the tree search restated in plain Python (include/generals_vec.h "tree search below
the root"): select with loops over the open slots in float64, reporting per decision the gap between
the best score and the best differing one, and backup with the replicas added in order.  Nothing here imports the package:
tests/test_tree_reference.py pins it against a hand-made tree, the GPU tests hold the kernels to it."""
import math

import numpy as np

import _halving_reference as HR

NONE = HR.NONE
NOT_EXPANDED, DEAD = -1, -2
IN_USE, TERMINAL = 1, 2
STORED, OVER, SEAT_DEAD = 1, 2, 4


def new_tree(nodes, n, C):
    """the nine node-major arrays of an empty tree: every slot NONE and not expanded, no node in use"""
    return dict(child_action=np.full((nodes, n, C), NONE, np.int64), child_logit=np.zeros((nodes, n, C), np.float32),
                child_node=np.full((nodes, n, C), NOT_EXPANDED, np.int32), child_count=np.zeros((nodes, n, C), np.int32),
                child_sum=np.zeros((nodes, n, C), np.float64), node_value=np.zeros((nodes, n), np.float64),
                node_status=np.zeros((nodes, n), np.int32), node_parent=np.zeros((nodes, n), np.int32),
                node_slot=np.zeros((nodes, n), np.int32))


TREE_FIELDS = tuple(new_tree(1, 1, 1))


def pick(T, u, r, q_lo, q_inv, c_visit, c_scale):
    """the rule at node u of row r -> (slot or -1 when no slot is open, gap): gap = the best score minus the second best
    (inf for a single open slot); 0 is an exact tie, which goes to the lower slot"""
    C = T["child_action"].shape[2]
    opened = [c for c in range(C) if T["child_action"][u, r, c] != NONE and T["child_node"][u, r, c] != DEAD]
    if not opened:
        return -1, math.inf
    N = {c: int(T["child_count"][u, r, c]) for c in opened}
    logit = {c: float(T["child_logit"][u, r, c]) for c in opened}
    total, nmax = sum(N.values()), max(N.values())
    top = max(logit.values())
    w = {c: math.exp(logit[c] - top) for c in opened}
    q = {c: float(T["child_sum"][u, r, c]) / float(N[c]) for c in opened if N[c] > 0}
    v_mix = float(T["node_value"][u, r])
    if total != 0:
        num = den = 0.0
        for c in opened:
            if N[c] > 0:
                num += w[c] * q[c]
                den += w[c]
        v_mix = (v_mix + float(total) * (num / den)) / (1.0 + float(total))
    z = {c: logit[c] + ((c_visit + float(nmax)) * c_scale) * (((q[c] if N[c] > 0 else v_mix) - q_lo) * q_inv) for c in opened}
    ztop = max(z.values())
    e = {c: math.exp(z[c] - ztop) for c in opened}
    esum = 0.0
    for c in opened:
        esum += e[c]
    score = {c: e[c] / esum - float(N[c]) / (1.0 + float(total)) for c in opened}
    best = max(score.values())
    slot = min(c for c in opened if score[c] == best)
    rest = [score[c] for c in opened if c != slot]
    return slot, (best - max(rest) if rest else math.inf)


def select(T, slot, k, weights=None, c_visit=50.0, c_scale=1.0):
    """slot int [n, k] or None (the identity) -> (leaf_node, leaf_slot int32 [n, k], leaf_action int64 [n, k], leaf_depth
    int32 [n, k], gaps: the gap of every decision made)"""
    q_lo, q_inv = HR.q_range(**dict(HR.DEFAULT_WEIGHTS, **(weights or {})))
    nodes, n, C = T["child_action"].shape
    assert slot is not None or k == C
    leaf_node, leaf_slot = np.zeros((n, k), np.int32), np.zeros((n, k), np.int32)
    leaf_action, leaf_depth = np.full((n, k), NONE, np.int64), np.zeros((n, k), np.int32)
    gaps = []
    for r in range(n):
        for c in range(k):
            s = c if slot is None else int(slot[r, c])
            u, depth, action = 0, 0, NONE
            if not 0 <= s < C:
                s = -1
            else:
                for _ in range(nodes):
                    child = int(T["child_node"][u, r, s])
                    if child == NOT_EXPANDED:
                        action = int(T["child_action"][u, r, s])
                        break
                    if not 0 <= child < nodes:
                        s = -1
                        break
                    u, depth, s = child, depth + 1, -1
                    if T["node_status"][u, r] & TERMINAL:
                        break
                    s, gap = pick(T, u, r, q_lo, q_inv, c_visit, c_scale)
                    if s < 0:
                        break
                    gaps.append(gap)
                else:
                    if s >= 0 and T["child_node"][u, r, s] != NOT_EXPANDED:
                        s = -1
            leaf_node[r, c], leaf_slot[r, c], leaf_depth[r, c] = u, s, depth
            leaf_action[r, c] = action if s >= 0 else NONE
    return leaf_node, leaf_slot, leaf_action, leaf_depth, gaps


def backup(T, leaf_node, leaf_slot, new_node, terms, status, net_value=None, value_weight=0.0, weights=None):
    """updates T in place; terms int32 [n, k, R, 8], status int32 [n, k], net_value float32 [n, k] or None"""
    w = dict(HR.DEFAULT_WEIGHTS, **(weights or {}))
    nodes, n, C = T["child_action"].shape
    terms = np.asarray(terms)
    k, R = terms.shape[1], terms.shape[2]
    scores = HR.playout_scores(terms, **w)
    for r in range(n):
        for c in range(k):
            u, s = int(leaf_node[r, c]), int(leaf_slot[r, c])
            if not 0 <= u < nodes or s >= C:
                continue
            if s >= 0:
                total, cnt = 0.0, 0
                for j in range(R):
                    if terms[r, c, j, 0] != 0:
                        total = total + float(scores[r, c, j])
                        cnt += 1
                st = int(status[r, c])
                if not st & STORED or cnt == 0:
                    T["child_node"][u, r, s] = DEAD
                    continue
                v = int(new_node[r, c])
                if not 1 <= v < nodes:
                    continue
                g = total / float(cnt)
                if net_value is not None:
                    g = (1.0 - float(value_weight)) * g + float(value_weight) * float(np.float32(net_value[r, c]))
                T["child_node"][u, r, s] = v
                T["node_value"][v, r] = g
                T["node_status"][v, r] = IN_USE | (TERMINAL if st & (OVER | SEAT_DEAD) else 0)
                T["node_parent"][v, r], T["node_slot"][v, r] = u, s
            else:
                if u == 0 or not T["node_status"][u, r] & TERMINAL:
                    continue
                g = float(T["node_value"][u, r])
                u, s = int(T["node_parent"][u, r]), int(T["node_slot"][u, r])
            for _ in range(nodes):
                if not (0 <= u < nodes and 0 <= s < C):
                    break
                T["child_sum"][u, r, s] = float(T["child_sum"][u, r, s]) + g
                T["child_count"][u, r, s] += 1
                if u == 0:
                    break
                u, s = int(T["node_parent"][u, r]), int(T["node_slot"][u, r])
