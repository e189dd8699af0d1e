"""The tree-search restatement (tests/_tree_reference.py) pinned against a hand-made three-level tree whose select path and
backup sums are worked out here, and TreeSearch's schedule against its definition.  No GPU."""
import math

import numpy as np

import _halving_reference as HR
import _tree_reference as TR


def _hand_tree():
    """One row, three slots a node, six nodes.  Default weights: q_lo = -1, q_inv_range = 1 / 2; c_visit 50, c_scale 1.

        root 0   slots 10, 11, NONE    edges -> node 1, not expanded, not expanded    counts 2, 0, 0   sums 0.4, 0, 0
        node 1   slots 20, 21, 22      edges -> node 2, node 3, DEAD                  counts 1, 1, 0   sums 0.8, -0.4, 0
                 value 0.2, logits 0
        node 2   slots 30, 31, NONE    edges not expanded                              counts 0         value 0.8, logits 0
        node 3   terminal, value -1 (the seat lost there)
    """
    T = TR.new_tree(6, 1, 3)
    T["node_status"][[0, 1, 2], 0] = TR.IN_USE
    T["node_status"][3, 0] = TR.IN_USE | TR.TERMINAL
    T["child_action"][0, 0] = [10, 11, TR.NONE]
    T["child_node"][0, 0] = [1, TR.NOT_EXPANDED, TR.NOT_EXPANDED]
    T["child_count"][0, 0] = [2, 0, 0]
    T["child_sum"][0, 0] = [0.4, 0.0, 0.0]
    T["child_action"][1, 0] = [20, 21, 22]
    T["child_node"][1, 0] = [2, 3, TR.DEAD]
    T["child_count"][1, 0] = [1, 1, 0]
    T["child_sum"][1, 0] = [0.8, -0.4, 0.0]
    T["node_value"][1, 0], T["node_parent"][1, 0], T["node_slot"][1, 0] = 0.2, 0, 0
    T["child_action"][2, 0] = [30, 31, TR.NONE]
    T["node_value"][2, 0], T["node_parent"][2, 0], T["node_slot"][2, 0] = 0.8, 1, 0
    T["node_value"][3, 0], T["node_parent"][3, 0], T["node_slot"][3, 0] = -1.0, 1, 1
    return T


def test_select_walks_the_path_worked_out_by_hand():
    """Column 0 starts at root slot 0, which leads to node 1.  There slots 0 and 1 are open (slot 2 is dead), both visited
    once: sumN = 2, nmax = 1, q = 0.8 and -0.4, equal priors.  z = 51 * ((q + 1) / 2) = 45.9 and 15.3, so pi' is
    (1 / (1 + e^-30.6), e^-30.6 / (1 + e^-30.6)) and the scores are pi' - 1/3: slot 0 by a gap of (1 - e^-30.6) / (1 + e^-30.6).
    Node 2 has two open slots, nothing visited: v_mix is its value on both, pi' = 1/2 each, an exact tie -> slot 0, which is
    not expanded: the leaf is (2, 0), action 30, depth 2.  Column 1 starts at root slot 1, not expanded: leaf (0, 1), action 11."""
    T = _hand_tree()
    node, slot, action, depth, gaps = TR.select(T, None, 3)
    assert node[0].tolist() == [2, 0, 0] and slot[0].tolist() == [0, 1, 2]
    assert action[0].tolist() == [30, 11, TR.NONE] and depth[0].tolist() == [2, 0, 0]
    e = math.exp(-30.6)
    assert len(gaps) == 2 and abs(gaps[0] - (1 - e) / (1 + e)) < 1e-12 and gaps[1] == 0.0
    # permuted root slots, two columns
    node, slot, action, depth, _ = TR.select(T, np.array([[1, 0]]), 2)
    assert node[0].tolist() == [0, 2] and slot[0].tolist() == [1, 0] and action[0].tolist() == [11, 30]
    # one more visit of edge (1, 0) with a bad value turns node 1 towards its terminal child: q = -0.9 / 2 and -0.4,
    # counts 2 and 1 of 3: z = 52 * 0.275 = 14.3 and 52 * 0.3 = 15.6, pi' = (0.214, 0.786), scores 0.214 - 0.5 and 0.786 - 0.25
    T["child_sum"][1, 0, 0], T["child_count"][1, 0, 0] = -0.9, 2
    node, slot, action, depth, gaps = TR.select(T, np.array([[0]]), 1)
    p1 = 1.0 / (1.0 + math.exp(14.3 - 15.6))
    assert (node[0, 0], slot[0, 0], action[0, 0], depth[0, 0]) == (3, -1, TR.NONE, 2)
    assert abs(gaps[0] - ((p1 - 0.25) - ((1 - p1) - 0.5))) < 1e-12
    # a dead root edge, and a node whose slots are all closed
    T["child_node"][0, 0, 1] = TR.DEAD
    T["child_node"][2, 0] = [TR.DEAD, TR.DEAD, TR.NOT_EXPANDED]
    T["child_sum"][1, 0, 0], T["child_count"][1, 0, 0] = 0.8, 1
    node, slot, action, depth, _ = TR.select(T, None, 3)
    assert node[0].tolist() == [2, 0, 0] and slot[0].tolist() == [-1, -1, 2] and depth[0].tolist() == [2, 0, 0]
    assert action[0].tolist() == [TR.NONE] * 3


def test_backup_adds_the_sums_worked_out_by_hand():
    """Column 0 expanded edge (2, 0) into node 4: replica 0 is alive with land 30 of 40 and army 60 of 80, so its score is
    0.5 * 0.75 + 0.5 * 0.75 - 0.5 = 0.25; replica 1 is invalid.  g = 0.25 goes to edges (2, 0), (1, 0) and (0, 0): sums 0.25,
    1.05 and 0.65, counts 1, 2 and 3.  Column 1's board was not stored: edge (0, 1) dies and nothing is added.  Column 2 is a
    padding slot whose playouts are invalid: dead as well."""
    T = _hand_tree()
    terms = np.zeros((1, 3, 2, 8), np.int32)
    terms[0, 0, 0] = [1, 8, 1, 0, 30, 60, 10, 20]
    terms[0, 1, :] = [1, 8, 1, 0, 5, 5, 5, 5]
    leaf_node, leaf_slot = np.array([[2, 0, 0]], np.int32), np.array([[0, 1, 2]], np.int32)
    new_node, status = np.array([[4, 5, 5]], np.int32), np.array([[TR.STORED, 0, TR.STORED]], np.int32)
    TR.backup(T, leaf_node, leaf_slot, new_node, terms, status)
    assert T["child_node"][2, 0].tolist() == [4, TR.NOT_EXPANDED, TR.NOT_EXPANDED]
    assert T["child_node"][0, 0].tolist() == [1, TR.DEAD, TR.DEAD]
    assert (T["node_value"][4, 0], T["node_status"][4, 0], T["node_parent"][4, 0], T["node_slot"][4, 0]) == (0.25, TR.IN_USE, 2, 0)
    assert T["child_sum"][2, 0].tolist() == [0.25, 0.0, 0.0] and T["child_count"][2, 0].tolist() == [1, 0, 0]
    assert T["child_sum"][1, 0].tolist() == [0.8 + 0.25, -0.4, 0.0] and T["child_count"][1, 0].tolist() == [2, 1, 0]
    assert T["child_sum"][0, 0].tolist() == [0.4 + 0.25, 0.0, 0.0] and T["child_count"][0, 0].tolist() == [3, 0, 0]
    assert T["node_status"][5, 0] == 0
    # a terminal revisit: the walk stopped at node 3 (value -1), whose parent edge is (1, 1): -0.4 - 1 and 0.65 - 1
    TR.backup(T, np.array([[3]], np.int32), np.array([[-1]], np.int32), np.array([[5]], np.int32), terms[:, :1], status[:, :1])
    assert T["child_sum"][1, 0].tolist() == [1.05, -0.4 + -1.0, 0.0] and T["child_count"][1, 0].tolist() == [2, 2, 0]
    assert T["child_sum"][0, 0, 0] == 0.65 + -1.0 and T["child_count"][0, 0, 0] == 4
    # a walk that stopped at a node that is not terminal adds nothing; a won first turn makes the new node terminal, and
    # the net's value is mixed in as (1 - w) * g + w * value
    before = {k: v.copy() for k, v in T.items()}
    TR.backup(T, np.array([[2]], np.int32), np.array([[-1]], np.int32), np.array([[5]], np.int32), terms[:, :1], status[:, :1])
    assert all(np.array_equal(before[k], T[k]) for k in T)
    TR.backup(T, np.array([[2]], np.int32), np.array([[1]], np.int32), np.array([[5]], np.int32), terms[:, :1],
              np.array([[TR.STORED | TR.OVER]], np.int32), net_value=np.array([[0.5]], np.float32), value_weight=0.25)
    assert T["node_status"][5, 0] == TR.IN_USE | TR.TERMINAL and T["node_value"][5, 0] == 0.75 * 0.25 + 0.25 * 0.5
    assert T["child_count"][0, 0, 0] == 5


def test_the_schedule_and_node_count():
    """TreeSearch's waves and nodes follow from the halving schedule: R_r waves of K_r columns, a node per column and wave"""
    import types
    import generalsreinforcementlearning_amd as g
    e = types.SimpleNamespace(max_w=5, max_h=5, max_p=2, device=0)
    for m, sims, R in ((16, 64, 1), (64, 256, 1), (1, 1, 2), (5, 7, 3), (2, 2, 1)):
        sched = HR.schedule(m, sims)
        s = g.TreeSearch(e, candidates=m, simulations=sims, replicas=R)
        assert s.schedule == sched and s.waves == sum(r for _, r in sched)
        assert s.simulations_per_row == HR.playouts_per_row(m, sims) and s.nodes == 1 + s.simulations_per_row
        assert s.playouts_per_row == R * s.simulations_per_row
    s = g.TreeSearch(e, candidates=16, simulations=64)
    assert s.schedule == [(16, 1), (8, 2), (4, 4), (2, 8)] and s.waves == 15 and s.nodes == 65
    assert g.TreeSearch(e, candidates=64, simulations=256).nodes == 251
