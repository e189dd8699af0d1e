"""TEST INFRASTRUCTURE - what gvec_search_playouts_bot must return, computed on the CPU oracle.

The plan of tests/_search_reference.py (which root, seat and move every playout starts with, which rows are invalid) and its
one OracleBatch of V = n * K * R envs, played turn by turn instead of by rollout(): every turn is the oracle agent's moves of
(seed, env v), the scripted opponent's moves (tests/_bot_reference.py: a numpy restatement of the rule, reading the state
dict alone) written over them for the seats of bot_players, on turn 0 the seat's slot replaced by the candidate, one step.
The agent's draws and the exploration mix are both keyed by (seed, env index, the env's own turn counter, player), so env v of
the batch draws what playout v must.  A finished env plays no further turn (the oracle's step refuses it and changes
nothing), as a finished playout plays none."""
import numpy as np

import _oracle as O
from _bot_reference import bot_actions
from _search_reference import IMPORTED, Plan, coverage_roots, repeat_state   # noqa: F401  (coverage_roots: for the tests)


def reference_terms_bot(roots, root_envs, players, candidates, replicas, depth, seed, max_w, max_h, max_p, bot_players, permille=0,
                        fog=True, mix=(6554, 19661), prod=(1, 1, 1), interval=25):
    """roots: the full read_state / game_state dict of the engine's envs.  root_envs [n] (None: 0..n-1), players [n],
    candidates [n][K], bot_players: a bit mask of seats -> terms int32 [n, K, R, 8]."""
    plan = Plan(roots, root_envs, players, candidates, replicas, max_w, max_h, max_p, fog)
    st0 = repeat_state(roots, plan.src)
    ora = O.OracleBatch(plan.V, max_w, max_h, max_p, fog=fog, prod=prod, interval=interval)
    ora.set_agent_mix(*mix)
    ora.reset(st0["army"], st0["owner"], st0["type"], st0["width"], st0["height"], st0["players"])
    ora.write_state({k: st0[k] for k in IMPORTED})
    back = ora.read_state()
    for k, want in st0.items():
        assert np.array_equal(back[k], want), f"the oracle did not take the root state: field {k}"
    for t in range(int(depth)):
        cur = ora.read_state()
        acts = ora.agent_actions(seed)
        acts = bot_actions(cur, bot_players, fog, seed, permille, agent=acts.copy(), out=acts, max_p=max_p)
        if t == 0:
            acts = plan.override(acts)
        ora.step(acts)
    return plan.terms(st0["turn"], ora.read_state())
