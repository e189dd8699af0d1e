"""The tree search's argument handling, which needs no device: the three entry points refuse what they cannot run with -1 and
a message naming the field before anything touches a GPU, n == 0 is a no-op, and TreeSearch raises ValueError before any
library call."""
import re
import types

import pytest

from _api_calls import passes_checks, rejected


@pytest.fixture(scope="module")
def L():
    from generalsreinforcementlearning_amd.csrc import build as B
    B.build(verbose=False)
    import generalsreinforcementlearning_amd as g
    return g.load()


P = 16                                                           # a non-NULL address nothing dereferences


class _Rows:
    rows = property(lambda self: self.tree.n)    # what _api_calls.passes_checks asks for


def _tree(lib, **kw):
    a = dict(n=4, nodes=9, num_slots=8, reserved=0, **{k: P for k in ("child_action", "child_logit", "child_node", "child_count", "child_sum",
                                                                        "node_value", "node_status", "node_parent", "node_slot")})
    a.update(kw)
    return lib.Tree(**a)


def _select(lib, tree=None, **kw):
    class Args(_Rows, lib.TreeSelectArgs):
        pass
    a = dict(tree=tree or _tree(lib), k=8, reserved=0, slot=None, q_lo=-1.0, q_inv_range=0.5, c_visit=50.0, c_scale=1.0, leaf_node=P,
             leaf_slot=P, leaf_action=P, leaf_depth=P)
    a.update(kw)
    return Args(**a)


def _backup(lib, tree=None, **kw):
    class Args(_Rows, lib.TreeBackupArgs):
        pass
    a = dict(tree=tree or _tree(lib), k=8, replicas=2, leaf_node=P, leaf_slot=P, new_node=P, terms=P, status=P, net_value=None,
             value_weight=0.0, win=1.0, loss=-1.0, land=0.5, army=0.5)
    a.update(kw)
    return Args(**a)


def test_select_and_backup_check_their_arguments_without_a_gpu(L):
    from generalsreinforcementlearning_amd import _lib as lib
    for fn, make in (("gvec_tree_select", _select), ("gvec_tree_backup", _backup)):
        rejected(L, fn, None, "is NULL")
        for tree_kw, text in ((dict(n=-1), "n -1"), (dict(num_slots=0), "num_slots 0"), (dict(num_slots=65), "num_slots 65"),
                              (dict(nodes=0), "nodes 0"), (dict(n=2 ** 20, nodes=2 ** 11), "2^31"), (dict(reserved=1), "reserved"),
                              (dict(child_sum=None), "child_sum"), (dict(node_slot=None), "node_slot")):
            rejected(L, fn, make(lib, _tree(lib, **tree_kw)), text)
        rejected(L, fn, make(lib, k=0), "k 0")
        rejected(L, fn, make(lib, k=9), "k 9")
        passes_checks(L, fn, make(lib, _tree(lib, n=0)))                  # nothing to do: no device needed
        passes_checks(L, fn, make(lib))                                   # with a device present: not called
        passes_checks(L, fn, make(lib, _tree(lib, num_slots=64, nodes=251), k=64))
    rejected(L, "gvec_tree_select", _select(lib, k=4), "slot is NULL")    # the identity needs k == num_slots
    rejected(L, "gvec_tree_select", _select(lib, reserved=3), "reserved")
    passes_checks(L, "gvec_tree_select", _select(lib, k=4, slot=P))
    for field in ("leaf_node", "leaf_slot", "leaf_action", "leaf_depth"):
        rejected(L, "gvec_tree_select", _select(lib, **{field: None}), "is NULL")
    rejected(L, "gvec_tree_backup", _backup(lib, replicas=0), "replicas 0")
    passes_checks(L, "gvec_tree_backup", _backup(lib, net_value=P, value_weight=0.5))
    for field in ("leaf_node", "leaf_slot", "new_node", "terms", "status"):
        rejected(L, "gvec_tree_backup", _backup(lib, **{field: None}), "is NULL")


def test_expand_checks_its_arguments_without_a_gpu(L):
    """through the Python front on a stand-in engine whose handle is NULL: every check of a field comes before the handle's, so
    each refusal names its field, and a call that passes them all ends at the handle - nothing can be launched"""
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.search import search_expand_device
    eng = types.SimpleNamespace(L=L, h=None)

    def refused(text, bot=0, permille=0, **kw):
        a = dict(num_roots=1, candidates_ptr=P, root_players_ptr=P, terms_ptr=P, num_candidates=5, replicas=2, depth=3)
        a.update(kw)
        with pytest.raises(g.GvecError, match=re.escape(text)) as ei:
            search_expand_device(eng, bot_players=bot, bot_random_permille=permille, **a)
        assert ei.value.code == -1 and "gvec_search_expand" in str(ei.value)

    for kw, text in ((dict(root_players_ptr=None), "root_players"), (dict(candidates_ptr=None), "candidates"), (dict(terms_ptr=None), "terms"),
                     (dict(num_roots=-2), "num_roots"), (dict(num_candidates=0), "num_candidates"), (dict(replicas=-1), "replicas"),
                     (dict(depth=0), "depth"), (dict(num_roots=2 ** 30, num_candidates=4), "2^31")):
        refused(text, **kw)
    refused("bot_random_permille", permille=1001)
    refused("bot_players", bot=1 << 8)
    refused("h is NULL")                                                  # every field passed: the handle comes last
    refused("h is NULL", num_roots=0)                                     # ... and even a no-op needs one
    with pytest.raises(ValueError):
        search_expand_device(eng, 1, P, P, P, 5, 2, 3, bot_players=-1)


def _fake_engine():
    return types.SimpleNamespace(max_w=5, max_h=5, max_p=2, device=0)


def test_tree_search_raises_value_errors_before_any_library_call():
    import generalsreinforcementlearning_amd as g
    e = _fake_engine()
    s = g.TreeSearch(e, candidates=16, simulations=64, depth=8)
    assert s.schedule == [(16, 1), (8, 2), (4, 4), (2, 8)] and s.waves == 15 and s.nodes == 65 and s.C == 16
    assert g.TreeSearch(e, candidates=4, simulations=8, children=9).C == 9
    for kw in (dict(candidates=0), dict(candidates=65), dict(simulations=0), dict(simulations=True), dict(depth=0), dict(replicas=0),
               dict(replicas=1.5), dict(children=3, candidates=4), dict(children=65), dict(children="8"), dict(value_weight=-0.1),
               dict(value_weight=1.5), dict(value_weight=0.5), dict(prior_fn=3), dict(rollout="mcts"), dict(bot_players=[0]),
               dict(rollout="bot", bot_players=[2]), dict(rollout="bot", bot_random_permille=1001), dict(c_visit=-1.0),
               dict(c_scale=float("nan")), dict(score="high")):
        with pytest.raises(ValueError):
            g.TreeSearch(e, **kw)
    assert g.TreeSearch(e, value_weight=0.5, prior_fn=lambda obs, mask: None).value_weight == 0.5
    bot = g.TreeSearch(e, rollout="bot", bot_players=[1], bot_random_permille=100)
    assert (bot.bot_players, bot.bot_random_permille) == (0b10, 100)
    assert g.TreeSearch.round_seed(7, 3) == g.HalvingSearch.round_seed(7, 3)
