"""The tree search's two example entry points run end to end on tiny configs: examples/train_search_distill.py --search tree
(the network is the prior of the root and of the inner nodes) writes a checkpoint, and examples/evaluate_arena.py --tree
M:N:D[:C] seats a TreeSearch entrant with that checkpoint as its prior, and with the uniform prior."""
import importlib.util
import json
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.gpu
def test_distill_with_the_tree_search_and_an_arena_with_its_checkpoint(tmp_path, capsys):
    path = str(tmp_path / "tree.pt")
    out = _example("train_search_distill").main(["--num-envs", "8", "--board", "8", "--players", "2", "--horizon", "3", "--iterations", "2",
                                                 "--batch-size", "32", "--halving", "4:8:3", "--search", "tree", "--save", path])
    rows = out["iterations"]
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(rows) == 2 and printed == rows
    for r in rows:
        assert all(math.isfinite(r[k]) for k in ("ce", "kl", "value_loss", "entropy")), r
        assert r["ce"] > 0.0 and r["playouts_per_decision"] == 8                 # (4, 1), (2, 2): eight simulations a decision
    assert out["rejected"] == 0 and out["parameter_change"] > 0.0
    # the checkpoint as the prior of the root (playout_policy's net) and of the inner nodes (prior_fn), six slots a node
    res = _example("evaluate_arena").main([path, "--random", "--tree", "4:8:3:6", "--num-envs", "8", "--board", "8", "--players", "2",
                                           "--max-turns", "12", "--episodes", "1", "--poll-every", "4"])
    assert res["names"] == ["tree.pt", "random-0", "tree-4:8:3"]
    assert res["games"] == 8 and set(res["games_per_env"]) == {1} and all(math.isfinite(r) for r in res["ratings"])


@pytest.mark.gpu
@pytest.mark.parametrize("rollout,tag", [("agent", ""), ("bot", "bot-")])
def test_evaluate_arena_with_a_tree_entrant(capsys, rollout, tag):
    out = _example("evaluate_arena").main(["--random", "--halving", "4:8:3", "--tree", "4:8:3", "--playout-rollout", rollout, "--num-envs", "12",
                                           "--board", "8", "--players", "2", "--max-turns", "12", "--episodes", "1", "--poll-every", "4"])
    assert out["names"] == ["random-0", f"halving-{tag}4:8:3", f"tree-{tag}4:8:3"]
    assert out["games"] == 12 and set(out["games_per_env"]) == {1} and all(math.isfinite(r) for r in out["ratings"])
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split()[0] for ln in lines[1:4]] == out["names"]


def test_tree_argument_is_parsed():
    ex = _example("evaluate_arena")
    assert ex.parse_tree("16:64:8") == (16, 64, 8, None) and ex.parse_tree("16:64:8:32") == (16, 64, 8, 32)
    for bad in ("16:64", "a:b:c", "0:64:8", "16:0:8", "16:64:0", "65:64:8", "16:64:8:8", "16:64:8:65", "16:64:8:32:1"):
        with pytest.raises(SystemExit):
            ex.parse_tree(bad)
