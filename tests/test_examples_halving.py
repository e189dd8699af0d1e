"""examples/evaluate_arena.py --halving runs end to end on a tiny config: a sequential-halving entrant (uniform prior) beside
the flat playout searcher and a random entrant, with either rollout, and the table names it."""
import importlib.util
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
@pytest.mark.parametrize("rollout,tag", [("agent", ""), ("bot", "bot-")])
def test_evaluate_arena_with_a_halving_entrant(capsys, rollout, tag):
    out = _example("evaluate_arena").main(["--random", "--playouts", "4:2:4", "--halving", "4:8:4", "--playout-rollout", rollout,
                                           "--num-envs", "18", "--board", "8", "--players", "2", "--max-turns", "20", "--episodes", "1",
                                           "--poll-every", "4"])
    assert out["names"] == ["random-0", f"playouts-{tag}4:2:4", f"halving-{tag}4:8:4"]
    assert out["games"] == 18 and set(out["games_per_env"]) == {1} and all(math.isfinite(r) for r in out["ratings"])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].split() == ["entrant", "games", "win", "elim", "length", "return", "rating"]
    assert [ln.split()[0] for ln in lines[1:4]] == out["names"]


def test_halving_argument_is_parsed():
    ex = _example("evaluate_arena")
    assert ex.parse_halving("16:64:8") == (16, 64, 8) and ex.parse_halving("64:256:16") == (64, 256, 16)
    for bad in ("16:64", "a:b:c", "0:64:8", "16:0:8", "16:64:0", "65:64:8", "16:64:8:1"):
        with pytest.raises(SystemExit):
            ex.parse_halving(bad)
