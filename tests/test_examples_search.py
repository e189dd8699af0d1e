"""examples/evaluate_arena.py --playouts runs end to end on a tiny config: a playout-search entrant (uniform prior) against a
random one, and the table names it."""
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
def test_evaluate_arena_with_a_playout_entrant(capsys):
    out = _example("evaluate_arena").main(["--random", "--playouts", "4:2:4", "--num-envs", "16", "--board", "8", "--players", "2",
                                           "--max-turns", "20", "--episodes", "1", "--poll-every", "4"])
    assert out["names"] == ["random-0", "playouts-4:2:4"] and out["games"] == 16 and set(out["games_per_env"]) == {1}
    assert all(math.isfinite(r) for r in out["ratings"])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].split() == ["entrant", "games", "win", "elim", "length", "return", "rating"]
    assert lines[1].split()[:2] == ["random-0", "16"] and lines[2].split()[:2] == ["playouts-4:2:4", "16"]


def test_playouts_argument_is_parsed():
    ex = _example("evaluate_arena")
    assert ex.parse_playouts("8:4:16") == (8, 4, 16)
    for bad in ("8:4", "a:b:c", "0:1:1", "4:2:4:1"):
        with pytest.raises(SystemExit):
            ex.parse_playouts(bad)
