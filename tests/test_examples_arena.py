"""The arena examples run end to end (smoke tests on tiny configs): evaluate_arena.py with two random entrants prints a table,
and train_ppo_selfplay.py --arena-every rates the learner against its own snapshots and writes a checkpoint the evaluator loads."""
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
def test_evaluate_arena_example_runs(capsys):
    out = _example("evaluate_arena").main(["--random", "--random", "--num-envs", "32", "--board", "8", "--players", "2", "--max-turns", "20",
                                           "--episodes", "2", "--poll-every", "8"])
    assert out["names"] == ["random-0", "random-1"] and out["games"] == 64 and set(out["games_per_env"]) == {2}
    assert all(math.isfinite(r) for r in out["ratings"]) and out["ratings"][0] == 1500.0
    assert out["score"][0][1] + out["score"][1][0] == 64 == out["pair_games"][0][1]
    text = capsys.readouterr().out
    lines = text.splitlines()
    assert lines[0].split() == ["entrant", "games", "win", "elim", "length", "return", "rating"]
    assert lines[1].split()[:2] == ["random-0", "64"] and lines[2].split()[:2] == ["random-1", "64"]


@pytest.mark.gpu
def test_ppo_example_rates_itself_and_saves(tmp_path):
    path = str(tmp_path / "net.pt")
    out = _example("train_ppo_selfplay").main(["--num-envs", "32", "--board", "8", "--players", "2", "--horizon", "8", "--iterations", "3",
                                               "--batch-size", "256", "--max-turns", "10", "--arena-every", "1", "--arena-episodes", "1",
                                               "--arena-envs", "16", "--save", path])
    rows = out["iterations"]
    assert rows[0]["arena"] is None                                     # no snapshot to play yet
    for k in (1, 2):
        e = rows[k]["arena"]
        assert e["snapshot_iterations"] == list(range(k)) and e["snapshot_ratings"][0] == 1500.0
        assert math.isfinite(e["rating"]) and e["games"] == 16
    res = _example("evaluate_arena").main([path, "--random", "--num-envs", "16", "--board", "8", "--max-turns", "10", "--episodes", "1",
                                           "--poll-every", "4"])
    assert res["names"] == ["net.pt", "random-0"] and res["games"] == 16 and all(math.isfinite(r) for r in res["ratings"])
