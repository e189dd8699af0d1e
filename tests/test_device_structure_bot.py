"""The scripted opponent's rule has one definition, gvec_bot.hpp, and the playout search calls it (no GPU, no build: regular
expressions over csrc, in the manner of tests/test_device_structure.py).

Two kernels play the rule - bot_kernel for gvec_bot_actions and search_bot_kernel inside its playouts - and the search's
identity with the composition of existing calls holds only while they play the same one."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "generalsreinforcementlearning_amd", "csrc")


def _sources():
    """{file name: text without // comments} of every csrc/*.hip and *.hpp"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        with open(path) as f:
            out[os.path.basename(path)] = re.sub(r"//[^\n]*", "", f.read())
    return out


def _sites(pattern):
    return [(name, m.group(0)) for name, text in _sources().items() for m in re.finditer(pattern, text)]


def test_the_rule_has_one_definition():
    # the selection key's tile order and the exploration draw's first constant
    assert [n for n, _ in _sites(r"1023u\s*-")] == ["gvec_bot.hpp"] * 2          # the key is built once and taken apart once
    assert [n for n, _ in _sites(r"0x5851F42Du")] == ["gvec_bot.hpp"]
    # ... and the functions that make it up
    for name in ("bot_mix_draw", "bot_random_seats", "wave_max_u64", "row_any", "rows_to_bits", "from_dir", "bot_sample"):
        defs = _sites(r"__device__\s+__forceinline__\s+[\w:<>, ]+?\s+" + name + r"\s*\(")
        assert [n for n, _ in defs] == ["gvec_bot.hpp"], (name, defs)


def test_both_kernels_call_it():
    src = _sources()
    for unit, kernel in (("gvec_kernels.hip", "bot_kernel"), ("gvec_search.hip", "search_bot_kernel")):
        text = src[unit]
        assert '#include "gvec_bot.hpp"' in text
        body = text[text.index("void " + kernel + "("):]
        body = body[:body.index("\n}\n")]
        assert len(re.findall(r"\bbot_sample<MAXP, NSLOT>\(", body)) == 1, unit
        assert len(re.findall(r"\bbot_random_seats<MAXP>\(", body)) == 1, unit
        assert body.index("agent_sample<") < body.index("bot_sample<"), unit    # the agent's draw first: bot_sample overwrites m
    kernels = src["gvec_kernels.hip"]
    assert "army_to_lds" not in kernels[kernels.index("void bot_kernel("):kernels.index("counter_sum_kernel")]


def test_the_search_unit_has_no_rule_of_its_own():
    text = _sources()["gvec_search.hip"]
    assert "bot_sample(" in re.sub(r"<[^<>]*>", "", text)                        # bot_sample<MAXP, NSLOT>( is a call of bot_sample(
    assert "ds_bpermute" not in text and "bperm(" not in text                    # no cross-lane idiom of its own
    for own_bfs in (r"\bfront\s*\[", r"\breached\s*\[", r"\bneed_bfs\b", r"\bwave_max_u64\b", r"\bfrom_dir\b"):
        assert not re.search(own_bfs, text), own_bfs
    assert len(re.findall(r"\bwhile\s*\(", text)) == 2                           # the two turn loops, no BFS loop beside them
    # the existing kernel is a kernel of its own, with its old signature
    assert re.search(r"void search_kernel\(StepArgs A, SearchArgs S\)", text)
    assert re.search(r"void search_bot_kernel\(StepArgs A, SearchArgs S, BotArgs G\)", text)
