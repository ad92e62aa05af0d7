"""CPU tests of the arena's turn record (Q21, "the replay as it was meant"): versus.play(record_turns=True) on the oracle's rules,
replay_states as the audit of a recorded game, the Game JSON round trip through print_game, and the layouts of diee_arena_ex's structs."""
import copy
import ctypes as C
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import diee_amd

versus = importlib.import_module("die-e_amd.versus")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = versus.Player
RANDOM = versus.Agent.RANDOM
_played = {}


@pytest.fixture
def played(oracle):
    """8 Random-vs-Random games on the oracle's rules with their turns: played once, shared, left unchanged"""
    if not _played:
        from oracle.arena_backend import OracleRules
        rules = OracleRules()
        _played["rules"] = rules
        _played["res"] = versus.play(P(RANDOM), P(RANDOM), diee_amd.MctsConfig.default(4), 1.25, seed=5, num_games=8, round_limit=400,
                                     rules=rules, record_turns=True)
    return _played["res"], _played["rules"]


def test_recorded_turns_replay_to_the_final_states(played):
    """every game's replay ends on final_states[g], all 32 bytes; turn 0's roll is the initial state's; the rolls chain: turn t + 1's
    roll is turn t's next_roll -- except behind the first half of a double, where apply_move (backgammon_logic.rs:176-186) draws no
    dice: the side moves again on the same roll with is_second_play set, and the dice recorded as next_roll are not used.  (The
    issue states the chain without that exception; with it the check covers every turn and asks no less.)"""
    res, rules = played
    assert len(res.games) == 8 and len(res.turns) == 8 and all(len(t) > 0 for t in res.turns)
    by_id = {g.initial_state["id"]: g for g in res.games}
    doubles = skipped = 0
    for g in range(8):
        game = by_id[g]
        assert game.turns is res.turns[g]
        states = versus.replay_states(game, rules)
        assert len(states) == len(game.turns)
        assert states[-1].tobytes() == res.final_states[g].tobytes()
        turns = game.turns
        assert turns[0]["roll"] == game.initial_state["roll"]
        for t in range(len(turns) - 1):
            a, b = turns[t], turns[t + 1]
            if a["action"] and a["roll"][0] == a["roll"][1] and not a["is_second_play"]:
                assert b["roll"] == a["roll"] and b["is_second_play"] and b["player"] == a["player"]
                doubles += 1
            else:
                assert b["roll"] == a["next_roll"] and not b["is_second_play"]
        for t in turns:
            assert set(t) == {"roll", "action", "player", "next_roll", "is_second_play"} and t["player"] == RANDOM
            assert len(t["action"]) <= 2 and all(len(m) == 2 for m in t["action"])
            skipped += not t["action"]
    assert doubles > 0 and skipped > 0                                  # both special turns occur in these games
    # the batched form says the same
    allst = versus.replay_all(res.games, rules)
    assert all(s[-1].tobytes() == res.final_states[g.initial_state["id"]].tobytes() for s, g in zip(allst, res.games))


def test_without_record_turns_nothing_changes(played):
    rec, rules = played
    res = versus.play(P(RANDOM), P(RANDOM), diee_amd.MctsConfig.default(4), 1.25, seed=5, num_games=8, round_limit=400, rules=rules)
    assert res.turns is None and all(g.turns == [] for g in res.games)
    assert res.final_states.tobytes() == rec.final_states.tobytes()
    assert [(g.initial_state["id"], g.winner) for g in res.games] == [(g.initial_state["id"], g.winner) for g in rec.games]


def test_save_load_print_round_trip_shows_a_board_per_turn(played, tmp_path):
    res, rules = played
    game = res.games[0]
    path = versus.save_game(game, str(tmp_path))
    doc = versus.load_game(path)
    assert doc["turns"] == game.turns and set(doc) == {"id", "player1", "player2", "turns", "winner", "initial_state"}
    lines = []
    versus.print_game(path, out=lines.append)
    at = [i for i, l in enumerate(lines) if l == "State after action has been played:"]
    boards = [lines[i + 1] for i in at]
    assert len(boards) == len(game.turns) and len(set(boards)) == len(game.turns)          # (the reference prints the initial board every time)
    # print_game's host-side apply agrees with the rules: its last board is the final state's
    g = game.initial_state["id"]
    final = versus.Game(RANDOM, RANDOM, res.final_states[g], g).initial_state
    assert boards[-1] == versus.to_pretty_str(final)
    # a file without next_roll (the reference's own Turn) prints as before: the initial board once per turn
    old = copy.deepcopy(doc)
    old["turns"] = [{k: t[k] for k in ("roll", "action", "player")} for t in old["turns"][:3]]
    p2 = tmp_path / "old.json"
    p2.write_text(json.dumps(old))
    lines = []
    versus.print_game(str(p2), out=lines.append)
    assert lines.count(versus.to_pretty_str(old["initial_state"])) == 1 + 3


def test_a_tampered_game_is_caught_at_the_turn(played):
    res, rules = played
    doc = res.games[1].to_json()
    n = len(doc["turns"])
    k = next(t for t in range(n // 2, n) if doc["turns"][t]["action"])
    # an illegal action: a checker moved from a point to itself
    bad = copy.deepcopy(doc)
    bad["turns"][k]["action"] = [[5, 5]]
    with pytest.raises(ValueError, match=rf"game {doc['initial_state']['id']} .*turn {k}: .*not a valid move"):
        versus.replay_states(bad, rules)
    # one roll altered
    bad = copy.deepcopy(doc)
    r = bad["turns"][k]["roll"]
    bad["turns"][k]["roll"] = [r[0] % 6 + 1, r[1]]
    with pytest.raises(ValueError, match=rf"turn {k}: recorded roll"):
        versus.replay_states(bad, rules)
    # the dice a turn was given altered: the NEXT turn's roll no longer fits the state (unless the turn is the first half of a double)
    j = next(t for t in range(n - 1) if not (doc["turns"][t]["action"] and doc["turns"][t]["roll"][0] == doc["turns"][t]["roll"][1]
                                             and not doc["turns"][t]["is_second_play"]))
    bad = copy.deepcopy(doc)
    d = bad["turns"][j]["next_roll"]
    bad["turns"][j]["next_roll"] = [d[0] % 6 + 1, d[1]]
    with pytest.raises(ValueError, match=rf"turn {j + 1}: recorded roll"):
        versus.replay_states(bad, rules)
    # a skipped turn where the Random agent had a legal play
    bad = copy.deepcopy(doc)
    bad["turns"][k]["action"] = []
    with pytest.raises(ValueError, match=rf"turn {k}: a skipped turn"):
        versus.replay_states(bad, rules)
    # the reference's own record (no next_roll) has nothing to replay
    bad = copy.deepcopy(doc)
    del bad["turns"][0]["next_roll"]
    with pytest.raises(ValueError, match="turn 0: .*next_roll"):
        versus.replay_states(bad, rules)
    versus.replay_states(doc, rules)                                    # (the untouched game passes)


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    """tests/abi_check_arena_log.c: _Static_assert(sizeof(diee_turn) == 12) and the offsets of diee_turn, diee_arena_log, diee_arena_opts"""
    exe = str(tmp_path / "abi_check_arena_log")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_check_arena_log.c"), "-o", exe])
    doc = json.loads(subprocess.check_output([exe]).decode())
    mirrors = {"diee_turn": diee_amd.Turn, "diee_arena_log": diee_amd.ArenaLog, "diee_arena_opts": diee_amd.ArenaOpts}
    seen = 0
    for key, off in doc.items():
        st, field = key.split(".")
        if st == "sizeof":
            assert C.sizeof(mirrors[field]) == off, key
            continue
        assert getattr(mirrors[st], field).offset == off, key
        seen += 1
    assert seen == 7 + 4 + 3
    assert diee_amd.TURN.itemsize == 12 and [diee_amd.TURN.fields[n][1] for n, _ in diee_amd.Turn._fields_] == [0, 4, 6, 8, 9, 10, 11]
    L = diee_amd.load_library()
    assert hasattr(L, "diee_arena_ex") and hasattr(L, "diee_free_arena_log")
    log = diee_amd.ArenaLog()
    L.diee_free_arena_log(C.byref(log)); L.diee_free_arena_log(None)    # a log no call filled: harmless
    opts = diee_amd.ArenaOpts(C.sizeof(diee_amd.ArenaOpts), (C.c_uint32 * 2)(0, 0), None)
    assert L.diee_arena_ex(None, 0, None, 0, 1, None, 1.0, 0, 1, 0, C.byref(opts), None, None, None, None, None, None, None) == diee_amd.ERR_ARG


def test_record_turns_switch_is_logged_once(monkeypatch):
    msgs = []
    monkeypatch.delenv("DIEE_RECORD_TURNS", raising=False)
    assert versus.record_turns_from_env(msgs.append) is False and not msgs
    monkeypatch.setenv("DIEE_RECORD_TURNS", "1")
    assert versus.record_turns_from_env(msgs.append) is True and len(msgs) == 1 and "Q21" in msgs[0]
