"""CPU tests of the device-resident arena's host side (diee_arena, die-e_amd/versus.py::play_device): the ctypes mirror of its
result struct, play()'s max_rounds, and the order of play_device's `games`."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import diee_amd

versus = importlib.import_module("die-e_amd.versus")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_result_mirror_matches_the_header(tmp_path):
    """size and field offsets of diee_arena_result as a C compiler lays out include/diee.h, against die-e_amd.ArenaResult"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed"
    fields = [n for n, _ in diee_amd.ArenaResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "diee.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(diee_arena_result));\n'
                   + "".join(f'    printf(" %zu", offsetof(diee_arena_result, {f}));\n' for f in fields)
                   + '    printf(" %d %d\\n", DIEE_AGENT_RANDOM, DIEE_AGENT_MODEL);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(diee_amd.ArenaResult)
    assert out[1:1 + len(fields)] == [getattr(diee_amd.ArenaResult, f).offset for f in fields]
    assert out[-2:] == [diee_amd.AGENT_RANDOM, diee_amd.AGENT_MODEL]


def _summary(res):
    return (res.wins_p1, res.wins_p2, res.draws, res.rounds, res.final_states.tobytes(),
            [(g.initial_state["id"], g.winner) for g in res.games])


def test_play_max_rounds_on_the_oracle_backends(oracle):
    """max_rounds = k stops play() after k rounds; max_rounds = 0 is the call without the argument"""
    from oracle.arena_backend import OracleRules, OracleSearch
    P = versus.Player
    cfg = diee_amd.MctsConfig.default(5)

    def run(**kw):
        return versus.play(P(versus.Agent.MODEL), P(versus.Agent.RANDOM), cfg, 1.25, seed=31, num_games=6, round_limit=400,
                           rules=OracleRules(), search1=OracleSearch(oracle.hash_eval_fn(), oracle.game(1)), **kw)
    full, zero = run(), run(max_rounds=0)
    assert _summary(full) == _summary(zero) and full.rounds > 7
    cut = run(max_rounds=7)
    assert cut.rounds == 7 and len(cut.games) < 6 and cut.wins_p1 + cut.wins_p2 <= len(cut.games)
    # the first 7 rounds of the full game are the same rounds: one more round of the cut call's states is the 8-round call's result
    cut8 = run(max_rounds=8)
    assert cut8.rounds == 8 and cut8.final_states.tobytes() != cut.final_states.tobytes()
    # Random vs Random with a limit below max_rounds: the loop ends by itself
    r = versus.play(P(versus.Agent.RANDOM), P(versus.Agent.RANDOM), cfg, 1.25, seed=5, num_games=6, round_limit=5, rules=OracleRules(),
                    max_rounds=9)
    assert r.rounds == 5 and r.draws == 6


def test_games_order_of_play_device_is_plays():
    """play() appends a game when it is retired: by round, player 1's list before player 2's, by game index inside a list.  The helper
    that orders play_device's games is held to a direct replay of that rule on synthetic per-game outputs."""
    rng = np.random.default_rng(3)
    n = 40
    retired_round = rng.integers(0, 6, n).astype(np.uint32)
    retired_side = rng.integers(0, 2, n).astype(np.int8)
    winner = rng.integers(-1, 2, n).astype(np.int8)
    alive = rng.random(n) < 0.2
    retired_round[alive] = 0xFFFFFFFF; retired_side[alive] = -1; winner[alive] = 0
    expect = []
    for rnd in range(6):                                   # play()'s loop: `order = concatenate([p1, p2])`, each ascending
        for side in (0, 1):
            expect += [g for g in range(n) if retired_round[g] == rnd and retired_side[g] == side]
    assert [int(g) for g in versus.retired_order(winner, retired_round, retired_side)] == expect
    assert len(expect) == int((~alive).sum())
    init = versus.new_states(n)
    init["roll"] = (3, 4)
    P = versus.Player
    games = versus.games_from_device(P(versus.Agent.MODEL), P(versus.Agent.RANDOM), init, winner, retired_round, retired_side)
    names = {-1: "Model", 1: "Random", 0: "None"}
    assert [(g.initial_state["id"], g.winner) for g in games] == [(g, names[int(winner[g])]) for g in expect]
    assert all(g.player1 == "Model" and g.player2 == "Random" for g in games)
