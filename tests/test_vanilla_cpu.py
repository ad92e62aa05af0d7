"""CPU tests of Agent::Mcts's host side: the ctypes mirror of diee_vanilla_stats, the arena driver serving an Mcts player through a
search object (here the Python restatement, tests/vanilla_ref.py), and the restatement's own invariants."""
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


def test_vanilla_stats_mirror_matches_the_header(tmp_path):
    """size and field offsets of diee_vanilla_stats as a C compiler lays out include/diee.h, against die-e_amd.VanillaStats"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed"
    fields = [n for n, _ in diee_amd.VanillaStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "diee.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(diee_vanilla_stats));\n'
                   + "".join(f'    printf(" %zu", offsetof(diee_vanilla_stats, {f}));\n' for f in fields)
                   + '    printf(" %d %zu\\n", DIEE_AGENT_MCTS, sizeof(diee_stats));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(diee_amd.VanillaStats) == 8 * 8 + 8
    assert out[1:1 + len(fields)] == [getattr(diee_amd.VanillaStats, f).offset for f in fields]
    assert out[-2] == diee_amd.AGENT_MCTS == 2
    assert out[-1] == C.sizeof(diee_amd.Stats)                 # diee_stats keeps its size
    assert "diee_mcts_vanilla_batch" in diee_amd.EXPORTS and hasattr(diee_amd.Engine, "mct_search")


def _summary(res):
    return (res.wins_p1, res.wins_p2, res.draws, res.rounds, res.final_states.tobytes(),
            [(g.initial_state["id"], g.winner) for g in res.games])


def test_play_serves_an_mcts_player_through_a_search_object(oracle):
    """versus.play(Mcts, Random) on the oracle's rules with the restatement as the search: 4 games to the end -- play() itself asserts
    that every action it applies is one of the state's legal plays (versus.rs:229) --, and the same games for the same seed"""
    from oracle.arena_backend import OracleRules
    from vanilla_ref import RefSearch
    P = versus.Player
    cfg = diee_amd.MctsConfig(iterations=5, c=2.0, round_limit=6, dir_alpha=0.3, dir_eps=0.25)
    calls = []

    class Counting(RefSearch):
        def vanilla(self, states, c, seed, ids, rounds, ref_quirks):
            calls.append((len(states), ref_quirks))
            return super().vanilla(states, c, seed, ids, rounds, ref_quirks)

    def run(**kw):
        return versus.play(P(versus.Agent.MCTS), P(versus.Agent.RANDOM), cfg, 1.25, seed=41, num_games=4, round_limit=400,
                           rules=OracleRules(), search1=Counting(), **kw)
    a = run(vanilla_rollouts=True)
    assert a.wins_p1 + a.wins_p2 + a.draws == 4 and len(a.games) == 4 and a.wins_p1 + a.wins_p2 > 0
    assert all(g.player1 == "Mcts" and g.player2 == "Random" for g in a.games)
    assert calls and not any(q for _, q in calls)                               # vanilla_rollouts=True: the quirk is off
    b = run(vanilla_rollouts=True)
    assert _summary(a) == _summary(b)
    del calls[:]
    c = run()                                                                   # the default: the reference's agent as written
    assert calls and all(q for _, q in calls) and c.wins_p1 + c.wins_p2 + c.draws == 4
    # an Mcts player on the other side, and neither an engine nor a search object: refused
    d = versus.play(P(versus.Agent.RANDOM), P(versus.Agent.MCTS), cfg, 1.25, seed=41, num_games=2, round_limit=12, rules=OracleRules(),
                    search2=RefSearch())
    assert d.rounds <= 12 and d.wins_p1 + d.wins_p2 + d.draws == 2
    with pytest.raises(NotImplementedError):
        versus.play(P(versus.Agent.RANDOM), P(versus.Agent.MCTS), cfg, 1.25, num_games=2, rules=OracleRules())
    with pytest.raises(NotImplementedError):
        versus.play_tictactoe(P(versus.Agent.MCTS), P(versus.Agent.RANDOM), cfg, 1.25, num_games=2)


def test_edge_case_roots_meet_their_preconditions(oracle):
    """tests/vanilla_cases.py: the roots of tests/test_vanilla_edges_gpu.py have the play counts the cases are about, and the
    restatement alone takes the paths they are about -- selection through roots wider than a wavefront, scores that are NaN where
    that changes the answer, rollouts of zero, one and two plies"""
    import vanilla_cases as vc
    assert len(vc.wide_roots()) == 6 and len(vc.const_roots()) == 5          # (the builders assert the play counts and off = [5, 6])
    for quirks in (True, False):
        beyond = vc.check_wide(quirks)
        print(vc.line(f"wide roots, quirks {'on' if quirks else 'off'}, {beyond} descents beyond depth 1", vc.wide_reference(quirks)["stats"]))
    differ = vc.check_consts()
    print(vc.line(f"c = -1.0 (differs from c = 0.0 on roots {differ})", vc.const_reference(-1.0)["stats"]))
    print(vc.line("c = 0.0", vc.const_reference(0.0)["stats"]))
    for rl, st in vc.check_limits().items():
        print(vc.line(f"round_limit {rl}, quirks off", st))


@pytest.mark.parametrize("quirks", [True, False])
def test_invariants_of_the_restatement(oracle, quirks):
    from vanilla_ref import mct_search
    walk = oracle.random_walk_states(5, 12, 400)
    late = walk[walk["off"].max(axis=1) >= 12][::3][:6]
    roots = [oracle.bg_new()] + [late[i] for i in range(len(late))]
    roots[0]["roll"] = (3, 1)
    assert len(roots) == 7, len(roots)
    terminal_seen = False
    for g, root in enumerate(roots):
        for iterations in (0, 3, 25):
            r = mct_search(root, iterations, 2.0, 12, seed=9, game_id=g, rnd=2, ref_quirks=quirks)
            nodes, st = r["nodes"], r["stats"]
            if iterations == 0:
                assert (r["play"] == oracle.NO_MOVE).all() and r["n_children"] == 0
                continue
            assert st["iterations"] == iterations == int(nodes[0].visits)               # the root is on every backpropagated path
            assert int(r["child_visits"].sum()) == int(nodes[0].visits)                 # ... and so is exactly one of its children
            assert len(nodes) == 1 + st["expansions"] and st["rollouts"] == st["expansions"] + st["dead_end_hits"]
            assert st["iterations"] == st["terminal_hits"] + st["rollouts"]
            for i, nd in enumerate(nodes):                      # a node with children started one backpropagation: when it was created
                below = sum(int(nodes[c].visits) for c in nd.children)
                assert int(nd.visits) == (below if i == 0 else 1 + below if nd.children else int(nd.visits)) >= 1
            finished = [nd for nd in nodes if oracle.bg_check_winner(nd.state) is not None]
            terminal_seen = terminal_seen or bool(finished)
            if quirks and not finished:
                assert all(float(nd.value) == 0.0 for nd in nodes) and st["rollout_plies"] == 0 and st["rollout_decided"] == 0
            if quirks:
                assert st["rollout_plies"] == 0
            legal = [oracle.play_np(p).tolist() for p in oracle.bg_valid_moves(oracle.bg_state(
                pts=root["pts"], bar=root["bar"], off=root["off"], roll=root["roll"], player=root["player"], second=root["second"]))]
            assert r["play"].tolist() in legal
    assert terminal_seen                                                        # late roots: the values' other branch was reached
