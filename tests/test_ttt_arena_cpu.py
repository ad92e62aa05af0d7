"""The tic-tac-toe arena in one engine call on the host path (diee_ttt_arena on default ctxs; die-e_amd/csrc/ttt_host.cpp: Engine::arena)
against the Python driver versus.play_tictactoe, field by field.  Temperature 1.0: x ** 1 is x for both power functions, so the two
drivers sample from the same rows.  Needs no GPU."""
import pytest

import diee_amd
from diee_amd import versus

A = versus.Agent
KIND = {A.MODEL: diee_amd.AGENT_MODEL, A.RANDOM: diee_amd.AGENT_RANDOM, A.MCTS: diee_amd.AGENT_MCTS}


@pytest.fixture(scope="module")
def engines():
    es = []
    for seed in (0, 1):                                                    # "two models": two weight blobs
        e = diee_amd.Engine(0, diee_amd.GAME_TTT)
        e.load_weights(diee_amd.random_weights(seed, diee_amd.GAME_TTT))
        es.append(e)
    yield es
    for e in es:
        e.close()


def _cfg(iters, round_limit=400):
    return diee_amd.MctsConfig(iterations=iters, c=2.0, round_limit=round_limit, dir_alpha=0.3, dir_eps=0.25)


@pytest.mark.parametrize("agents,n,round_limit", [(ag, n, 400) for ag in ((A.MODEL, A.MODEL), (A.MODEL, A.RANDOM), (A.RANDOM, A.MCTS)) for n in (1, 6)]
                         + [((A.MODEL, A.RANDOM), 6, 3)])
def test_one_call_equals_the_python_driver(engines, agents, n, round_limit):
    """round_limit = 3 retires every game as a draw in round 2: nobody has three marks before round 4"""
    cfg = _cfg(20 if A.MCTS in agents else 8)
    p1, p2 = (versus.Player(a, None if a == A.RANDOM else engines[s]) for s, a in enumerate(agents))
    want = versus.play_tictactoe(p1, p2, cfg, 1.0, seed=5, num_games=n, round_limit=round_limit, vanilla_rollouts=True)
    got = versus.play_tictactoe_device(p1, p2, cfg, 1.0, seed=5, num_games=n, round_limit=round_limit, vanilla_rollouts=True, engine=engines[0])
    assert (got.wins_p1, got.wins_p2, got.draws, got.rounds) == (want.wins_p1, want.wins_p2, want.draws, want.rounds)
    assert got.final_states.tobytes() == want.final_states.tobytes()
    r = got.device
    assert got.wins_p1 + got.wins_p2 + r["draws"] == n and (r["retired_round"] < got.rounds).all()
    assert [st["games"] for st in r["stats"]] == [int((r["retired_side"] == s).sum()) for s in (0, 1)]
    assert sum(st["plies"] for st in r["stats"]) == int((r["retired_round"] + 1).sum())     # a live game takes one turn per round
    if round_limit == 3:
        assert got.rounds == 3 and r["draws"] == n and (r["retired_round"] == 2).all()


def test_max_rounds_stops_the_call(engines):
    r = engines[0].ttt_arena(diee_amd.AGENT_MODEL, engines[1], diee_amd.AGENT_MODEL, 6, _cfg(8), 1.0, seed=5, max_rounds=2)
    full = engines[0].ttt_arena(diee_amd.AGENT_MODEL, engines[1], diee_amd.AGENT_MODEL, 6, _cfg(8), 1.0, seed=5)
    assert r["rounds"] == 2 and (r["retired_round"] == 0xFFFFFFFF).all() and (r["winner"] == 0).all() and (r["retired_side"] == -1).all()
    assert ((r["final_states"]["board"] != 0).sum(axis=1) == 2).all() and full["rounds"] > 2
    assert [st["move_steps"] for st in r["stats"]] == [2, 2] and r["stats"][0]["nn_evals"] > 0


def test_refusals(engines):
    def status(*args, **kw):
        with pytest.raises(diee_amd.DieeError) as ei:
            diee_amd.ttt_arena(*args, **kw)
        return ei.value.status
    M, R = diee_amd.AGENT_MODEL, diee_amd.AGENT_RANDOM
    bare = diee_amd.Engine(0, diee_amd.GAME_TTT)
    assert status(engines[0], M, None, M, 4, _cfg(4)) == diee_amd.ERR_ARG                  # a Model agent without ctx
    assert status(engines[0], M, bare, M, 4, _cfg(4)) == diee_amd.ERR_NO_WEIGHTS
    assert status(engines[0], M, None, R, 0, _cfg(4)) == diee_amd.ERR_ARG
    assert status(engines[0], M, None, R, 4, _cfg(4), round_limit=0) == diee_amd.ERR_ARG
    assert status(engines[0], 7, None, R, 4, _cfg(4)) == diee_amd.ERR_ARG
    assert diee_amd.load_library().diee_ttt_arena(None, R, None, R, 4, None, 1.0, 0, 9, 0, None, None, None, None, None, None, None) == diee_amd.ERR_ARG
    assert diee_amd.ttt_arena(None, R, bare, R, 4, _cfg(4))["rounds"] >= 5                  # a weightless ctx hosts Random players
    bare.close()
