"""Agent::Mcts for tic-tac-toe on the host (diee_ttt_mcts_vanilla_batch on a default ctx; die-e_amd/csrc/ttt_host.cpp) against the
restatement tests/ttt_vanilla_ref.py, bit for bit: moves, the root's children and every counter.  Needs no GPU."""
import itertools

import numpy as np
import pytest

import diee_amd
from diee_amd import versus
from test_ttt_search_gpu import _roots
from ttt_vanilla_ref import assert_same, mct_search_batch

N = 9                                                                      # the seven boards, the first two twice
IDS, ROUNDS = np.arange(N, dtype=np.uint32) * 7 + 3, np.arange(N, dtype=np.uint32) % 4 + 1


def _cfg(iters, c=2.0, round_limit=400):
    return diee_amd.MctsConfig(iterations=iters, c=c, round_limit=round_limit, dir_alpha=0.3, dir_eps=0.25)


@pytest.fixture(scope="module")
def eng():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    assert e.get_option("search") == "host"
    yield e
    e.close()


@pytest.mark.parametrize("quirks,iters,round_limit,c", itertools.product((1, 0), (0, 1, 60), (0, 1, 2, 400), (2.0, -1.0, float("nan"))))
def test_host_search_equals_the_restatement(oracle, eng, quirks, iters, round_limit, c):
    roots, cfg = _roots(N), _cfg(iters, c, round_limit)
    got = eng.ttt_mct_search(roots, cfg, 11, IDS, ROUNDS, ref_quirks=bool(quirks))
    assert_same(got, mct_search_batch(roots, cfg, 11, IDS, ROUNDS, bool(quirks)))
    assert got["moves"][5] == 10 and got["moves"][6] == 10                 # the full board and the won one run no iteration
    if iters == 60:
        assert got["n_children"][0] == 2 and got["stats"]["terminal_hits"] > 0
        assert quirks or round_limit == 0 or got["stats"]["rollout_decided"] > 0


def test_default_keys_are_the_index_and_round_zero(oracle, eng):
    roots, cfg = _roots(4), _cfg(30)
    assert_same(eng.ttt_mct_search(roots, cfg, 5, ref_quirks=False), mct_search_batch(roots, cfg, 5, None, None, False))


def test_play_tictactoe_serves_an_mcts_player(eng):
    P, cfg = versus.Player, _cfg(40)
    runs = [versus.play_tictactoe(P(versus.Agent.MCTS, eng), P(versus.Agent.RANDOM), cfg, 1.25, seed=9, num_games=6, vanilla_rollouts=True) for _ in range(2)]
    assert runs[0].rounds <= 9 and not (runs[0].final_states["board"] == 0).all(axis=1).any()
    assert runs[0].final_states.tobytes() == runs[1].final_states.tobytes() and runs[0].wins_p1 == runs[1].wins_p1


def test_error_codes(eng):
    def status(e, roots, cfg):
        with pytest.raises(diee_amd.DieeError) as ei:
            e.ttt_mct_search(roots, cfg)
        return ei.value.status
    bad = _roots(3)
    bad[1]["board"][4] = 2
    assert status(eng, bad, _cfg(10)) == diee_amd.ERR_ARG
    bad = _roots(3)
    bad[2]["player"] = 0
    assert status(eng, bad, _cfg(10)) == diee_amd.ERR_ARG
    assert status(eng, _roots(3), _cfg(1 << 20)) == diee_amd.ERR_ARG
    assert status(eng, _roots(3), _cfg(10, round_limit=4095)) == diee_amd.ERR_ARG
