"""Agent::Mcts for tic-tac-toe on the device: diee_ttt_mcts_vanilla_batch with option "search" = "device" (k_ttt_vanilla,
die-e_amd/csrc/ttt_vanilla_kernels.hip) against the restatement tests/ttt_vanilla_ref.py, bit for bit.  16 games per workgroup, 4 per wave.
The tree of a game is in LDS up to 63 iterations (every case of 60, 1 or 0 iterations below) and in HBM beyond (the 200-iteration case and
the case that crosses the per-launch bound)."""
import numpy as np
import pytest

import diee_amd
from test_ttt_search_gpu import BOARDS, _roots
from ttt_vanilla_ref import assert_same, mct_search_batch

pytestmark = pytest.mark.gpu
ITERS_PER_LAUNCH = 4096                                                    # kVanillaItersPerLaunch of ttt_vanilla_device.h


@pytest.fixture(scope="module")
def eng():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)                              # no weights: the vanilla search needs none
    e.set_option("nn", "device").set_option("search", "device")
    yield e
    e.close()


def _check(eng, roots, iters, quirks, c=2.0, round_limit=400):
    n = len(roots)
    cfg = diee_amd.MctsConfig(iterations=iters, c=c, round_limit=round_limit, dir_alpha=0.3, dir_eps=0.25)
    ids, rounds = np.arange(n, dtype=np.uint32) * 7 + 3, np.arange(n, dtype=np.uint32) % 4 + 1
    got = eng.ttt_mct_search(roots, cfg, 11, ids, rounds, ref_quirks=bool(quirks))
    assert_same(got, mct_search_batch(roots, cfg, 11, ids, rounds, bool(quirks)))
    return got


# one row, a full wave, a wave plus one, a full workgroup, a workgroup plus one, a ragged third workgroup; no and one iteration; scores
# that are NaN or lack the exploration term; rollouts of zero, one and two plies; a tree in HBM (200 iterations)
@pytest.mark.parametrize("n,quirks,iters,c,round_limit", [(n, q, 60, 2.0, 400) for n in (1, 4, 5, 16, 17, 37) for q in (1, 0)]
                         + [(17, 1, 0, 2.0, 400), (17, 1, 1, 2.0, 400), (17, 1, 60, float("nan"), 400), (17, 0, 60, -1.0, 400)]
                         + [(17, 0, 60, 2.0, rl) for rl in (0, 1, 2)] + [(17, 0, 200, 2.0, 400)])
def test_device_search_equals_the_restatement(oracle, eng, n, quirks, iters, c, round_limit):
    roots = _roots(n)
    assert list(roots[0]["board"]) == BOARDS[0]
    got = _check(eng, roots, iters, quirks, c, round_limit)
    if iters >= 60:                                                         # the case does not pass empty
        assert got["n_children"][0] == 2 and got["stats"]["terminal_hits"] > 0
        assert quirks or round_limit == 0 or got["stats"]["rollout_decided"] > 0


def test_state_carries_over_launches(oracle, eng):
    """three roots with at most four empty cells: their trees (at most 65 nodes) are exhausted early, then every iteration is a terminal
    hit; the visit counts run into the thousands over three launches"""
    roots = _roots(5)[[0, 3, 4]]
    roots[1]["board"][[6, 8]] = (-1, 1)                                     # the mid-game board of BOARDS[3], two more cells taken: three left
    got = _check(eng, roots, 2 * ITERS_PER_LAUNCH + 3, 0)
    assert got["stats"]["terminal_hits"] > 2 * ITERS_PER_LAUNCH and got["child_visits"].max() > 1000.0


def test_a_backgammon_ctx_is_refused():
    e = diee_amd.Engine(0)
    with pytest.raises(diee_amd.DieeError) as ei:
        e.ttt_mct_search(_roots(2), diee_amd.MctsConfig.default(10))
    assert ei.value.status == diee_amd.ERR_UNSUPPORTED
    e.close()
