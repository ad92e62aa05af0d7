"""Option "search" = "device" of a tic-tac-toe ctx: alpha_mcts_parallel as one launch of k_ttt_search per iteration
(die-e_amd/csrc/ttt_search_kernels.hip), against the SAME ctx with "search" = "host": the host search over the device network, which
tests/test_ttt_device_gpu.py holds bit-exact to the oracle.  16 games per workgroup, 4 per wave."""
import numpy as np
import pytest

import diee_amd

pytestmark = pytest.mark.gpu
# game 0: two empty cells, its tree is exhausted after a handful of iterations whatever the network says; then the five boards of the
# search test of test_ttt_device_gpu.py in turn (game 16 is the empty board), the full board, a position won with cells left
BOARDS = [[1, -1, 1, -1, -1, 1, 0, 1, 0], [-1, 1, 0, 0, -1, 0, 0, 0, 1], [0] * 9, [-1, -1, 0, 1, 1, 0, 0, 0, 0], [-1, 1, -1, -1, 1, 1, 0, 0, 0],
          [1, -1, 1, 1, -1, -1, -1, 1, 1], [-1, -1, -1, 1, 1, 0, 0, 0, 0]]
KEYS = ("nn_evals", "expansions", "children", "max_children", "selections", "depth_sum", "terminal_hits")


def _roots(n):
    s = diee_amd.ttt_new(n)
    for i in range(n):
        b = BOARDS[i % len(BOARDS)]
        s[i]["board"] = b
        s[i]["player"] = -1 if sum(1 for x in b if x) % 2 == 0 else 1
    return s


@pytest.fixture(scope="module")
def eng():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    e.set_option("nn", "device")
    e.load_weights(diee_amd.random_weights(0, diee_amd.GAME_TTT))
    yield e
    e.close()


def _cfg(iters, c=2.0):
    return diee_amd.MctsConfig(iterations=iters, c=c, round_limit=400, dir_alpha=0.3, dir_eps=0.25)


@pytest.mark.parametrize("n,quirks,iters,c", [(n, q, 60, 2.0) for n in (1, 16, 17, 37) for q in (1, 0)]
                         + [(17, 1, 0, 2.0), (17, 1, 1, 2.0), (17, 1, 60, float("nan"))])
def test_mcts_batch_equals_the_host_search(eng, n, quirks, iters, c):
    roots, cfg = _roots(n), _cfg(iters, c)
    assert list(roots[0]["board"]) == BOARDS[0] and roots[0]["player"] == 1 and (n < 17 or not roots[16]["board"].any())
    eng.set_option("search", "host")
    h = eng.alpha_mcts_parallel(roots, cfg, 5, 2, ref_quirks=bool(quirks))
    if iters == 60 and c == 2.0:                                            # the case does not pass empty
        assert h["stats"]["terminal_hits"] > 0
        assert n != 1 or h["stats"]["nn_evals"] < 61                        # iterations in which nobody selected: a flag word stays clear
        if n == 17 and quirks:                                              # the stale slot of game 0, driven from the second workgroup
            assert eng.alpha_mcts_parallel(roots, cfg, 5, 2, ref_quirks=False)["root_visits"][0] != h["root_visits"][0]
    eng.set_option("search", "device")
    d = eng.alpha_mcts_parallel(roots, cfg, 5, 2, ref_quirks=bool(quirks))
    for key in ("probs", "root_visits", "n_children"):
        assert np.array_equal(d[key], h[key], equal_nan=True), key
    for key in KEYS:
        assert d["stats"][key] == h["stats"][key], key


def test_a_tree_past_65535_nodes_equals_the_host_search(eng):
    """RunNode::link keeps first_child in 20 bits: one empty-board root searched until its node indices pass 16 bits.  At c = 2.0 the tree
    stops growing near 13 000 children (the host search over the fp32 host network: 12 401 at 15 000 iterations, 13 019 at 40 000: the
    descents end on finished games), at c = 8.0 near 47 000 (45 797 at 20 000, 47 006 at 40 000); c = 32.0 gave 99 612 at 30 000."""
    roots, cfg = diee_amd.ttt_new(1), _cfg(30000, 32.0)
    eng.set_option("search", "host")
    h = eng.alpha_mcts_parallel(roots, cfg, 5, 2, ref_quirks=False)
    assert h["stats"]["children"] >= 65536                                  # children + 1 = the tree's nodes: the case does not pass empty
    eng.set_option("search", "device")
    d = eng.alpha_mcts_parallel(roots, cfg, 5, 2, ref_quirks=False)
    for key in ("probs", "root_visits", "n_children"):
        assert np.array_equal(d[key], h[key], equal_nan=True), key
    for key in KEYS:
        assert d["stats"][key] == h["stats"][key], key


@pytest.mark.parametrize("quirks", [1, 0])
def test_self_play_equals_the_host_search(eng, quirks):
    out = {}
    for where in ("host", "device"):
        eng.set_option("search", where)
        out[where] = eng.self_play_parallel(19, _cfg(30), 1.25, 77, ref_quirks=bool(quirks), first_game_id=40)
    assert len(out["host"]["outcome"]) > 0
    for key in ("outcome", "game", "state", "ps"):
        assert out["device"][key].tobytes() == out["host"][key].tobytes(), key


def test_the_option():
    blob = diee_amd.random_weights(0, diee_amd.GAME_TTT)
    e, fresh = diee_amd.Engine(0, diee_amd.GAME_TTT), diee_amd.Engine(0, diee_amd.GAME_TTT)
    e.load_weights(blob); fresh.load_weights(blob); fresh.set_option("nn", "device")

    def refused(key, value):
        with pytest.raises(diee_amd.DieeError) as ei:
            e.set_option(key, value)
        assert ei.value.status == diee_amd.ERR_ARG
    refused("search", "device")                                             # before nn = device
    e.set_option("nn", "device"); e.set_option("search", "device")
    assert e.get_option("search") == "device"
    refused("nn", "host")
    refused("search", "fast")
    e.set_option("search", "host")
    assert e.get_option("search") == "host"
    a, b = (x.alpha_mcts_parallel(_roots(17), _cfg(20), 5, 2) for x in (e, fresh))
    assert a["probs"].tobytes() == b["probs"].tobytes() and a["stats"]["nn_evals"] == b["stats"]["nn_evals"]
    e.close(); fresh.close()
