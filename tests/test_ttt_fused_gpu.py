"""Option "search_fused" = "1" of a tic-tac-toe ctx: the device search as ONE launch of k_ttt_search_run
(die-e_amd/csrc/ttt_search_run_kernels.hip) against the SAME ctx with "search_fused" = "0", one launch of k_ttt_search per iteration, which
tests/test_ttt_search_gpu.py holds bit-exact to the host search.  16 games per workgroup; the tree is in LDS up to "search_fused_lds_iters"
iterations and in HBM above; under the quirks only a call of at most 16 roots is fused."""
import numpy as np
import pytest

import diee_amd
from test_ttt_search_gpu import BOARDS, KEYS, _cfg, _roots

pytestmark = pytest.mark.gpu
M = diee_amd.AGENT_MODEL


@pytest.fixture(scope="module")
def eng():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    e.set_option("nn", "device").set_option("search", "device")
    e.load_weights(diee_amd.random_weights(0, diee_amd.GAME_TTT))
    yield e
    e.close()


def _both(eng, call):
    out = []
    for fused in ("0", "1"):
        eng.set_option("search_fused", fused)
        out.append((call(), int(eng.get_option("search_last_launches"))))
    return out


# iters "L": the largest whose tree is kept in LDS, read from the ctx
@pytest.mark.parametrize("n,quirks,iters,c", [(n, 0, 60, 2.0) for n in (1, 16, 17, 37)] + [(17, 0, i, 2.0) for i in (0, 1, "L", "L+1")]
                         + [(17, 0, 60, float("nan")), (1, 1, 60, 2.0), (16, 1, 60, 2.0), (17, 1, 60, 2.0)])
def test_mcts_batch_equals_the_search_of_one_launch_per_iteration(eng, n, quirks, iters, c):
    lds = int(eng.get_option("search_fused_lds_iters"))
    assert 50 <= lds < 60                                                   # the default 50 iterations fit; 60 is the HBM placement
    iters = {"L": lds, "L+1": lds + 1}.get(iters, iters)
    roots, cfg = _roots(n), _cfg(iters, c)
    assert list(roots[0]["board"]) == BOARDS[0]
    (d, d_launches), (f, f_launches) = _both(eng, lambda: eng.alpha_mcts_parallel(roots, cfg, 5, 2, ref_quirks=bool(quirks)))
    assert d_launches == iters + 1 and f_launches == (iters + 1 if quirks and n > 16 else 1)
    for key in ("probs", "root_visits", "n_children"):
        assert np.array_equal(f[key], d[key], equal_nan=True) and f[key].tobytes() == d[key].tobytes(), key
    for key in KEYS:
        assert f["stats"][key] == d["stats"][key], key
    if iters == 60 and c == 2.0:                                            # the case does not pass empty
        assert d["stats"]["terminal_hits"] > 0
        assert n != 1 or d["stats"]["nn_evals"] < iters + 1                 # iterations in which nobody selected: the evaluation is skipped


def test_self_play_equals_the_search_of_one_launch_per_iteration(eng):
    (d, _), (f, launches) = _both(eng, lambda: eng.self_play_parallel(19, _cfg(30), 1.25, 77, ref_quirks=False, first_game_id=40))
    assert len(d["outcome"]) > 0 and launches == 1
    for key in ("outcome", "game", "state", "ps"):
        assert f[key].tobytes() == d[key].tobytes(), key


def test_arena_equals_the_search_of_one_launch_per_iteration(eng):
    other = diee_amd.Engine(0, diee_amd.GAME_TTT)
    other.load_weights(diee_amd.random_weights(1, diee_amd.GAME_TTT))
    other.set_option("nn", "device").set_option("search", "device")

    def play():
        r = diee_amd.ttt_arena(eng, M, other, M, 17, _cfg(8), 1.25, seed=7, flags=[0, 0])
        for st in r["stats"]:
            assert st.pop("seconds") > 0.0 and st["selections"] > 0
        r.pop("seconds")
        return {k: v.tobytes() if hasattr(v, "tobytes") else v for k, v in r.items()}
    (d, d_launches), (f, f_launches) = _both(eng, play)
    other.close()
    assert (d_launches, f_launches) == (9, 1) and f == d


def test_the_options():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    e.load_weights(diee_amd.random_weights(0, diee_amd.GAME_TTT))

    def status(key, value):
        with pytest.raises(diee_amd.DieeError) as ei:
            e.set_option(key, value)
        return ei.value.status
    e.set_option("nn", "device")
    assert status("search_fused", "1") == diee_amd.ERR_ARG                  # before search = device
    e.set_option("search_fused", "0")
    e.set_option("search", "device")
    assert e.get_option("search_fused") == "0" and e.get_option("search_last_launches") == "0"
    assert status("search_fused", "yes") == diee_amd.ERR_ARG
    assert status("search_last_launches", "1") == diee_amd.ERR_ARG and status("search_fused_lds_iters", "50") == diee_amd.ERR_ARG
    assert status("refill_width", "2") == diee_amd.ERR_UNSUPPORTED
    e.set_option("search_fused", "1")
    assert e.get_option("search_fused") == "1"
    e.set_option("search", "host")                                          # resets it
    assert e.get_option("search_fused") == "0"
    e.set_option("search", "device")
    assert e.get_option("search_fused") == "0"
    e.close()
