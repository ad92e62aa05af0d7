"""Option "search_fused" = "2" of a tic-tac-toe ctx: a self-play call without the quirks as ONE search-and-play launch of k_ttt_selfplay_run
plus the delivery (die-e_amd/csrc/ttt_selfplay_kernels.hip) against the SAME ctx on "1", the host loop over one k_ttt_search_run launch per
move-step, which tests/test_ttt_fused_gpu.py holds bit-exact to the host search.  16 games per workgroup; the tree is in LDS up to
"search_fused_lds_iters" iterations and in HBM above."""
import numpy as np
import pytest

import diee_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    e.set_option("nn", "device").set_option("search", "device")
    e.load_weights(diee_amd.random_weights(0, diee_amd.GAME_TTT))
    yield e
    e.close()


def _both(eng, call):
    out = []
    for fused in ("1", "2"):
        eng.set_option("search_fused", fused)
        assert eng.get_option("search_fused") == fused
        out.append((call(), int(eng.get_option("self_play_last_launches")), int(eng.get_option("search_last_launches"))))
    return out


def _same_records(f, d):
    for key in ("outcome", "game", "state", "ps"):
        assert f[key].dtype == d[key].dtype and f[key].shape == d[key].shape and f[key].tobytes() == d[key].tobytes(), key


# iters "L": the largest whose tree is kept in LDS, read from the ctx
@pytest.mark.parametrize("n,iters,round_limit,max_steps,temperature",
                         [(n, 30, 400, 0, 1.25) for n in (1, 16, 17, 37)] + [(17, i, 400, 0, 1.25) for i in (1, "L", "L+1")]
                         + [(37, 30, 3, 0, 1.25), (37, 30, 4, 0, 1.25), (37, 30, 400, 6, 1.25), (17, 30, 400, 0, 1.0)])
def test_self_play_equals_the_loop_of_one_search_per_move_step(eng, n, iters, round_limit, max_steps, temperature):
    lds = int(eng.get_option("search_fused_lds_iters"))
    iters = {"L": lds, "L+1": lds + 1}.get(iters, iters)
    cfg = diee_amd.MctsConfig(iterations=iters, c=2.0, round_limit=round_limit, dir_alpha=0.3, dir_eps=0.25)
    (d, d_sp, _), (f, f_sp, f_last) = _both(eng, lambda: eng.self_play_parallel(n, cfg, temperature, 77, ref_quirks=False, first_game_id=40,
                                                                                max_steps=max_steps))
    # the case does not pass empty (the reference path's output)
    assert d["stats"]["fragments"] == len(d["outcome"]) > 0 and d["stats"]["illegal_decodes"] == 0
    if n == 37 and round_limit == 400 and max_steps == 0:
        per_game = [set(d["outcome"][d["game"] == g]) for g in np.unique(d["game"])]
        assert {1, -1} in per_game and {0} in per_game                     # decided games and a drawn one
    if round_limit < 400:                                                   # the zero flush: round_limit fragments a game, the one recorded after it dropped
        assert not d["outcome"].any() and len(d["outcome"]) == n * round_limit and d["stats"]["plies"] == n * (round_limit + 1)
    if max_steps:
        assert 0 < len(np.unique(d["game"])) < n and d["stats"]["games"] == len(np.unique(d["game"]))
    assert d_sp == d["stats"]["move_steps"] and (f_sp, f_last) == (1, 1)
    _same_records(f, d)
    for key in d["stats"]:
        assert key == "seconds" or f["stats"][key] == d["stats"][key], key


def test_the_quirks_and_a_single_search_take_their_own_paths(eng):
    (d, _, _), (f, f_sp, _) = _both(eng, lambda: eng.self_play_parallel(19, diee_amd.MctsConfig.default(30), 1.25, 77, ref_quirks=True, first_game_id=40))
    assert len(d["outcome"]) > 0 and f_sp > 1                               # the host loop: a search, or more, per move-step
    _same_records(f, d)
    roots, cfg = diee_amd.ttt_new(17), diee_amd.MctsConfig.default(30)
    (d, _, _), (f, _, f_last) = _both(eng, lambda: eng.alpha_mcts_parallel(roots, cfg, 5, 2, ref_quirks=False))
    assert f_last == 1
    for key in ("probs", "root_visits", "n_children"):
        assert f[key].tobytes() == d[key].tobytes(), key


def test_the_options():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    e.load_weights(diee_amd.random_weights(0, diee_amd.GAME_TTT))

    def status(key, value):
        with pytest.raises(diee_amd.DieeError) as ei:
            e.set_option(key, value)
        return ei.value.status
    e.set_option("nn", "device")
    assert status("search_fused", "2") == diee_amd.ERR_ARG                  # before search = device
    assert e.get_option("self_play_last_launches") == "0"
    e.set_option("search", "device")
    assert status("search_fused", "3") == diee_amd.ERR_ARG and status("self_play_last_launches", "1") == diee_amd.ERR_ARG
    e.set_option("search_fused", "2")
    assert e.get_option("search_fused") == "2"
    e.set_option("search", "host")                                          # resets it
    assert e.get_option("search_fused") == "0" and e.get_option("self_play_last_launches") == "0"
    e.close()
