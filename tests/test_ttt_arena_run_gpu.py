"""Option "search_fused" = "2" of the ctx that hosts diee_ttt_arena: a call of Model and Random players without the quirks as ONE launch of
k_ttt_arena_run (die-e_amd/csrc/ttt_arena_run_kernels.hip) against the same ctxs on "0", the round loop over k_ttt_search, which
tests/test_ttt_arena_gpu.py holds to the host loop: every output byte for byte.  The two halves of a call are mapped to workgroups of 16
games separately: 1 game is an empty first half, 17 are halves of 8 and 9, 33 are 16 and 17, so a workgroup holds one game."""
import pytest

import diee_amd

pytestmark = pytest.mark.gpu
M, R, V = diee_amd.AGENT_MODEL, diee_amd.AGENT_RANDOM, diee_amd.AGENT_MCTS
Q = diee_amd.FLAG_REF_QUIRKS


@pytest.fixture(scope="module")
def engines():
    es = []
    for seed in (0, 1):                                                    # "two models": two ctxs, two weight blobs
        e = diee_amd.Engine(0, diee_amd.GAME_TTT)
        e.load_weights(diee_amd.random_weights(seed, diee_amd.GAME_TTT))
        es.append(e.set_option("nn", "device").set_option("search", "device"))
    yield es
    for e in es:
        e.close()


def _both(engines, agents, n, iters=8, temperature=1.25, flags=(0, 0), round_limit=400, **kw):
    """the call on "0" and on "2": (outputs, arena_last_launches) of each"""
    cfg = diee_amd.MctsConfig(iterations=iters, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)
    out = []
    for fused in ("0", "2"):
        for e in engines:
            e.set_option("search_fused", fused)
        r = diee_amd.ttt_arena(engines[0], agents[0], engines[1], agents[1], n, cfg, temperature, seed=7, round_limit=round_limit, flags=list(flags), **kw)
        for st in r["stats"]:
            assert st.pop("seconds") > 0.0
        r.pop("seconds")
        out.append(({k: v.tobytes() if hasattr(v, "tobytes") else v for k, v in r.items()}, int(engines[0].get_option("arena_last_launches"))))
    (want, _), (got, _) = out
    assert set(got) == set(want) >= {"winner", "retired_round", "retired_side", "final_states", "wins_p1", "wins_p2", "draws", "rounds", "stats"}
    for k in want:
        assert got[k] == want[k], k
    return out


# iters "L+1": the smallest whose tree lies in HBM, read from the ctx
@pytest.mark.parametrize("agents,n,iters,kw", [(ag, n, 8, {}) for ag in ((M, M), (M, R), (R, M), (R, R)) for n in (1, 17, 33)]
                         + [((M, M), 17, "L+1", {}), ((M, M), 17, 8, {"round_limit": 3}), ((M, R), 17, 8, {"max_rounds": 2})])
def test_one_launch_equals_the_round_loop(engines, agents, n, iters, kw):
    if iters == "L+1":
        iters = int(engines[0].get_option("search_fused_lds_iters")) + 1
    (want, loop), (got, one) = _both(engines, agents, n, iters, **kw)
    assert one == 1 and (loop > 1 or M not in agents)
    assert want["wins_p1"] + want["wins_p2"] + want["draws"] == (0 if kw.get("max_rounds") else n)
    searched = [a == M for a in agents]
    assert [st["move_steps"] > 0 and st["selections"] > 0 for st in want["stats"]] == searched      # the case does not pass empty


@pytest.mark.parametrize("agents,iters,flags", [((M, R), 8, (Q, 0)), ((M, M), 8, (0, Q)), ((V, M), 20, (0, 0))])
def test_the_quirks_and_an_mcts_player_keep_the_round_loop(engines, agents, iters, flags):
    (want, _), (_, launches) = _both(engines, agents, 17, iters, flags=flags)
    assert launches > 1 and want["wins_p1"] + want["wins_p2"] + want["draws"] == 17


def test_a_call_that_outlasts_nine_rounds_is_replayed_on_the_round_loop(engines):
    # 1 / temperature = 1000: det_powf flushes every row whose largest entry is not 1 to zeros, and an all-zero row skips the turn
    (want, _), (_, launches) = _both(engines, (M, M), 17, 8, temperature=0.001, max_rounds=12)
    assert want["rounds"] == 12                                             # some game is alive past round 9 (the reference run)
    assert launches > 1


def test_the_option(engines):
    with pytest.raises(diee_amd.DieeError) as ei:
        engines[0].set_option("arena_last_launches", "1")
    assert ei.value.status == diee_amd.ERR_ARG
    assert _both(engines, (R, R), 1)[1][1] == 1
    engines[0].set_option("search", "host")
    assert engines[0].get_option("arena_last_launches") == "0"
    engines[0].set_option("search", "device")
