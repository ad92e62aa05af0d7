"""The tic-tac-toe arena on the device: diee_ttt_arena with option "search" = "device" (k_ttt_arena_split / k_ttt_arena_move around k_ttt_search
and k_ttt_vanilla, die-e_amd/csrc/ttt_arena_kernels.hip) against "search" = "host" of the same ctxs over the device network (the round loop
of ttt_host.cpp, which tests/test_ttt_arena_cpu.py holds against the Python driver), every output bit for bit.  16 games per workgroup: at
17 games a side's list is 8 against 9 and one workgroup holds one game, at 40 both lists cross a workgroup."""
import pytest

import diee_amd

pytestmark = pytest.mark.gpu
M, R, V = diee_amd.AGENT_MODEL, diee_amd.AGENT_RANDOM, diee_amd.AGENT_MCTS


@pytest.fixture(scope="module")
def engines():
    es = []
    for seed in (0, 1):                                                    # "two models": two ctxs, two weight blobs
        e = diee_amd.Engine(0, diee_amd.GAME_TTT)
        e.load_weights(diee_amd.random_weights(seed, diee_amd.GAME_TTT))
        es.append(e.set_option("nn", "device"))
    yield es
    for e in es:
        e.close()


def _play(engines, search, agents, n, **kw):
    for e in engines:
        e.set_option("search", search)
    cfg = diee_amd.MctsConfig(iterations=20 if V in agents else 8, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)
    flags = [0 if a == V else diee_amd.FLAG_REF_QUIRKS for a in agents]      # the Mcts agent plays its rollouts
    r = diee_amd.ttt_arena(engines[0], agents[0], engines[1] if agents[1] != R else None, agents[1], n, cfg, 1.25, seed=7, flags=flags, **kw)
    for st in r["stats"]:
        assert st.pop("seconds") > 0.0
    r.pop("seconds")
    return {k: v.tobytes() if hasattr(v, "tobytes") else v for k, v in r.items()}


@pytest.mark.parametrize("agents,n,kw", [(ag, n, {}) for ag in ((M, M), (M, R), (V, R), (R, R)) for n in (1, 17, 40)]
                         + [((M, M), 17, {"round_limit": 3}), ((M, R), 17, {"max_rounds": 2})])
def test_device_arena_equals_the_host_loop(engines, agents, n, kw):
    want, got = _play(engines, "host", agents, n, **kw), _play(engines, "device", agents, n, **kw)
    for k in want:
        assert got[k] == want[k], k
    assert got["wins_p1"] + got["wins_p2"] + got["draws"] == (0 if kw.get("max_rounds") else n)
    searched = [a != R for a in agents]
    assert [st["move_steps"] > 0 and st["selections"] > 0 for st in got["stats"]] == searched      # the case does not pass empty


def test_refusals(engines):
    def status(*args):
        with pytest.raises(diee_amd.DieeError) as ei:
            diee_amd.ttt_arena(*args)
        return ei.value.status
    cfg = diee_amd.MctsConfig.default(4)
    bg = diee_amd.Engine(0)
    assert status(bg, R, None, R, 4, cfg) == diee_amd.ERR_UNSUPPORTED
    assert status(engines[0], R, bg, R, 4, cfg) == diee_amd.ERR_UNSUPPORTED
    bg.close()
    engines[0].set_option("search", "device"); engines[1].set_option("search", "host")
    assert status(engines[0], M, engines[1], M, 4, cfg) == diee_amd.ERR_ARG
