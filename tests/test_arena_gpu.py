"""GPU tests of the device-resident arena (diee_arena / Engine.arena / versus.play_device): the games of one engine call are the
games of versus.play -- the Python driver over diee_mcts_batch, itself pinned to the oracle -- bit for bit: final states, result,
and the retired games with their winners IN ORDER."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

versus = importlib.import_module("die-e_amd.versus")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = versus.Player
MODEL, RANDOM = versus.Agent.MODEL, versus.Agent.RANDOM
SEED_SKIPS = 21           # case 7: a seed whose 8 games (case 1) contain skipped turns (a checker on the bar facing six made points)


@pytest.fixture(scope="module")
def engines():
    import diee_amd
    e1 = diee_amd.Engine(0); e1.load_weights(diee_amd.random_weights(0))
    e2 = diee_amd.Engine(0); e2.load_weights(diee_amd.random_weights(1))
    yield e1, e2
    e1.close(); e2.close()


def cfg_of(iterations):
    import diee_amd
    return diee_amd.MctsConfig(iterations=iterations, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)


def games_of(res):
    return [(g.initial_state["id"], g.winner) for g in res.games]


def assert_same(dev, ref):
    assert dev.final_states.tobytes() == ref.final_states.tobytes()
    assert (dev.wins_p1, dev.wins_p2, dev.draws, dev.rounds) == (ref.wins_p1, ref.wins_p2, ref.draws, ref.rounds)
    assert games_of(dev) == games_of(ref)                                     # in play()'s order of retirement
    assert dev.device["illegal_decodes"] == 0


def both(p1, p2, cfg, seed, n, limit, max_rounds=0, engine=None):
    dev = versus.play_device(p1, p2, cfg, 1.25, seed=seed, num_games=n, round_limit=limit, max_rounds=max_rounds, engine=engine)
    kw = {"rules": versus.EngineRules(engine)} if engine is not None else {}
    ref = versus.play(p1, p2, cfg, 1.25, seed=seed, num_games=n, round_limit=limit, max_rounds=max_rounds, **kw)
    assert_same(dev, ref)
    return dev, ref


def skipped_turns(dev):
    """turns in which no move was applied (include/diee.h: stats[s].plies counts every turn, fragments the applied moves)"""
    return sum(s["plies"] - s["fragments"] for s in dev.device["stats"])


def test_case1_eight_games_to_completion_and_the_oracle(engines, oracle):
    """k_tail sizes, real wins; once more against the arena on the oracle's rules and search (independent of the engine's search)"""
    from oracle.arena_backend import OracleRules, OracleSearch
    e1, e2 = engines
    cfg = cfg_of(6)
    dev, ref = both(P(MODEL, e1), P(MODEL, e2), cfg, SEED_SKIPS, 8, 400)
    assert dev.wins_p1 + dev.wins_p2 + dev.draws == 8 and dev.wins_p1 + dev.wins_p2 > 0
    assert len(dev.games) == 8
    # case 7: the skip path ran (and the Python driver agrees on every state behind it)
    assert skipped_turns(dev) > 0
    st = dev.device["stats"]
    assert st[0]["move_steps"] > 0 and st[1]["move_steps"] > 0 and st[0]["expansions"] > 0 and st[1]["expansions"] > 0
    assert st[0]["games"] + st[1]["games"] == 8

    def ev(e):
        return oracle.make_eval(lambda s: e.forward_t(s.view(oracle.BG_STATE).reshape(-1)), 1352)
    f1, f2 = ev(e1), ev(e2)
    orc = versus.play(P(MODEL), P(MODEL), cfg, 1.25, seed=SEED_SKIPS, num_games=8, round_limit=400, rules=OracleRules(),
                      search1=OracleSearch(f1), search2=OracleSearch(f2))
    assert_same(dev, orc)


def test_case2_96_games_through_the_kernel_families(engines):
    """each side starts at 48 games (fused family, free-running search); the limit of 60 rounds retires the games that move in round
    59 as draws and leaves the few that had to skip that turn to play on among themselves (cluster family / k_tail sizes)"""
    e1, e2 = engines
    dev, _ = both(P(MODEL, e1), P(MODEL, e2), cfg_of(8), SEED_SKIPS, 96, 60)
    assert dev.draws > 0
    assert dev.wins_p1 + dev.wins_p2 + dev.draws == 96
    rr = dev.device["retired_round"]
    live_at = lambda r: int((rr >= r).sum())
    # round 0: all 96 games alive, 48 to move on each side by construction (versus.rs:172-174)
    assert live_at(0) == 96 and int((dev.device["initial_states"]["player"] == -1).sum()) == 48 >= 41
    st = dev.device["stats"]
    # band_launches[b] = that player's turns whose list had a size in band b (<= 16, 32, 64, ...): a side of 33 ... 64 and one of <= 16 games
    assert st[0]["band_launches"][2] + st[1]["band_launches"][2] > 0
    assert st[0]["band_launches"][0] + st[1]["band_launches"][0] > 0
    assert any(0 < live_at(r) <= 16 for r in range(dev.rounds))


@pytest.mark.parametrize("variant", ["quirks", "no_quirks", "launch_per_iteration"])
def test_case3_five_rounds(engines, variant):
    import diee_amd
    e1, e2 = engines
    cfg = cfg_of(8)
    if variant == "no_quirks":
        # the Python driver searches with the quirks on: without them the reference is a driver over the same searches without them
        class NoQuirks(versus.EngineSearch):
            def mcts(self, states, c, seed, step, ids, rounds):
                r = self.e.alpha_mcts_parallel(states, c, seed, step, ids, rounds, ref_quirks=False)
                return r["probs"], r["n_children"]
        dev = e1.arena(diee_amd.AGENT_MODEL, e2, diee_amd.AGENT_MODEL, 96, cfg, 1.25, seed=7, round_limit=60, max_rounds=5, ref_quirks=False)
        ref = versus.play(P(MODEL, e1), P(MODEL, e2), cfg, 1.25, seed=7, num_games=96, round_limit=60, max_rounds=5,
                          search1=NoQuirks(e1), search2=NoQuirks(e2))
        assert dev["final_states"].tobytes() == ref.final_states.tobytes()
        # (PlayResult.draws = games - wins counts the games still alive; the call's own counter has retired draws only)
        assert (dev["wins_p1"], dev["wins_p2"], dev["draws"], dev["rounds"]) == (ref.wins_p1, ref.wins_p2, 0, 5) and len(ref.games) == 0
        assert dev["illegal_decodes"] == 0 and (dev["retired_round"] == 0xFFFFFFFF).all() and (dev["winner"] == 0).all()
        return
    if variant == "launch_per_iteration":
        for e in engines:
            e.set_options(free_eval=0, spec_eval=0)
    try:
        dev, _ = both(P(MODEL, e1), P(MODEL, e2), cfg, 7, 96, 60, max_rounds=5)
    finally:
        for e in engines:
            e.set_options(free_eval=1, spec_eval=1)
    assert dev.rounds == 5 and len(dev.games) == 0 and (dev.device["retired_round"] == 0xFFFFFFFF).all()


def test_case4_the_arenas_own_width(engines):
    e1, e2 = engines
    dev, _ = both(P(MODEL, e1), P(MODEL, e2), cfg_of(4), 11, 400, 400, max_rounds=3)
    assert dev.rounds == 3 and (dev.device["retired_round"] == 0xFFFFFFFF).all() and (dev.device["winner"] == 0).all()
    assert dev.device["stats"][0]["plies"] + dev.device["stats"][1]["plies"] == 3 * 400


def test_case5_one_engine_on_both_sides(engines):
    e1, _ = engines
    dev, _ = both(P(MODEL, e1), P(MODEL, e1), cfg_of(6), 13, 8, 400, max_rounds=4)
    assert dev.rounds == 4


@pytest.mark.parametrize("a1,a2", [(MODEL, RANDOM), (RANDOM, MODEL), (RANDOM, RANDOM)])
def test_case6_random_agents(engines, a1, a2):
    e1, e2 = engines
    p1 = P(a1, e1 if a1 == MODEL else None)
    p2 = P(a2, e2 if a2 == MODEL else None)
    dev, _ = both(p1, p2, cfg_of(6), 17, 12, 400, engine=e1 if a1 == a2 == RANDOM else None)
    assert dev.wins_p1 + dev.wins_p2 + dev.draws == 12 and len(dev.games) == 12


def test_case8_errors(engines):
    import diee_amd
    e1, e2 = engines
    cfg = cfg_of(4)
    M = diee_amd.AGENT_MODEL

    def status(*a, **kw):
        with pytest.raises(diee_amd.DieeError) as x:
            diee_amd.arena(*a, **kw)
        return x.value.status
    assert status(e1, M, e2, M, 0, cfg) == diee_amd.ERR_ARG
    assert status(e1, M, e2, M, 4, cfg, round_limit=0) == diee_amd.ERR_ARG
    assert status(e1, M, None, M, 4, cfg) == diee_amd.ERR_ARG                    # a Model agent without a ctx
    assert status(e1, 7, e2, M, 4, cfg) == diee_amd.ERR_ARG
    bare = diee_amd.Engine(0)
    assert status(e1, M, bare, M, 4, cfg) == diee_amd.ERR_NO_WEIGHTS
    assert status(bare, M, e1, M, 4, cfg) == diee_amd.ERR_NO_WEIGHTS
    r = diee_amd.arena(bare, diee_amd.AGENT_RANDOM, e2, M, 4, cfg, max_rounds=2)  # a ctx without weights hosts a Random agent
    assert r["rounds"] == 2
    bare.close()
    ttt = diee_amd.Engine(0, diee_amd.GAME_TTT)
    assert status(e1, M, ttt, M, 4, cfg) == diee_amd.ERR_UNSUPPORTED
    assert status(ttt, M, e1, M, 4, cfg) == diee_amd.ERR_UNSUPPORTED
    ttt.close()
    try:
        far = diee_amd.Engine(1)                                                 # a second GPU, where the box has one
    except diee_amd.DieeError:
        far = None
    if far is not None:
        far.load_weights(diee_amd.random_weights(1))
        assert status(e1, M, far, M, 4, cfg) == diee_amd.ERR_ARG
        far.close()
    # the engines still work after the refused calls
    assert diee_amd.arena(e1, M, e2, M, 4, cfg, max_rounds=1)["rounds"] == 1


CHILD = r"""
import importlib, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
az = importlib.import_module("die-e_amd.alphazero")
import diee_amd
assert os.environ.get("DIEE_ARENA") == "device"
out = []
for mode in ("device", "default"):
    if mode == "default":
        del os.environ["DIEE_ARENA"]
    root = os.path.join(sys.argv[2], mode)
    os.makedirs(os.path.join(root, "models", "backgammon"))
    np.save(os.path.join(root, "models", "backgammon", "best_model.npy"), diee_amd.random_weights(1))
    eng = diee_amd.Engine(0)
    conf = az.AlphaZeroConfig(temperature=1.25, learn_iterations=1, self_play_iterations=1, num_epochs=1, training_batch_size=16,
                              num_self_play_batches=4)
    a = az.AlphaZero(eng, conf, diee_amd.MctsConfig(iterations=6, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25),
                     az.OptimizerParams(1e-4, 1e-3), blob=diee_amd.random_weights(0), root=root, quiet=True)
    msgs = []
    a.log = lambda m, msgs=msgs: msgs.append(str(m))
    verdict = a.play_vs_best_model(n_games=4)
    out.append((verdict, [m for m in msgs if "Match result" in m]))
    eng.close()
print("VERDICTS", repr(out[0][0]), "|", repr(out[1][0]))
print("SAME", out[0] == out[1])
"""


def test_case9_diee_arena_device_in_a_child_process(tmp_path):
    """DIEE_ARENA=device switches play_vs_best_model to the device arena: one of the three verdicts, the default path's for the seed"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, DIEE_ARENA="device")
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    line = next(l for l in out.splitlines() if l.startswith("VERDICTS"))
    verdicts = ("new model was better!", "current best model is still better!",
                "new model vs current best was inconclusive, keeping current best!")
    assert any(f"{v!r} | {v!r}" in line for v in verdicts), out
    assert "SAME True" in out, out
