"""GPU tests of Agent::Mcts (diee_mcts_vanilla_batch / Engine.mct_search, DIEE_AGENT_MCTS in diee_arena): the engine's vanilla UCB1
search is the Python restatement (tests/vanilla_ref.py, on the oracle's game functions) bit for bit -- plays, the roots' children with
their visits and values, every counter --, whatever the launch budget and the batch; the device arena plays the host driver's games."""
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
MODEL, RANDOM, MCTS = versus.Agent.MODEL, versus.Agent.RANDOM, versus.Agent.MCTS
SEED = 77                 # case 1, quirks off: rollouts that reach a winner, finished games and dead ends inside the trees (asserted on the reference)
COUNTERS = ("iterations", "expansions", "terminal_hits", "dead_end_hits", "rollouts", "rollout_plies", "rollout_decided", "depth_sum")


def cfg_of(iterations, round_limit=30, c=2.0):
    import diee_amd
    return diee_amd.MctsConfig(iterations=iterations, c=c, round_limit=round_limit, dir_alpha=0.3, dir_eps=0.25)


def case_roots(orc):
    """16 roots: 8 late-game positions of random walks (rollouts reach a winner inside the limit), 3 positions whose successor in the
    walk had no legal play (a checker on the bar facing made points: dead ends inside the tree), the opening position, and one root
    each without a legal play, with exactly one, with a finished game; then a late position again"""
    walk = orc.random_walk_states(5, 40, 400)
    _, cnt = orc.valid_moves_batch(walk)
    late = walk[(walk["off"].max(axis=1) >= 12) & (cnt > 1)]
    roots = np.zeros(16, dtype=orc.BG_STATE)
    roots[:8] = late[:: max(1, len(late) // 8)][:8]
    before = np.nonzero((cnt[1:] == 0) & (cnt[:-1] > 1) & (walk["off"][:-1].max(axis=1) < 12))[0]
    roots[8:11] = walk[before[[0, len(before) // 2, -1]]]
    roots[11] = orc.bg_new(); roots[11]["roll"] = (6, 5)
    roots[12] = walk[cnt == 0][0]
    roots[13] = walk[cnt == 1][0]
    won = late[3].copy()                                       # side -1 has borne off everything
    won["pts"] = np.where(won["pts"] < 0, 0, won["pts"]); won["bar"][0] = 0; won["off"][0] = 15
    roots[14] = won
    roots[15] = late[-1]
    return roots


@pytest.fixture(scope="module")
def roots(oracle):
    return case_roots(oracle)


@pytest.fixture(scope="module")
def engine():
    import diee_amd
    e = diee_amd.Engine(0)                                      # no weights: the search needs none
    yield e
    e.close()


_REF = {}


def reference(roots, iterations, quirks, ids, rounds):
    """the restatement's answer for a case, computed once"""
    from vanilla_ref import mct_search_batch
    key = (iterations, quirks)
    if key not in _REF:
        _REF[key] = mct_search_batch(roots, iterations, 2.0, 30, SEED, ids, rounds, quirks)
    return _REF[key]


def assert_equal(out, ref):
    assert out["plays"].tobytes() == ref["plays"].tobytes()
    assert (out["n_children"] == ref["n_children"]).all()
    assert out["child_visits"].tobytes() == ref["child_visits"].tobytes()
    assert out["child_values"].tobytes() == ref["child_values"].tobytes()
    for k in COUNTERS:
        assert out["stats"][k] == ref["stats"][k], k


IDS = np.arange(16, dtype=np.uint32) * 3 + 1
ROUNDS = (np.arange(16, dtype=np.uint32) * 5) % 7


@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("iterations", [40, 5, 0])
def test_case1_parity_with_the_restatement(engine, roots, oracle, iterations, quirks):
    ref = reference(roots, iterations, quirks, IDS, ROUNDS)
    st = ref["stats"]
    if iterations == 40 and not quirks:                         # the branches this case is about were taken, by the reference alone
        assert st["rollout_decided"] > 0 and st["dead_end_hits"] > 0 and st["terminal_hits"] > 0 and st["rollout_plies"] > 0
    if iterations == 5:                                         # fewer iterations than plays: a root that is never fully expanded
        _, cnt = oracle.valid_moves_batch(roots)
        assert (cnt > 5).any() and (ref["n_children"] <= 5).all()
    out = engine.mct_search(roots, cfg_of(iterations), SEED, IDS, ROUNDS, ref_quirks=quirks)
    assert_equal(out, ref)
    # roots 12 (no legal play) and 14 (finished game) answer EMPTY_MOVE with no iterations; root 13 has its one play
    assert (out["plays"][[12, 14]] == -2).all() and (out["n_children"][[12, 14]] == 0).all()
    if iterations:
        assert out["n_children"][13] == 1 and out["child_visits"][13, 0] == iterations
        assert st["iterations"] == 14 * iterations
    else:
        assert (out["plays"] == -2).all() and st["iterations"] == 0


@pytest.mark.parametrize("quirks", [True, False])
def test_case2_launch_budget(engine, roots, quirks):
    """the trees persist in HBM between launches: 1, 7 and the derived number of iterations per launch give the same output"""
    cfg = cfg_of(40)
    outs = []
    try:
        for budget in (1, 7, 0):
            engine.set_option("vanilla_iters_per_launch", budget)
            outs.append(engine.mct_search(roots, cfg, SEED, IDS, ROUNDS, ref_quirks=quirks))
    finally:
        engine.set_option("vanilla_iters_per_launch", 0)
    for o in outs[:2]:
        assert_equal(o, outs[2])
    assert outs[2]["stats"]["iterations"] == 14 * 40


def test_case2_batch_independence(engine, oracle):
    """300 roots in one call equal the same roots searched 1, 16 and 283 at a time (each root keeps its game id and round)"""
    walk = oracle.random_walk_states(9, 6, 400)
    states = walk[np.linspace(0, len(walk) - 1, 300).astype(int)]
    ids = np.arange(300, dtype=np.uint32) + 1000
    rounds = (np.arange(300, dtype=np.uint32) * 7) % 11
    cfg = cfg_of(12, round_limit=10)
    whole = engine.mct_search(states, cfg, 5, ids, rounds, ref_quirks=False)
    assert whole["stats"]["iterations"] > 0 and whole["stats"]["rollout_plies"] > 0
    for lo, hi in ((0, 1), (1, 17), (17, 300)):
        part = engine.mct_search(states[lo:hi], cfg, 5, ids[lo:hi], rounds[lo:hi], ref_quirks=False)
        for k in ("plays", "n_children", "child_visits", "child_values"):
            assert part[k].tobytes() == whole[k][lo:hi].tobytes(), (k, lo, hi)


def games_of(res):
    return [(g.initial_state["id"], g.winner) for g in res.games]


def assert_same_games(dev, ref):
    assert dev.final_states.tobytes() == ref.final_states.tobytes()
    assert (dev.wins_p1, dev.wins_p2, dev.draws, dev.rounds) == (ref.wins_p1, ref.wins_p2, ref.draws, ref.rounds)
    assert games_of(dev) == games_of(ref)
    assert dev.device["illegal_decodes"] == 0


@pytest.mark.parametrize("a1,a2", [(MCTS, RANDOM), (RANDOM, MCTS)])
def test_case3_arena_mcts_and_random(engine, a1, a2):
    """versus.play (the host driver over diee_mcts_vanilla_batch) and versus.play_device (diee_arena): the same PlayResult"""
    cfg = cfg_of(12, round_limit=20)
    p1, p2 = P(a1, engine if a1 == MCTS else None), P(a2, engine if a2 == MCTS else None)
    dev = versus.play_device(p1, p2, cfg, 1.25, seed=23, num_games=8, round_limit=400, vanilla_rollouts=True)
    ref = versus.play(p1, p2, cfg, 1.25, seed=23, num_games=8, round_limit=400, vanilla_rollouts=True)
    assert_same_games(dev, ref)
    assert dev.wins_p1 + dev.wins_p2 + dev.draws == 8 and len(dev.games) == 8
    st = dev.device["stats"][0 if a1 == MCTS else 1]
    assert st["selections"] > 0 and st["expansions"] > 0 and st["move_steps"] > 0 and st["nn_evals"] == 0 and st["plies"] >= st["fragments"] > 0
    assert dev.device["stats"][1 if a1 == MCTS else 0]["selections"] == 0


def test_case3_arena_mcts_and_model(engine):
    import diee_amd
    e2 = diee_amd.Engine(0); e2.load_weights(diee_amd.random_weights(1))
    try:
        cfg = cfg_of(6, round_limit=20)
        p1, p2 = P(MCTS, engine), P(MODEL, e2)
        dev = versus.play_device(p1, p2, cfg, 1.25, seed=29, num_games=6, round_limit=400, max_rounds=6)
        ref = versus.play(p1, p2, cfg, 1.25, seed=29, num_games=6, round_limit=400, max_rounds=6)
        assert_same_games(dev, ref)
        assert dev.rounds == 6
        st = dev.device["stats"]
        assert st[0]["selections"] > 0 and st[0]["nn_evals"] == 0 and st[1]["nn_evals"] > 0
    finally:
        e2.close()


def test_case4_errors(engine, roots):
    import diee_amd

    def status(e, cfg):
        with pytest.raises(diee_amd.DieeError) as x:
            e.mct_search(roots[:2], cfg, 1)
        return x.value.status
    assert status(engine, cfg_of(1 << 20)) == diee_amd.ERR_ARG
    assert status(engine, cfg_of(4, round_limit=4095)) == diee_amd.ERR_ARG
    ttt = diee_amd.Engine(0, diee_amd.GAME_TTT)
    assert status(ttt, cfg_of(4)) == diee_amd.ERR_UNSUPPORTED
    ttt.close()
    with pytest.raises(diee_amd.DieeError) as x:                # an arena with an Mcts player checks the same bounds
        diee_amd.arena(engine, diee_amd.AGENT_MCTS, None, diee_amd.AGENT_RANDOM, 2, cfg_of(4, round_limit=4095))
    assert x.value.status == diee_amd.ERR_ARG
    # a ctx without weights serves the call (round_limit = 4094 is the largest allowed); with weights it still searches with the network
    out = engine.mct_search(roots[:4], cfg_of(3, round_limit=4094), 1)
    assert out["stats"]["iterations"] == 12
    with pytest.raises(diee_amd.DieeError) as x:
        engine.alpha_mcts_parallel(roots[:2], cfg_of(2))
    assert x.value.status == diee_amd.ERR_NO_WEIGHTS
    engine.load_weights(diee_amd.random_weights(0))
    r = engine.alpha_mcts_parallel(roots[:2], cfg_of(4))
    assert (r["n_children"] > 0).all()
    assert engine.mct_search(roots[:4], cfg_of(3, round_limit=4094), 1)["plays"].tobytes() == out["plays"].tobytes()


def test_case5_cli_in_a_child_process(tmp_path):
    """`diee.py play -a mcts --agent-two random -o DIR` (the one command of the reference's CLI the project used to refuse)"""
    cfg = tmp_path / "tiny.toml"
    cfg.write_text("temperature = 1.25\nlearn_iterations = 1\nnum_epochs = 1\ntraining_batch_size = 16\nself_play_iterations = 1\n"
                   "num_self_play_batches = 4\niterations = 3\nexploration_const = 2.0\nsimulate_round_limit = 8\n"
                   "dirichlet_alpha = 0.3\ndirichlet_epsilon = 0.25\nwd = 0.0001\nlr = 0.001\n")
    games = tmp_path / "games"; games.mkdir()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "diee.py"), "-c", str(cfg), "-g", "backgammon", "play", "-a", "mcts",
                        "--agent-two", "random", "-o", str(games)], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "Player 1: Mcts" in out and "Saving games" in out
    assert len(list(games.iterdir())) == 400                    # versus.rs:160: 400 games
