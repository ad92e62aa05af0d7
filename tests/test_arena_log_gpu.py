"""GPU tests of the arena's turn log (diee_arena_ex / Engine.arena(record_turns=True) / versus.play_device(record_turns=True)) and of
the flag word per player: the device's log is, game by game and field by field, what versus.play records -- the Python driver, an
independent statement of the rule, on the engine and on the oracle -- and every recorded game replays to its final state."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

versus = importlib.import_module("die-e_amd.versus")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = versus.Player
MODEL, RANDOM, MCTS = versus.Agent.MODEL, versus.Agent.RANDOM, versus.Agent.MCTS
SEED_SKIPS = 21           # the seed of tests/test_arena_gpu.py whose 8 games contain skipped turns
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def engines():
    import diee_amd
    e1 = diee_amd.Engine(0); e1.load_weights(diee_amd.random_weights(0))
    e2 = diee_amd.Engine(0); e2.load_weights(diee_amd.random_weights(1))
    yield e1, e2
    e1.close(); e2.close()


def cfg_of(iterations, round_limit=400):
    import diee_amd
    return diee_amd.MctsConfig(iterations=iterations, c=2.0, round_limit=round_limit, dir_alpha=0.3, dir_eps=0.25)


def games_of(res):
    return [(g.initial_state["id"], g.winner) for g in res.games]


def assert_same(dev, ref):
    """tests/test_arena_gpu.py's comparison, plus the turns of every game index and of every Game"""
    assert dev.final_states.tobytes() == ref.final_states.tobytes()
    assert (dev.wins_p1, dev.wins_p2, dev.draws, dev.rounds) == (ref.wins_p1, ref.wins_p2, ref.draws, ref.rounds)
    assert games_of(dev) == games_of(ref)
    assert dev.device["illegal_decodes"] == 0
    assert len(dev.turns) == len(ref.turns) == dev.n_games
    for g, (a, b) in enumerate(zip(dev.turns, ref.turns)):
        assert len(a) == len(b), (g, len(a), len(b))
        for t, (x, y) in enumerate(zip(a, b)):
            assert x == y, (g, t, x, y)
    assert [g.turns for g in dev.games] == [g.turns for g in ref.games]


def check_log(dev, kinds=None):
    """what the log must satisfy on its own: first[] against retired_round, one `retired` record per retired game and on its last turn,
    the skipped records against the stats, player / agent / second against the rules of the arena"""
    import diee_amd
    r = dev.device
    rec, first, rr = r["turns"], r["first"], r["retired_round"]
    n = dev.n_games
    assert first[0] == 0 and first[n] == len(rec)
    lens = np.diff(first.astype(np.int64))
    want = np.where(rr == NONE, r["rounds"], rr.astype(np.int64) + 1)
    assert (lens == want).all()
    for g in range(n):
        t = rec[int(first[g]):int(first[g + 1])]
        assert int(t["retired"].sum()) == (0 if rr[g] == NONE else 1)
        if rr[g] != NONE:
            assert t["retired"][-1] == 1 and t["play"][-1][0] != diee_amd.NO_MOVE          # a skipped turn retires nothing
        assert (t["roll"][0] == r["initial_states"]["roll"][g]).all() and t["player"][0] == r["initial_states"]["player"][g]
    assert set(np.unique(rec["player"])) <= {-1, 1} and set(np.unique(rec["second"])) <= {0, 1}
    skipped = int((rec["play"][:, 0] == diee_amd.NO_MOVE).sum())
    assert skipped == sum(s["plies"] - s["fragments"] for s in r["stats"])
    assert len(rec) == sum(s["plies"] for s in r["stats"])
    if kinds is not None:
        assert (rec["agent"][rec["player"] == -1] == kinds[0]).all() and (rec["agent"][rec["player"] == 1] == kinds[1]).all()
    return skipped


def replays_reach_final_states(dev, rules, only_live=False):
    n = dev.n_games
    docs = [{"id": f"g{g}", "player1": dev.player1, "player2": dev.player2, "turns": dev.turns[g],
             "initial_state": versus.Game(dev.player1, dev.player2, dev.device["initial_states"][g], g).initial_state} for g in range(n)]
    states = versus.replay_all(docs, rules)
    for g in range(n):
        assert len(states[g]) == len(dev.turns[g])
        assert states[g][-1].tobytes() == dev.final_states[g].tobytes(), g


_case1 = {}


@pytest.fixture
def case1(engines, oracle):
    """Model vs Model, 8 games, 6 iterations, seed 21, to completion: the device call (default chunking), the Python driver on the
    engine, the Python driver on the oracle's rules and search -- each run once"""
    if not _case1:
        from oracle.arena_backend import OracleRules, OracleSearch
        e1, e2 = engines
        cfg = cfg_of(6)
        p1, p2 = P(MODEL, e1), P(MODEL, e2)
        _case1["dev"] = versus.play_device(p1, p2, cfg, 1.25, seed=SEED_SKIPS, num_games=8, round_limit=400, record_turns=True)
        _case1["ref"] = versus.play(p1, p2, cfg, 1.25, seed=SEED_SKIPS, num_games=8, round_limit=400, record_turns=True)

        def ev(e):
            return oracle.make_eval(lambda s: e.forward_t(s.view(oracle.BG_STATE).reshape(-1)), 1352)
        _case1["orc"] = versus.play(P(MODEL), P(MODEL), cfg, 1.25, seed=SEED_SKIPS, num_games=8, round_limit=400, rules=OracleRules(),
                                    search1=OracleSearch(ev(e1)), search2=OracleSearch(ev(e2)), record_turns=True)
    return _case1


def test_eight_games_the_log_is_the_drivers_and_the_oracles(engines, case1):
    import diee_amd
    e1, _ = engines
    dev = case1["dev"]
    assert_same(dev, case1["ref"])
    assert_same(dev, case1["orc"])
    assert len(dev.games) == 8 and dev.wins_p1 + dev.wins_p2 > 0
    assert check_log(dev, (diee_amd.AGENT_MODEL, diee_amd.AGENT_MODEL)) > 0                # the seed's skipped turns are in the log
    assert all(t["player"] == MODEL for g in dev.turns for t in g)
    replays_reach_final_states(dev, versus.EngineRules(e1))


def test_eight_games_in_chunks_of_four_rounds(engines, case1):
    """arena_log_rounds = 4: the call crosses many chunk boundaries; the log does not depend on it"""
    e1, e2 = engines
    assert e1.get_option("arena_log_rounds") == "64" and e1.get_option("arena_log_mb") == "1024"
    e1.set_option("arena_log_rounds", 4)
    try:
        dev4 = versus.play_device(P(MODEL, e1), P(MODEL, e2), cfg_of(6), 1.25, seed=SEED_SKIPS, num_games=8, round_limit=400, record_turns=True)
    finally:
        e1.set_option("arena_log_rounds", 64)
    assert dev4.rounds > 3 * 4
    assert_same(dev4, case1["ref"])
    assert dev4.device["turns"].tobytes() == case1["dev"].device["turns"].tobytes()
    assert (dev4.device["first"] == case1["dev"].device["first"]).all()
    check_log(dev4)
    # without a log the same call returns the same games (the log changes nothing it does not own)
    plain = versus.play_device(P(MODEL, e1), P(MODEL, e2), cfg_of(6), 1.25, seed=SEED_SKIPS, num_games=8, round_limit=400)
    assert plain.turns is None and all(g.turns == [] for g in plain.games) and "turns" not in plain.device
    assert plain.final_states.tobytes() == dev4.final_states.tobytes() and games_of(plain) == games_of(dev4)


def test_96_games_past_the_round_limit(engines):
    """tests/test_arena_gpu.py case 2 with the log: fused, cluster and k_tail sizes; the games that skip the turn of round 59 play past the
    limit (so no [games][round_limit] array could hold the log); the draws carry `retired` on their last record"""
    e1, e2 = engines
    cfg = cfg_of(8)
    p1, p2 = P(MODEL, e1), P(MODEL, e2)
    e1.set_option("arena_log_rounds", 4)
    try:
        dev = versus.play_device(p1, p2, cfg, 1.25, seed=SEED_SKIPS, num_games=96, round_limit=60, record_turns=True)
    finally:
        e1.set_option("arena_log_rounds", 64)
    ref = versus.play(p1, p2, cfg, 1.25, seed=SEED_SKIPS, num_games=96, round_limit=60, record_turns=True)
    assert_same(dev, ref)
    check_log(dev)
    r = dev.device
    assert dev.rounds > 60 and int((np.diff(r["first"].astype(np.int64)) > 60).sum()) > 0  # games longer than round_limit turns
    st = r["stats"]
    assert st[0]["band_launches"][2] + st[1]["band_launches"][2] > 0 and st[0]["band_launches"][0] + st[1]["band_launches"][0] > 0
    draws = np.nonzero((r["winner"] == 0) & (r["retired_round"] != NONE))[0]
    assert len(draws) == dev.draws > 0
    for g in draws:
        assert r["turns"][int(r["first"][g + 1]) - 1]["retired"] == 1 and r["retired_round"][g] >= 59


def test_max_rounds_stops_live_games(engines):
    """max_rounds = 5: every game has 5 turns, none retired, and the replays reach the live games' final states"""
    e1, e2 = engines
    p1, p2 = P(MODEL, e1), P(MODEL, e2)
    dev = versus.play_device(p1, p2, cfg_of(6), 1.25, seed=7, num_games=12, round_limit=60, max_rounds=5, record_turns=True)
    ref = versus.play(p1, p2, cfg_of(6), 1.25, seed=7, num_games=12, round_limit=60, max_rounds=5, record_turns=True)
    assert_same(dev, ref)
    check_log(dev)
    assert dev.rounds == 5 and len(dev.games) == 0 and (dev.device["retired_round"] == NONE).all()
    assert all(len(t) == 5 for t in dev.turns) and int(dev.device["turns"]["retired"].sum()) == 0
    replays_reach_final_states(dev, versus.EngineRules(e1))


@pytest.mark.parametrize("a1,a2", [(RANDOM, RANDOM), (MCTS, RANDOM)])
def test_random_and_mcts_agents_hosted_by_engine(engines, a1, a2):
    import diee_amd
    e1, _ = engines
    kinds = {RANDOM: diee_amd.AGENT_RANDOM, MCTS: diee_amd.AGENT_MCTS}
    cfg = cfg_of(8)
    dev = versus.play_device(P(a1), P(a2), cfg, 1.25, seed=17, num_games=6, round_limit=400, engine=e1, record_turns=True)
    srch = versus.EngineSearch(e1)
    ref = versus.play(P(a1), P(a2), cfg, 1.25, seed=17, num_games=6, round_limit=400, rules=versus.EngineRules(e1), search1=srch,
                      search2=srch, record_turns=True)
    assert_same(dev, ref)
    check_log(dev, (kinds[a1], kinds[a2]))
    assert len(dev.games) == 6
    assert {t["player"] for g in dev.turns for t in g} == {a1, a2}
    replays_reach_final_states(dev, versus.EngineRules(e1))               # (a skipped turn of these agents had no legal play: replay_all checks it)


def test_mcts_with_played_rollouts_against_a_model_runs_on_the_device(engines):
    """a flag word per player: quirks off for the Mcts side (its rollouts are played), on for the Model side, as play() searches them.
    On the parent commit play_device raised ValueError for this pairing"""
    e1, e2 = engines
    cfg = cfg_of(4, round_limit=40)
    p1, p2 = P(MCTS, e1), P(MODEL, e2)
    dev = versus.play_device(p1, p2, cfg, 1.25, seed=5, num_games=6, round_limit=400, vanilla_rollouts=True, record_turns=True)
    ref = versus.play(p1, p2, cfg, 1.25, seed=5, num_games=6, round_limit=400, vanilla_rollouts=True, record_turns=True)
    assert_same(dev, ref)
    assert len(dev.games) == 6
    check_log(dev)
    # the rollouts were played: the same call with the quirks on both sides is another set of games
    quirky = versus.play_device(p1, p2, cfg, 1.25, seed=5, num_games=6, round_limit=400, vanilla_rollouts=False, record_turns=True)
    assert quirky.turns != dev.turns
    # the other way round (flags[0] is the Model's word, flags[1] the Mcts agent's), a few rounds
    p1, p2 = P(MODEL, e2), P(MCTS, e1)
    dev = versus.play_device(p1, p2, cfg, 1.25, seed=6, num_games=6, round_limit=400, max_rounds=6, vanilla_rollouts=True, record_turns=True)
    ref = versus.play(p1, p2, cfg, 1.25, seed=6, num_games=6, round_limit=400, max_rounds=6, vanilla_rollouts=True, record_turns=True)
    assert_same(dev, ref)


def test_flag_words(engines):
    """flags = {f, f} without a log gives the bytes of diee_arena; {quirks, none} is a driver whose second player searches without them"""
    import diee_amd
    e1, e2 = engines
    M = diee_amd.AGENT_MODEL
    cfg = cfg_of(8)
    keys = ("winner", "retired_round", "retired_side", "initial_states", "final_states")
    outs = {}
    for quirks in (True, False):
        f = diee_amd.FLAG_REF_QUIRKS if quirks else 0
        a = diee_amd.arena(e1, M, e2, M, 12, cfg, 1.25, seed=7, round_limit=60, max_rounds=5, ref_quirks=quirks)
        b = diee_amd.arena(e1, M, e2, M, 12, cfg, 1.25, seed=7, round_limit=60, max_rounds=5, ref_quirks=quirks, flags2=f)
        assert "turns" not in a and "turns" not in b
        for k in keys:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert all(a[k] == b[k] for k in ("wins_p1", "wins_p2", "draws", "rounds", "illegal_decodes"))
        search = ("games", "plies", "fragments", "move_steps", "nn_evals", "expansions", "children", "selections", "depth_sum")
        assert [[s[k] for k in search] for s in a["stats"]] == [[s[k] for k in search] for s in b["stats"]]     # (what a search computes, not how it was scheduled)
        outs[quirks] = a

    class NoQuirks(versus.EngineSearch):
        def mcts(self, states, c, seed, step, ids, rounds):
            r = self.e.alpha_mcts_parallel(states, c, seed, step, ids, rounds, ref_quirks=False)
            return r["probs"], r["n_children"]
    mixed = diee_amd.arena(e1, M, e2, M, 12, cfg, 1.25, seed=7, round_limit=60, max_rounds=5, ref_quirks=True, flags2=0)
    ref = versus.play(P(MODEL, e1), P(MODEL, e2), cfg, 1.25, seed=7, num_games=12, round_limit=60, max_rounds=5,
                      search1=versus.EngineSearch(e1), search2=NoQuirks(e2))
    assert mixed["final_states"].tobytes() == ref.final_states.tobytes()


def test_errors_and_the_capacity_bound(engines):
    import diee_amd
    e1, e2 = engines
    L = diee_amd.load_library()
    M, R = diee_amd.AGENT_MODEL, diee_amd.AGENT_RANDOM
    cfg = cfg_of(1)
    log = diee_amd.ArenaLog()
    res = diee_amd.ArenaResult()

    def ex(ctx1, a1, ctx2, a2, n, opts):
        return L.diee_arena_ex(ctx1, a1, ctx2, a2, n, C.byref(cfg), 1.25, 3, 400, 2, opts, C.byref(res), None, None, None, None, None, None)
    good = diee_amd.ArenaOpts(C.sizeof(diee_amd.ArenaOpts), (C.c_uint32 * 2)(1, 1), C.pointer(log))
    bad = diee_amd.ArenaOpts(C.sizeof(diee_amd.ArenaOpts) - 4, (C.c_uint32 * 2)(1, 1), None)
    assert ex(e1._h, R, None, R, 4, C.byref(bad)) == diee_amd.ERR_ARG and b"struct_size" in L.diee_last_error(e1._h)
    assert ex(e1._h, R, None, R, 4, None) == diee_amd.ERR_ARG
    ttt = diee_amd.Engine(0, diee_amd.GAME_TTT)
    assert ex(ttt._h, R, None, R, 4, C.byref(good)) == diee_amd.ERR_UNSUPPORTED
    ttt.close()
    # a call with every per-game output NULL still logs (the log needs retired_round on its own)
    assert ex(e1._h, R, None, R, 4, C.byref(good)) == diee_amd.OK
    assert log.n_games == 4 and log.first[4] == 8 and res.rounds == 2
    L.diee_free_arena_log(C.byref(log))
    assert not log.turns and not log.first and not log.owner
    # arena_log_mb too small: 20000 games x 12 bytes = 240 KB per round, 1 MiB holds a chunk of 3 rounds and a second one cut short to the
    # one round that still fits -- round 4 is not played: DIEE_ERR_CAPACITY, no truncated log
    # (a ctx of its own: the module's engines keep their slot space small)
    big = diee_amd.Engine(0)
    big.set_options(arena_log_mb=1, arena_log_rounds=3)
    try:
        with pytest.raises(diee_amd.DieeError) as x:
            diee_amd.arena(big, R, None, R, 20000, cfg, 1.25, seed=3, round_limit=400, record_turns=True)
        assert x.value.status == diee_amd.ERR_CAPACITY and "arena_log_mb" in str(x.value) and "round 4" in str(x.value)
        few = diee_amd.arena(big, R, None, R, 20000, cfg, 1.25, seed=3, round_limit=400, max_rounds=4, record_turns=True)     # 4 rounds fit
        assert few["rounds"] == 4 and len(few["turns"]) == 4 * 20000
        big.set_option("arena_log_mb", 0)
        with pytest.raises(diee_amd.DieeError) as x:
            diee_amd.arena(big, R, None, R, 4, cfg, 1.25, seed=3, record_turns=True)
        assert x.value.status == diee_amd.ERR_CAPACITY
        assert diee_amd.arena(big, R, None, R, 4, cfg, 1.25, seed=3, max_rounds=2)["rounds"] == 2    # the bound is the log's alone
        # the ctx serves the next call
        big.set_option("arena_log_mb", 1024)
        r = diee_amd.arena(big, R, None, R, 4, cfg, 1.25, seed=3, max_rounds=2, record_turns=True)
        assert r["rounds"] == 2 and len(r["turns"]) == 8 and (r["first"] == [0, 2, 4, 6, 8]).all()
    finally:
        big.close()
    r = diee_amd.arena(e1, M, e2, M, 4, cfg_of(4), 1.25, seed=3, max_rounds=2, record_turns=True)
    assert r["rounds"] == 2 and len(r["turns"]) == 8 and (r["turns"]["agent"] == M).all()


def test_cpp_host_records_and_replays_through_the_c_abi(tmp_path):
    """examples/arena_replay.cpp (g++, include/diee.hpp over include/diee.h): 8 Random-vs-Random games with a log, every game replayed
    with diee_bg_legal_moves / diee_bg_apply; exit 0 only if all 32-byte final states match"""
    exe = str(tmp_path / "arena_replay")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "arena_replay.cpp"), "-L", os.path.join(ROOT, "die-e_amd"), "-ldiee",
                           "-Wl,-rpath," + os.path.join(ROOT, "die-e_amd"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out + p.stderr.decode()
    assert "arena_replay: 8 games" in out and "8 replays reach the final state" in out
