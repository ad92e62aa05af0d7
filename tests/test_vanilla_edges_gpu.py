"""GPU tests of the paths of Agent::Mcts that the 16-root, 40-iteration case of tests/test_vanilla_gpu.py never takes: nodes with more
children than a wavefront has lanes (vanilla_level's later passes), scores that are NaN (the restart behind the last NaN), a result
kernel that writes fewer columns than the root has children, rollouts of zero, one and two plies, searches of thousands of iterations
followed by smaller ones on the retained slabs, and the device arena against the restatement instead of against the engine's own
search.  Every comparison is bit for bit with tests/vanilla_ref.py (plays, the roots' children with their visits and values, every
counter); the roots and what the restatement alone must do on them are in tests/vanilla_cases.py."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

versus = importlib.import_module("die-e_amd.versus")
P = versus.Player
RANDOM, MCTS = versus.Agent.RANDOM, versus.Agent.MCTS
ARRAYS = ("plays", "n_children", "child_visits", "child_values")


def cfg_of(iterations, round_limit=30, c=2.0):
    import diee_amd
    return diee_amd.MctsConfig(iterations=iterations, c=c, round_limit=round_limit, dir_alpha=0.3, dir_eps=0.25)


@pytest.fixture(scope="module")
def vc(oracle):
    import vanilla_cases
    return vanilla_cases


@pytest.fixture(scope="module")
def engine():
    import diee_amd
    e = diee_amd.Engine(0)                                      # no weights: the search needs none
    yield e
    e.close()


def assert_equal(out, ref):
    assert out["plays"].tobytes() == ref["plays"].tobytes()
    assert (out["n_children"] == ref["n_children"]).all()
    assert out["child_visits"].tobytes() == ref["child_visits"].tobytes()
    assert out["child_values"].tobytes() == ref["child_values"].tobytes()
    from vanilla_ref import COUNTERS
    for k in COUNTERS:
        assert out["stats"][k] == ref["stats"][k], k


def search(engine, vc, roots, iterations, c, round_limit, quirks, cap=256):
    ids, rounds = vc.keys_of(len(roots))
    return engine.mct_search(roots, cfg_of(iterations, round_limit, c), vc.SEED, ids, rounds, ref_quirks=quirks, cap=cap)


# ---- 1: wide nodes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirks", [True, False])
def test_case1_wide_nodes(engine, vc, quirks):
    """roots of 63 ... 157 plays, 230 iterations: once a root is fully expanded every iteration selects among all its children, one,
    two and three passes of 64 links; with 7 iterations per launch the selection runs in launches other than the one that built the node"""
    beyond = vc.check_wide(quirks)
    ref = vc.wide_reference(quirks)
    print(vc.line(f"wide roots, quirks {'on' if quirks else 'off'}, {beyond} descents beyond depth 1", ref["stats"]))
    roots = vc.wide_roots()
    assert_equal(search(engine, vc, roots, quirks=quirks, **vc.WIDE), ref)
    try:
        engine.set_option("vanilla_iters_per_launch", 7)
        assert_equal(search(engine, vc, roots, quirks=quirks, **vc.WIDE), ref)
    finally:
        engine.set_option("vanilla_iters_per_launch", 0)


# ---- 2: fewer columns than children --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 1])
def test_case2_small_cap(engine, vc, cap):
    ref = vc.wide_reference(False)
    assert (ref["n_children"] > cap).all()
    print(vc.line(f"wide roots, cap {cap}", ref["stats"]))
    out = search(engine, vc, vc.wide_roots(), quirks=False, cap=cap, **vc.WIDE)
    assert out["child_visits"].shape == (6, cap)
    assert out["plays"].tobytes() == ref["plays"].tobytes() and (out["n_children"] == ref["n_children"]).all()
    assert out["child_visits"].tobytes() == np.ascontiguousarray(ref["child_visits"][:, :cap]).tobytes()
    assert out["child_values"].tobytes() == np.ascontiguousarray(ref["child_values"][:, :cap]).tobytes()
    for k, v in ref["stats"].items():
        assert out["stats"][k] == v, k


# ---- 3: exploration constants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [-1.0, 0.0, 0.5, float("inf"), float("nan")], ids=lambda c: f"c={c}")
def test_case3_exploration_constants(engine, vc, c):
    """c < 0: sqrt of a negative number, every score NaN but below a parent of one visit; c = inf: inf * ln 1 = NaN there and +inf
    everywhere else; c = NaN: every score NaN.  max_by's partial_cmp(..).unwrap_or(Equal) (simple_mcts.rs:46-51) restarts the fold
    behind the last NaN; c = 0 is pure exploitation and goes deep.
    What these cases can and cannot tell: under c < 0 a node's children all have one visit when it is first selected through, all
    their scores are NaN, the last created child is chosen, and by induction it is the only one ever chosen -- whatever its own score
    later is, it is the last of the fold.  So NaN and other scores do meet in one node (a tiny negative c: c * ln / v rounds to -0 for
    the much-visited last child), but never so that a choice among the children *behind* the last NaN differs from the last child: a
    kernel that takes the NaN path at all is told from one that does not (c = -1, inf, NaN all walk the last-created chain, c = 0
    does not), the order inside the restart cannot be told by any c"""
    if c in (-1.0, 0.0):
        vc.check_consts()
    ref = vc.const_reference(c)
    print(vc.line(f"small and race roots, c = {c}", ref["stats"]))
    out = search(engine, vc, vc.const_roots(), c=c, quirks=False, **vc.CONSTS)
    # a non-finite c is served like any other (include/diee.h): the call runs every iteration and answers what the reference's fold would
    assert out["stats"]["iterations"] == 5 * vc.CONSTS["iterations"]
    assert_equal(out, ref)


# ---- 4: rollout limits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("round_limit", [0, 1, 2])
def test_case4_rollout_limits(engine, vc, round_limit, quirks):
    vc.check_limits()
    ref = vc.limit_reference(round_limit, quirks)
    print(vc.line(f"small roots, round_limit {round_limit}, quirks {'on' if quirks else 'off'}", ref["stats"]))
    assert_equal(search(engine, vc, vc.small_roots(), round_limit=round_limit, quirks=quirks, **vc.LIMITS), ref)


# ---- 5: long searches and slab reuse -------------------------------------------------------------------------------------------------
def test_case5_long_searches_then_smaller_ones_on_the_retained_slabs(vc, oracle):
    """one fresh engine, in this order: 5000 iterations (the ln table and node_cap grow, selection hundreds of levels deep), 1500 with
    played rollouts, then the 16 roots of test_vanilla_gpu at 40 iterations on slabs whose node_cap stays 5001, 300 roots (slot_cap grows,
    node_cap stays), and the 16 roots again"""
    import diee_amd
    from test_vanilla_gpu import IDS, ROUNDS, SEED, case_roots, reference
    from vanilla_ref import mct_search_batch
    root = vc.long_root()
    e = diee_amd.Engine(0)
    try:
        ref = vc.reference("L", root, 5000, 2.0, 30, True)                       # (a)
        print(vc.line("late[0], 5000 iterations, quirks on", ref["stats"]))
        assert ref["stats"]["depth_sum"] > 2 * 5000 and ref["stats"]["terminal_hits"] > 0      # most descents go on below the root's children
        assert_equal(search(e, vc, root, 5000, 2.0, 30, True), ref)
        ref = vc.reference("L", root, 1500, 2.0, 30, False)                      # (b)
        print(vc.line("late[0], 1500 iterations, quirks off", ref["stats"]))
        assert_equal(search(e, vc, root, 1500, 2.0, 30, False), ref)
        roots16 = case_roots(oracle)                                             # (c)
        ref16 = reference(roots16, 40, False, IDS, ROUNDS)
        print(vc.line("16 roots, 40 iterations, quirks off, node_cap 5001", ref16["stats"]))
        first = e.mct_search(roots16, cfg_of(40), SEED, IDS, ROUNDS, ref_quirks=False)
        assert_equal(first, ref16)
        walk = oracle.random_walk_states(9, 6, 400)                              # (d)
        states = walk[np.linspace(0, len(walk) - 1, 300).astype(int)]
        ids = np.arange(300, dtype=np.uint32) + 1000
        rounds = (np.arange(300, dtype=np.uint32) * 7) % 11
        cfg = cfg_of(12, round_limit=10)
        whole = e.mct_search(states, cfg, 5, ids, rounds, ref_quirks=False)
        pick = np.linspace(0, 299, 20).astype(int)
        ref20 = mct_search_batch(states[pick], 12, 2.0, 10, 5, ids[pick], rounds[pick], False)
        print(vc.line("20 of 300 roots, 12 iterations, quirks off", ref20["stats"]))
        assert ref20["stats"]["iterations"] > 0 and ref20["stats"]["rollout_plies"] > 0
        for k in ARRAYS:
            assert whole[k][pick].tobytes() == ref20[k].tobytes(), k
        fresh = diee_amd.Engine(0)
        try:
            other = fresh.mct_search(states, cfg, 5, ids, rounds, ref_quirks=False)
        finally:
            fresh.close()
        assert_equal(whole, other)
        again = e.mct_search(roots16, cfg_of(40), SEED, IDS, ROUNDS, ref_quirks=False)      # (e)
        assert_equal(again, ref16)
        assert_equal(again, first)
    finally:
        e.close()


# ---- 6: the arena against the restatement --------------------------------------------------------------------------------------------
def games_of(res):
    return [(g.initial_state["id"], g.winner) for g in res.games]


def assert_same_games(dev, ref):
    assert dev.final_states.tobytes() == ref.final_states.tobytes()
    assert (dev.wins_p1, dev.wins_p2, dev.draws, dev.rounds) == (ref.wins_p1, ref.wins_p2, ref.draws, ref.rounds)
    assert games_of(dev) == games_of(ref)
    assert dev.device["illegal_decodes"] == 0


@pytest.mark.parametrize("a1,a2", [(MCTS, MCTS), (MCTS, RANDOM), (RANDOM, MCTS)])
def test_case6_arena_against_the_restatement(engine, vc, a1, a2):
    """diee_arena's games are those of the host driver on the oracle's rules with the restatement as either side's search: the device
    search is not compared with itself.  Mcts against Mcts: two counter blocks, one set of slabs"""
    from oracle import oracle as orc
    from oracle.arena_backend import OracleRules
    from vanilla_ref import COUNTERS, RefSearch, mct_search_batch

    class Counting(RefSearch):                                  # RefSearch.vanilla, keeping the restatement's counters
        def __init__(self):
            self.stats = dict.fromkeys(COUNTERS, 0)

        def vanilla(self, states, cfg, seed, ids, rounds, ref_quirks):
            assert not ref_quirks                               # vanilla_rollouts=True
            r = mct_search_batch(np.ascontiguousarray(states).view(orc.BG_STATE).reshape(-1), cfg.iterations, cfg.c, cfg.round_limit, seed,
                                 ids, rounds, ref_quirks)
            for k in COUNTERS:
                self.stats[k] += r["stats"][k]
            return r["plays"]

    cfg = cfg_of(10, round_limit=12)
    kw = dict(seed=31, num_games=6, round_limit=400, max_rounds=8, vanilla_rollouts=True)
    dev = versus.play_device(P(a1, engine if a1 == MCTS else None), P(a2, engine if a2 == MCTS else None), cfg, 1.25, **kw)
    srch = [Counting() if a == MCTS else None for a in (a1, a2)]
    ref = versus.play(P(a1), P(a2), cfg, 1.25, rules=OracleRules(), search1=srch[0], search2=srch[1], **kw)
    assert_same_games(dev, ref)
    assert dev.rounds == 8
    for s, a in enumerate((a1, a2)):
        st = dev.device["stats"][s]
        if a == MCTS:
            print(vc.line(f"arena {a1} vs {a2}, side {s}", srch[s].stats))
            assert srch[s].stats["iterations"] > 0
            assert st["selections"] == srch[s].stats["iterations"]
            assert (st["expansions"], st["terminal_hits"], st["depth_sum"]) == tuple(srch[s].stats[k] for k in ("expansions", "terminal_hits", "depth_sum"))
        else:
            assert st["selections"] == 0


def test_case6_arena_mcts_against_mcts_to_the_end(engine):
    """four games to their end, both sides searching: the device arena against the host driver over the same engine's search"""
    cfg = cfg_of(6, round_limit=8)
    p = P(MCTS, engine)
    kw = dict(seed=31, num_games=4, round_limit=400, vanilla_rollouts=True)
    dev = versus.play_device(p, p, cfg, 1.25, **kw)
    ref = versus.play(p, p, cfg, 1.25, **kw)
    assert_same_games(dev, ref)
    st = dev.device["stats"]
    print(f"[vanilla-parity] arena Mcts vs Mcts to the end: rounds {dev.rounds}  wins {dev.wins_p1} / {dev.wins_p2}  draws {dev.draws}  "
          f"selections {st[0]['selections']} / {st[1]['selections']}")
    assert st[0]["selections"] > 0 and st[1]["selections"] > 0
    assert dev.wins_p1 + dev.wins_p2 + dev.draws == 4 and len(dev.games) == 4
