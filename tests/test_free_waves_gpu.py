"""k_free's shortened chain (die-e_amd/csrc/mcts_kernels.hip): a selection level with one child per lane found by one maximum and two
ballots, the virtual descents on their register / one-trip path while the tree is resident in LDS, every game's first-selection word
written before round 0.  None of it may show in a result: small batches -- odd sizes, one game more than a wave's worth of batch
scan, bear-off roots where the `node_selected` / stale-slot words (Q14) are live -- against the CPU oracle's lockstep search with the engine's
own evaluator, visits, probabilities and counters bit for bit; the same with the tree in HBM alone (free_lds_nodes = 64: the general descent),
one iteration per launch, and a ring of 4 launches (rows age out and are demanded again)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0xD1EE0001
KEYS = ("nn_evals", "expansions", "children", "terminal_hits", "depth_sum", "selections", "max_children")
DEFAULTS = dict(free_eval=1, free_min_games=17, free_max_games=800, free_rows1024_from=200, free_rollout_steps=24, free_cand_max=12,
                free_ring=128, free_lds_nodes=3072, free_iter_cap=4, spec_eval=1)
CASES = [(17, 30, "mixed"), (40, 30, "mixed"), (65, 30, "mixed"), (3, 48, "late"), (16, 48, "late")]
VARIANTS = [dict(), dict(free_lds_nodes=64), dict(free_iter_cap=1), dict(free_ring=4)]


@pytest.fixture(scope="module")
def eng():
    import diee_amd
    e = diee_amd.Engine(0)
    e.load_weights(diee_amd.random_weights(0))
    e.set_invariant_nn(True)                     # rows of the fused family = what the oracle's evaluator (forward_t) computes, at every size
    yield e
    e.close()


def gpu_eval(eng, oracle):
    def fn(states_u8):
        return eng.forward_t(states_u8.view(oracle.BG_STATE).reshape(-1))
    return oracle.make_eval(fn, 1352)


def cfgs(oracle, iters, **kw):
    import diee_amd
    d = dict(iterations=iters, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25); d.update(kw)
    return oracle.MctsCfg(**d), diee_amd.MctsConfig(**d)


def roots_of(oracle, n, pick):
    walk = oracle.random_walk_states(321, 400)
    late = walk[walk["off"].max(axis=1) >= 12]
    if pick == "late":
        return late[2:2 + n]
    k = min(n // 3, len(late))
    rest = walk[np.linspace(5, len(walk) - 1, n - k).astype(int)]
    return np.concatenate([late[:k], rest])


def check(res, roots, probs, ostats, name):
    assert res["probs"].tobytes() == probs.tobytes(), (name, np.abs(np.nan_to_num(res["probs"]) - np.nan_to_num(probs)).max())
    assert (res["root_visits"] == np.array([x["visits"] for x in roots], dtype=np.float32)).all(), name
    assert (res["n_children"] == np.array([len(x["children"]) for x in roots], dtype=np.uint32)).all(), name
    for key in KEYS:
        assert res["stats"][key] == ostats[key], (name, key, res["stats"][key], ostats[key])


_REF = {}


def reference(eng, oracle, states, iters, quirks, step, key):
    """the oracle's search of a case, computed once and shared by the option variants"""
    if key not in _REF:
        n = len(states)
        gids = np.arange(90, 90 + n, dtype=np.uint32); rds = (np.arange(n, dtype=np.uint32) * 3) % 7
        ocfg, _ = cfgs(oracle, iters)
        roots, probs, ostats, _x = oracle.alpha_mcts_parallel(1, states, ocfg, gpu_eval(eng, oracle), None, SEED, step, gids, rds, quirks)
        _REF[key] = (roots, probs, ostats.as_dict(), gids, rds)
    return _REF[key]


def free_search(eng, oracle, states, iters, quirks, step, gids, rds, **opts):
    _, gcfg = cfgs(oracle, iters)
    eng.set_options(free_min_games=1, spec_eval=0, **opts)          # (spec_eval = 0: k_tail stays out of the way)
    try:
        return eng.alpha_mcts_parallel(states, gcfg, SEED, step, gids, rds, ref_quirks=bool(quirks))
    finally:
        eng.set_options(**DEFAULTS)


@pytest.mark.parametrize("opts", VARIANTS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("n,iters,pick", CASES)
def test_small_batches_bit_exact_vs_oracle(eng, oracle, n, iters, pick, quirks, opts):
    states = roots_of(oracle, n, pick)
    assert len(states) == n
    roots, probs, os_, gids, rds = reference(eng, oracle, states, iters, quirks, 5, (n, iters, pick, quirks))
    r = free_search(eng, oracle, states, iters, quirks, 5, gids, rds, **opts)
    check(r, roots, probs, os_, f"{n} x {iters} {pick} quirks {quirks} {opts}")
    assert r["stats"]["tail_iterations"] == iters                    # the free-running search ran


def test_roots_with_more_than_64_sequences_before_dedup(eng, oracle):
    """doubles positions whose DFS lists more than 64 sequences: the multi-chunk compaction of the legal plays"""
    walk = oracle.random_walk_states(321, 400)
    dbl = walk[(walk["roll"][:, 0] == walk["roll"][:, 1]) & (walk["off"].max(axis=1) == 0)]
    def raw_count(st):                                               # sequences of the DFS before remove_duplicate_states
        return oracle.bg_valid_moves(np.array(st), with_raw_count=True)[1]
    big = []
    for i in range(len(dbl)):
        if raw_count(dbl[i]) > 64:
            big.append(i)
            if len(big) == 6:
                break
    assert len(big) >= 2, "no doubles position with S > 64 among the walk's states"
    states = np.concatenate([dbl[big], roots_of(oracle, 23 - len(big), "mixed")])
    for i in range(len(big)):
        assert raw_count(states[i]) > 64
    roots, probs, os_, gids, rds = reference(eng, oracle, states, 30, 1, 6, "S>64")
    r = free_search(eng, oracle, states, 30, 1, 6, gids, rds)
    check(r, roots, probs, os_, "S > 64")
    assert r["stats"]["tail_iterations"] == 30


def test_first_selection_on_a_finished_game(eng, oracle):
    """bear-off roots, quirks on, where the root expansion's own selection (iteration 0's) lands on a finished game for at least one game --
    its selection stays `none` and the batch's first slot counts it as a stale initial slot (Q14): what k_free's first-selection words
    carry.  One iteration of the oracle shows the condition: every terminal hit of iteration 0 is such a selection."""
    states = roots_of(oracle, 24, "late")
    gids = np.arange(90, 114, dtype=np.uint32); rds = (np.arange(24, dtype=np.uint32) * 3) % 7
    ocfg1, _ = cfgs(oracle, 1)
    _r, _p, st1, _x = oracle.alpha_mcts_parallel(1, states, ocfg1, gpu_eval(eng, oracle), None, SEED, 7, gids, rds, 1)
    hits = st1.as_dict()["terminal_hits"]
    assert hits > 0, hits                                            # at least one game's first selection is a finished game
    roots, probs, os_, gids, rds = reference(eng, oracle, states, 48, 1, 7, "first-sel")
    for opts in (dict(), dict(free_iter_cap=1)):
        r = free_search(eng, oracle, states, 48, 1, 7, gids, rds, **opts)
        check(r, roots, probs, os_, f"first selection {opts}")


def test_two_batches_side_by_side_into_the_bear_off(eng, oracle):
    """two batches share the slot space down to their last games (free_min_games = 1: every move-step's search runs free), each with its own
    flag words and first slot: whole games, so every batch passes through bear-off positions whose first selection is a finished game"""
    ocfg, gcfg = cfgs(oracle, 6, round_limit=120)
    batches = [(12, 0, 271), (9, 500, 272)]
    ref, _ = oracle.self_play_multi(1, batches, ocfg, 1.25, gpu_eval(eng, oracle), None, ref_quirks=1)
    eng.set_options(free_min_games=1, spec_eval=0)
    try:
        out = eng.self_play_multi(batches, gcfg, 1.25, ref_quirks=True, invariant_nn=True)
    finally:
        eng.set_options(**DEFAULTS)
    for o, r in zip(out, ref):
        assert o["ps"].tobytes() == r["ps"].tobytes() and o["state"].tobytes() == r["state"].tobytes() and (o["outcome"] == r["outcome"]).all()
        for key in KEYS:
            assert o["stats"][key] == r["stats"][key], key
        assert r["stats"]["terminal_hits"] > 0
    assert out[0]["stats"]["tail_iterations"] > 0


def test_tree_arena_too_small_is_still_reported(oracle):
    """nodes_per_expansion = 1: the trees outgrow their arena in mid-search; the call reports DIEE_ERR_CAPACITY (nothing is written past
    node_cap: the engine stays usable and the next search is bit-equal to the launch-per-iteration one)"""
    import diee_amd
    e = diee_amd.Engine(0)
    e.load_weights(diee_amd.random_weights(0))
    try:
        states = roots_of(oracle, 40, "mixed")
        e.set_options(free_min_games=1, spec_eval=0, nodes_per_expansion=1)
        with pytest.raises(diee_amd.DieeError) as ei:
            e.alpha_mcts_parallel(states, diee_amd.MctsConfig.default(64), SEED, 0)
        assert ei.value.status == diee_amd.ERR_CAPACITY
        e.set_option("nodes_per_expansion", 128)
        r = e.alpha_mcts_parallel(states, diee_amd.MctsConfig.default(16), SEED, 0)
        e.set_options(free_eval=0)
        plain = e.alpha_mcts_parallel(states, diee_amd.MctsConfig.default(16), SEED, 0)
        assert r["stats"]["tail_iterations"] == 16 and plain["stats"]["tail_iterations"] == 0
        assert r["probs"].tobytes() == plain["probs"].tobytes() and (r["n_children"] == plain["n_children"]).all()
    finally:
        e.close()


def test_two_threads_on_a_shared_gpu(oracle):
    """`shared_gpu` = 1, two engines searching from two threads at once, 40 games each: the free-running search waits for nobody, so the
    two contexts' launches may interleave freely -- both equal to the oracle's lockstep search"""
    import diee_amd
    engines = []
    for _ in range(2):
        e = diee_amd.Engine(0)
        e.load_weights(diee_amd.random_weights(0))
        e.set_invariant_nn(True)
        e.set_options(shared_gpu=1, free_min_games=1, spec_eval=0)
        engines.append(e)
    try:
        n, iters = 40, 24
        states = roots_of(oracle, n, "mixed")
        roots, probs, os_, gids, rds = reference(engines[0], oracle, states, iters, 1, 8, "shared")
        _, gcfg = cfgs(oracle, iters)
        res = [None, None]

        def run(i):
            res[i] = engines[i].alpha_mcts_parallel(states, gcfg, SEED, 8, gids, rds, ref_quirks=True)
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for i in range(2):
            assert res[i] is not None, "a search thread failed"
            check(res[i], roots, probs, os_, f"shared_gpu, thread {i}")
            assert res[i]["stats"]["tail_iterations"] == iters
    finally:
        for e in engines:
            e.close()
