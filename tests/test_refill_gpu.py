"""Slot refill (diee_self_play_refill): at most `width` games in flight, a retired game's slot taken in the next move-step by the
next unstarted game.  Without the quirks nothing couples the games of a batch but the Dirichlet sample of a move-step, and a game
admitted late reads the sample of its own round -- so per batch the records are those of ONE plain self_play_parallel call
(ref_quirks = 0) of the oracle, game by game, bit for bit; only the order of the games differs (they appear by the move-step of the
refill call in which they retired).  The oracle's evaluator is the engine's own ResNet, batch-size independent for the comparison
(diee_set_invariant_nn), so both sides see the same priors and values whatever shares a launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0xD1EE0001


@pytest.fixture(scope="module")
def eng():
    import diee_amd
    e = diee_amd.Engine(0)
    e.load_weights(diee_amd.random_weights(0))
    yield e
    e.close()


def gpu_eval(eng, oracle):
    calls = {"n": 0}

    def fn(states_u8):
        calls["n"] += 1
        st = states_u8.view(oracle.BG_STATE).reshape(-1)
        return eng.forward_t(st)
    return oracle.make_eval(fn, 1352), calls


def cfgs(oracle, iters, **kw):
    import diee_amd
    d = dict(iterations=iters, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25); d.update(kw)
    return oracle.MctsCfg(**d), diee_amd.MctsConfig(**d)


_REFS = {}


def oracle_refs(eng, oracle, batches, iters, round_limit, invariant=True):
    """one sequential oracle call per batch (computed once per case and shared, never modified)"""
    key = (tuple(batches), iters, round_limit, invariant)
    if key not in _REFS:
        ocfg, _ = cfgs(oracle, iters, round_limit=round_limit)
        if invariant:
            eng.set_invariant_nn(True)
        try:
            ev, _ = gpu_eval(eng, oracle)
            _REFS[key] = [oracle.self_play_parallel(1, n, ocfg, 1.25, seed, ev, None, ref_quirks=0, first_game_id=first)
                          for n, first, seed in batches]
        finally:
            eng.set_invariant_nn(False)
    return _REFS[key]


def by_game(d):
    o = np.argsort(d["game"], kind="stable")
    return {k: d[k][o] for k in ("game", "outcome", "state", "ps")}


def cmp_batch(m, ref, n, sort=True):
    a, b = (by_game(m), by_game(ref)) if sort else (m, ref)
    assert len(a["game"]) == len(b["game"]) > 0
    assert (a["game"] == b["game"]).all() and (a["outcome"] == b["outcome"]).all()
    assert a["state"].tobytes() == b["state"].tobytes()
    assert a["ps"].tobytes() == b["ps"].tobytes()
    # a game's records are contiguous in the delivered order
    g = m["game"]
    assert len(np.flatnonzero(np.diff(g.astype(np.int64)) != 0)) + 1 == len(np.unique(g))
    # (not nn_evals: the oracle skips it in iterations where no game OF THE CALL selected a leaf -- not a per-game sum)
    for key in ("expansions", "children", "terminal_hits", "depth_sum", "selections", "max_children"):
        assert m["stats"][key] == ref["stats"][key], key
    assert m["stats"]["illegal_decodes"] == 0 and m["stats"]["games"] == n
    assert m["stats"]["plies"] == int(ref["plies"].sum())
    assert m["stats"]["fragments"] == len(ref["outcome"])


def refill(eng, oracle, batches, width, iters, round_limit, invariant=True, **kw):
    _, gcfg = cfgs(oracle, iters, round_limit=round_limit)
    return eng.self_play_refill(batches, width, gcfg, 1.25, invariant_nn=invariant, **kw)


def test_refill_to_completion(eng, oracle):
    """whole games (random-init games run ~107 plies): 10 games through 4 slots, every game admitted late plays its own rounds"""
    batches = [(5, 0, SEED), (5, 300, SEED + 1)]
    refs = oracle_refs(eng, oracle, batches, 8, 400)
    for r in refs:
        assert (r["winners"] != 0).all(), "the inputs are wrong: a game hit the round limit"
    out = refill(eng, oracle, batches, 4, 8, 400)
    for (n, first, seed), m, r in zip(batches, out, refs):
        cmp_batch(m, r, n)
        assert set(np.unique(m["outcome"])) <= {-1, 1}


HEAVY = [(9, 0, SEED), (7, 100, SEED + 1), (5, 40, SEED + 2)]


@pytest.mark.parametrize("opts", [{}, {"deliver_stage_rows": 3}])
def test_refill_round_limit_and_heavy_recycling(eng, oracle, opts):
    """round_limit 5: every game is flushed by the limit after six move-steps, so the 6 slots (and record areas) turn over four times;
    a staging buffer of 3 rows splits every step's delivery"""
    refs = oracle_refs(eng, oracle, HEAVY, 6, 5)
    saved = {k: eng.get_option(k) for k in opts}
    try:
        eng.set_options(**opts)
        out = refill(eng, oracle, HEAVY, 6, 6, 5)
    finally:
        eng.set_options(**saved)
    for (n, first, seed), m, r in zip(HEAVY, out, refs):
        cmp_batch(m, r, n)
    assert int(eng.get_option("refill_record_areas")) == 6


PATHS = [(35, 0, SEED + 3), (25, 500, SEED + 4)]


@pytest.mark.parametrize("width,invariant,opts,tail", [
    (12, True, {}, None),                                   # under the invariant arithmetic a search of <= 16 games is launch per iteration
    (12, False, {}, True),                                  # k_tail (cluster family on both sides: <= 128 boards are one arithmetic, row by row)
    (40, True, {}, True),                                   # the free-running search
    (40, True, {"free_eval": 0, "spec_eval": 0}, False),    # launch per iteration
])
def test_refill_on_each_search_path(eng, oracle, width, invariant, opts, tail):
    """60 games in 2 batches, iterations 6, round_limit 10.  k_tail does not run on the batch-invariant arithmetic (its launches of <= 128
    rows are of the split-K cluster family), so the width-12 case runs twice: invariant like every other comparison here, and on the
    default arithmetic -- where the oracle's evaluator sees at most 35 boards and the engine at most 12, both the cluster family, whose
    rows do not depend on what shares the launch -- to hold k_tail itself to the oracle"""
    refs = oracle_refs(eng, oracle, PATHS, 6, 10, invariant=invariant)
    saved = {k: eng.get_option(k) for k in opts}
    try:
        eng.set_options(**opts)
        out = refill(eng, oracle, PATHS, width, 6, 10, invariant=invariant)
    finally:
        eng.set_options(**saved)
    for (n, first, seed), m, r in zip(PATHS, out, refs):
        cmp_batch(m, r, n)
    if tail is True:
        assert out[0]["stats"]["tail_iterations"] > 0
    elif tail is False:
        assert out[0]["stats"]["tail_iterations"] == 0


@pytest.mark.parametrize("width", [21, 64])
def test_refill_at_full_width_is_self_play_multi(eng, oracle, width):
    """width >= the games of the call: nothing is ever admitted late -- diee_self_play_multi's output, byte for byte, in its order"""
    _, gcfg = cfgs(oracle, 6, round_limit=5)
    multi = eng.self_play_multi(HEAVY, gcfg, 1.25, ref_quirks=False, invariant_nn=True)
    out = refill(eng, oracle, HEAVY, width, 6, 5)
    for m, r in zip(out, multi):
        for key in ("game", "outcome", "state", "ps"):
            assert m[key].tobytes() == r[key].tobytes(), key
        for key in ("games", "plies", "move_steps", "nn_evals", "expansions", "children", "terminal_hits", "depth_sum", "selections",
                    "max_children", "fragments"):
            assert m["stats"][key] == r["stats"][key], key


def test_refill_admission_timing(eng, oracle):
    """round_limit 3: no game can end early, every game takes the L move-steps of a sequential call -- so the slots turn over in waves,
    a game is admitted in the move-step after its predecessor retired, and the call takes ceil(games / width) x L move-steps"""
    batches = [(18, 0, SEED + 5), (12, 70, SEED + 6)]
    refs = oracle_refs(eng, oracle, batches, 2, 3)
    L = refs[0]["steps"]
    assert L == refs[1]["steps"] and L >= 3
    for w in (7, 10, 30):
        out = refill(eng, oracle, batches, w, 2, 3)
        assert max(o["stats"]["move_steps"] for o in out) == -(-30 // w) * L, w
        for (n, first, seed), m, r in zip(batches, out, refs):
            cmp_batch(m, r, n)


def test_refill_memory_is_bounded_by_width(eng, oracle):
    """64 games through 8 slots: the record areas go by the width (3 x width is the most any scheme that quarantines freed areas may
    take; this one hands an area on once its records are gathered, so it takes exactly `width`)"""
    import diee_amd
    out = refill(eng, oracle, [(40, 0, SEED + 7), (24, 900, SEED + 8)], 8, 2, 3)
    assert [o["stats"]["games"] for o in out] == [40, 24]
    areas = int(eng.get_option("refill_record_areas"))
    assert 0 < areas < 64 and areas <= 3 * 8
    with pytest.raises(diee_amd.DieeError) as ei:
        eng.set_option("refill_record_areas", 5)
    assert ei.value.status == diee_amd.ERR_ARG


def test_refill_argument_errors(eng, oracle):
    import diee_amd
    _, gcfg = cfgs(oracle, 2, round_limit=3)
    bt = (diee_amd.Batch * 1)(diee_amd.Batch(4, 0, SEED))
    sts = (diee_amd.Stats * 1)()
    st = eng._L.diee_self_play_refill(eng._h, C.byref(bt), 1, 2, C.byref(gcfg), 1.25, diee_amd.FLAG_REF_QUIRKS, 0, None, C.byref(sts))
    assert st == diee_amd.ERR_ARG
    with pytest.raises(diee_amd.DieeError) as ei:
        eng.self_play_refill([(4, 0, SEED)], 0, gcfg)
    assert ei.value.status == diee_amd.ERR_ARG
    # fetch=False: nothing is delivered, the records are still counted
    full = eng.self_play_refill([(4, 0, SEED)], 2, gcfg)
    dry = eng.self_play_refill([(4, 0, SEED)], 2, gcfg, fetch=False)
    assert "ps" not in dry[0] and dry[0]["stats"]["fragments"] == full[0]["stats"]["fragments"] == len(full[0]["outcome"]) > 0
