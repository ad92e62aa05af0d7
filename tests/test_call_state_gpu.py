"""Calls on one context do not see each other's leftovers: a sequence that reaches all three dispatch paths of a move-step's search
(k_tail, the free-running search, launch per iteration behind them), slot refill's table of Dirichlet samples and the arena, run twice
over on ONE engine, gives byte for byte what each call gives as the FIRST call of a fresh engine."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0xD1EE0001
ITERS = 8
STAT_KEYS = ("expansions", "children", "selections", "depth_sum", "tail_iterations")


def new_engine():
    import diee_amd
    e = diee_amd.Engine(0)
    e.load_weights(diee_amd.random_weights(0))
    return e


def cfg(**kw):
    import diee_amd
    d = dict(iterations=ITERS, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25); d.update(kw)
    return diee_amd.MctsConfig(**d)


def roots(oracle, n):
    return oracle.random_walk_states(77, 40)[200:200 + 7 * n:7]


def stats_of(st):
    return tuple(int(st[k]) for k in STAT_KEYS)


def records(batches):
    return [tuple(b[k].tobytes() for k in ("game", "outcome", "state", "ps")) + (stats_of(b["stats"]),) for b in batches]


def search(e, oracle, n):
    states = roots(oracle, n)
    assert len(states) == n
    gids = np.arange(100, 100 + n, dtype=np.uint32); rds = np.arange(n, dtype=np.uint32) % 5
    r = e.alpha_mcts_parallel(states, cfg(), SEED, 3, gids, rds, ref_quirks=True)
    return (r["probs"].tobytes(), r["n_children"].tobytes(), r["root_visits"].tobytes(), stats_of(r["stats"]))


def call_refill(e, oracle):
    return records(e.self_play_refill([(6, 0, SEED), (6, 100, SEED + 1)], 4, cfg(round_limit=5), 1.25, max_steps=4))


def call_free(e, oracle):
    r = search(e, oracle, 20)
    assert r[3][4] > 0                                      # (the speculative paths ran: 17 ... 800 roots are the free-running band)
    return r


def call_tail(e, oracle):
    r = search(e, oracle, 6)
    assert r[3][4] > 0
    return r


def call_arena(e, oracle):
    import diee_amd
    r = e.arena(diee_amd.AGENT_MODEL, None, diee_amd.AGENT_RANDOM, 20, cfg(), 1.25, seed=7, max_rounds=3)
    return (r["winner"].tobytes(), r["retired_round"].tobytes(), r["retired_side"].tobytes(), r["initial_states"].tobytes(),
            r["final_states"].tobytes(), (r["wins_p1"], r["wins_p2"], r["draws"], r["rounds"]), [stats_of(s) for s in r["stats"]])


def call_self_play(e, oracle):
    return records([e.self_play_parallel(20, cfg(), 1.25, SEED + 2, ref_quirks=True, max_steps=3)])


def call_refused(e, oracle):
    import diee_amd
    with pytest.raises(diee_amd.DieeError) as ei:
        e.self_play_refill([(6, 0, SEED)], 0, cfg(round_limit=5), 1.25, max_steps=4)
    assert ei.value.status == diee_amd.ERR_ARG               # refused on its arguments, before any launch
    return ei.value.status


CALLS = [call_refill, call_free, call_tail, call_arena, call_self_play, call_refused]


@pytest.fixture(scope="module")
def first_calls(oracle):
    """every call of the sequence as the first call of a fresh engine (computed once, never modified)"""
    out = []
    for fn in CALLS:
        e = new_engine()
        try:
            out.append(fn(e, oracle))
        finally:
            e.close()
    return out


def test_calls_on_one_context_leave_nothing_behind(oracle, first_calls):
    e = new_engine()
    try:
        for lap in range(2):
            for fn, ref in zip(CALLS, first_calls):
                assert fn(e, oracle) == ref, (lap, fn.__name__)
    finally:
        e.close()
