"""Roots and reference answers of the Agent::Mcts edge cases (TEST INFRASTRUCTURE; imported by tests only, imports nothing of die-e_amd/).

The roots are positions of the oracle's random walks, chosen for a property of the search on them -- a root wider than a wavefront, a
race in which exploitation decides --; every property is a precondition that `check_*` asserts on the restatement (tests/vanilla_ref.py)
alone, so the CPU tier (tests/test_vanilla_cpu.py) notices when a change to the walks would hollow a GPU case out
(tests/test_vanilla_edges_gpu.py).  A reference answer is computed once per process and shared.
"""
import numpy as np

from oracle import oracle as orc
from vanilla_ref import COUNTERS, mct_search_batch

SEED = 77
WIDE_PLAYS = (91, 69, 64, 63, 65, 157)         # lanes 40..63 of vanilla_level's first pass, 63 | 64 | 65, two passes, three passes
WIDE = dict(iterations=230, c=2.0, round_limit=30)
SMALL_PLAYS = (3, 34, 59, 3)
CONSTS = dict(iterations=300, round_limit=120)  # case 3, quirks off; c is the case's
CS = (-1.0, 0.0, 0.5, float("inf"), float("nan"))
LIMITS = dict(iterations=40, c=2.0)             # case 4; round_limit is the case's
ROUND_LIMITS = (0, 1, 2)


def _walk5():
    return orc.random_walk_states(5, 40, 400)


def wide_roots():
    """W: six roots with WIDE_PLAYS legal plays"""
    roots = np.zeros(6, dtype=orc.BG_STATE)
    roots[:4] = _walk5()[[3024, 778, 120, 3048]]
    roots[4] = orc.random_walk_states(9, 60, 400)[1869]
    roots[5] = orc.bg_state(pts=[0, 4, 2, -1, -1, -1, -1, -1, -1, -1, 1, -1, -1, 1, -1, -1, -1, 1, -1, -1, 2, 3, 1, -1],
                            bar=(0, 0), off=(0, 0), roll=(2, 1), player=-1, second=0)
    _, cnt = orc.valid_moves_batch(roots, 256)
    assert tuple(int(k) for k in cnt) == WIDE_PLAYS, cnt
    assert {63, 64, 65} <= set(WIDE_PLAYS) and any(66 <= k <= 128 for k in WIDE_PLAYS) and any(k >= 129 for k in WIDE_PLAYS)
    return roots


def _late(walk):
    _, cnt = orc.valid_moves_batch(walk)
    return walk[(walk["off"].max(axis=1) >= 12) & (cnt > 1)]


def small_roots():
    """S: the walk's first position and three late ones (rollouts reach a winner), SMALL_PLAYS legal plays"""
    walk = _walk5()
    late = _late(walk)
    roots = np.zeros(4, dtype=orc.BG_STATE)
    roots[0] = walk[0]; roots[1] = late[0]; roots[2] = late[len(late) // 2]; roots[3] = late[-1]
    _, cnt = orc.valid_moves_batch(roots, 256)
    assert tuple(int(k) for k in cnt) == SMALL_PLAYS, cnt
    return roots


def long_root():
    """late[0] alone: the root of the long searches"""
    return small_roots()[1:2].copy()


def race_root():
    """R: a bear-off race with two plays whose values differ -- where the last of equal scores is not the child behind the last NaN"""
    r = _walk5()[1218:1219].copy()
    _, cnt = orc.valid_moves_batch(r, 256)
    assert int(cnt[0]) == 2 and r["off"][0].tolist() == [5, 6], (cnt, r["off"])
    return r


def const_roots():
    """S plus R, the roots of the exploration-constant cases"""
    return np.concatenate([small_roots(), race_root()])


def keys_of(n):
    """game ids and rounds of the cases' roots"""
    i = np.arange(n, dtype=np.uint32)
    return i * 3 + 1, i.copy()


_REF = {}


def reference(name, roots, iterations, c, round_limit, quirks):
    """the restatement's answer for the roots of a case, computed once: mct_search_batch's dict for all roots, and under "per_root"
    the counters of each root alone"""
    key = (name, iterations, repr(float(c)), round_limit, bool(quirks))
    if key not in _REF:
        ids, rounds = keys_of(len(roots))
        parts = [mct_search_batch(roots[i:i + 1], iterations, c, round_limit, SEED, ids[i:i + 1], rounds[i:i + 1], quirks)
                 for i in range(len(roots))]
        ref = {k: np.concatenate([p[k] for p in parts]) for k in ("plays", "n_children", "child_visits", "child_values")}
        ref["per_root"] = [p["stats"] for p in parts]
        ref["stats"] = {k: sum(p["stats"][k] for p in parts) for k in COUNTERS}
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def wide_reference(quirks):
    return reference("W", wide_roots(), WIDE["iterations"], WIDE["c"], WIDE["round_limit"], quirks)


def const_reference(c):
    return reference("SR", const_roots(), CONSTS["iterations"], c, CONSTS["round_limit"], False)


def limit_reference(round_limit, quirks):
    return reference("S", small_roots(), LIMITS["iterations"], LIMITS["c"], round_limit, quirks)


def check_wide(quirks):
    """case 1 on the reference alone: every root is fully expanded, every later iteration is selected through it, and some descents go
    on below its children -> the number of those"""
    ref, n = wide_reference(quirks), WIDE["iterations"]
    beyond = 0
    for i, k in enumerate(WIDE_PLAYS):
        st = ref["per_root"][i]
        assert int(ref["n_children"][i]) == k, (i, ref["n_children"][i])
        assert st["depth_sum"] >= n - k, (i, st)
        beyond += st["depth_sum"] - (n - k)
    assert beyond > 0
    return beyond


def check_consts():
    """case 3 on the reference alone: c = -1 (every score NaN but below a parent of one visit) and c = 0 (no NaN) disagree somewhere,
    and pure exploitation goes deep on the walk's first position"""
    neg, zero = const_reference(-1.0), const_reference(0.0)
    differ = [i for i in range(len(neg["n_children"])) if neg["child_visits"][i].tobytes() != zero["child_visits"][i].tobytes()]
    assert differ, "c = -1.0 and c = 0.0 give the same child_visits on every root"
    assert zero["per_root"][0]["depth_sum"] > 3 * CONSTS["iterations"], zero["per_root"][0]
    return differ


def check_limits():
    """case 4 on the reference alone, quirks off: no ply at limit 0, plies at 1, rollouts decided at 1 and 2"""
    st = {rl: limit_reference(rl, False)["stats"] for rl in ROUND_LIMITS}
    assert st[0]["rollout_plies"] == 0 and st[0]["rollout_decided"] == 0
    assert st[1]["rollout_plies"] > 0
    assert st[1]["rollout_decided"] > 0 and st[2]["rollout_decided"] > 0
    return st


def line(what, stats):
    """the reference's counters of a case, as the suites print them"""
    return f"[vanilla-parity] {what}: " + "  ".join(f"{k} {stats[k]}" for k in COUNTERS)
