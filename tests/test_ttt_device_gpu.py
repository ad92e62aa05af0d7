"""Option "nn" = "device" of a tic-tac-toe ctx: the 64 x 4 ResNet in one launch of k_ttt_net (die-e_amd/csrc/ttt_kernels.hip), against
the float64 evaluation of oracle/nn_ref.py, against itself (row independence) and under the oracle's search.  B = 16 boards per workgroup."""
import numpy as np
import pytest
import torch

import diee_amd
from oracle import nn_ref
from test_ttt_cpu import _blob_with_batchnorm_statistics, _oracle_eval, cfgs

pytestmark = pytest.mark.gpu
B = 16


def _states(n, seed=11):
    """seeded random legal play from the empty board (0 .. 9 plies, so either side is to move), the empty and a full board first"""
    rng = np.random.default_rng(seed)
    out = diee_amd.ttt_new(n)
    full = diee_amd.ttt_new(); full["board"] = [1, -1, 1, 1, -1, -1, -1, 1, 1]; full["player"] = 1
    for i in range(1, n):
        s = diee_amd.ttt_new()
        for _ in range(int(rng.integers(0, 10))):
            if diee_amd.ttt_check_winner(s) is not None:
                break
            s = diee_amd.ttt_apply_move(s, rng.choice(diee_amd.ttt_valid_moves(s)))
        out[i] = full if i == 1 else s
    return out


def _exact_blob():
    """every conv: one tap of one input channel per output channel, weight -1 or +1, no bias, identity BatchNorm; FC weights exact in bf16"""
    rng = np.random.default_rng(5); parts = []
    def conv(co, ci, j):
        w = np.zeros((co, ci, 9), dtype=np.float32); o = np.arange(co)
        w[o, (7 * o + j) % ci, (o + j) % 9] = rng.choice([-1.0, 1.0, 1.0, 1.0], co)       # 7 is coprime to 3 and 64: all channels, all taps
        parts.extend([w.ravel(), np.zeros(co)])
    bn = lambda c: parts.extend([np.ones(c), np.zeros(c), np.zeros(c), np.full(c, 1 - 1e-5)])
    bf = lambda a: (a.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    conv(64, 3, 0); bn(64)
    for b in range(4):
        conv(64, 64, 2 * b + 1); conv(64, 64, 2 * b + 2); bn(64); bn(64)
    conv(32, 64, 9); bn(32); parts.extend([bf(rng.uniform(-0.06, 0.06, 9 * 288)), bf(rng.uniform(-0.06, 0.06, 9))])
    conv(3, 64, 10); bn(3); parts.extend([bf(rng.uniform(-0.2, 0.2, 27)), bf(rng.uniform(-0.2, 0.2, 1))])
    return np.concatenate(parts).astype(np.float32)


def _reference(blob, states):
    planes = np.stack([diee_amd.ttt_planes(s) for s in states])
    p, v, _ = nn_ref.forward_t(nn_ref.parse(blob, 64, 4, 9, 3, 9), planes, dtype=torch.float64, shape=(3, 3, 3))
    return p, v


def _engine(blob, nn="device"):
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    e.set_option("nn", nn)
    e.load_weights(blob)
    return e


@pytest.fixture(scope="module")
def case():
    """name -> (engine on the device path, the 3B + 5 states, their float64 reference)"""
    states = _states(3 * B + 5)
    blob = diee_amd.random_weights(0, diee_amd.GAME_TTT)
    out = {k: (_engine(b), states, _reference(b, states)) for k, b in (("init", blob), ("bn", _blob_with_batchnorm_statistics(blob)))}
    yield out
    for e, _, _ in out.values():
        e.close()


# measured on an MI355X over the 53 states: max |d policy| 2.02e-5 (init) / 2.43e-4 (bn), max |d value| 1.47e-4 (init) / 1.62e-3 (bn); the
# bound is 3 x the larger of the two, under the 19-block net's bar (2e-3 policy, 1e-2 value)
POLICY_BOUND, VALUE_BOUND = 3 * 2.43e-4, 3 * 1.62e-3
assert POLICY_BOUND <= 2e-3 and VALUE_BOUND <= 1e-2


@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 3 * B + 5])
@pytest.mark.parametrize("name", ["init", "bn"])
def test_forward_matches_the_float64_restatement(case, name, n):
    eng, states, (rp, rv) = case[name]
    p, v = eng.forward_t(states[:n])
    dp, dv = np.abs(p - rp[:n]).max(), np.abs(v - rv[:n]).max()
    print(f"{name} n={n}: max|dpolicy| {dp:.3e} max|dvalue| {dv:.3e}")
    assert dp < POLICY_BOUND and dv < VALUE_BOUND
    assert np.abs(p.sum(1) - 1).max() < 1e-5


def test_exact_arithmetic_blob_pins_taps_padding_and_channels():
    """integer activations (|x| <= 16) are exact in bf16, so the device may differ from float64 only as the host's fp32 loops do.  The
    host path deviates by 3.0e-8 (policy) and 3.0e-8 (value) on these inputs, and so did the device when measured; the bound is 10 x the
    host's deviation, floored at 1e-6."""
    blob, states = _exact_blob(), _states(B + 1, seed=12)
    rp, rv = _reference(blob, states)
    assert np.abs(rp - 1 / 9).max() > 0.05                                  # the net is alive: the policy is far from uniform
    host = _engine(blob, "host"); hp, hv = host.forward_t(states); host.close()
    dev = _engine(blob); p, v = dev.forward_t(states); dev.close()
    hdp, hdv = np.abs(hp - rp).max(), np.abs(hv - rv).max()
    dp, dv = np.abs(p - rp).max(), np.abs(v - rv).max()
    print(f"host {hdp:.3e} {hdv:.3e} device {dp:.3e} {dv:.3e}")
    assert dp <= max(10 * hdp, 1e-6) and dv <= max(10 * hdv, 1e-6)


def test_a_boards_bits_do_not_depend_on_row_batch_or_call(case):
    eng, states, _ = case["bn"]
    for k in (0, 7, 30):
        p1, v1 = eng.forward_t(states[k:k + 1])
        batch = np.roll(states, 3).copy()
        rows = [5, B + 6, 3 * B + 4]                                        # the last one in the partial workgroup
        batch[rows] = states[k]
        p, v = eng.forward_t(batch)
        for r in rows:
            assert p[r].tobytes() == p1[0].tobytes() and v[r].tobytes() == v1[0].tobytes()
        q, w = eng.forward_t(batch)
        assert q.tobytes() == p.tobytes() and w.tobytes() == v.tobytes()


@pytest.mark.parametrize("quirks", [1, 0])
def test_search_through_the_device_net_is_bit_exact_vs_oracle(case, oracle, quirks):
    eng = case["init"][0]
    boards = [[0] * 9, [-1, 1, 0, 0, -1, 0, 0, 0, 1], [-1, -1, 0, 1, 1, 0, 0, 0, 0], [1, -1, 1, -1, -1, 1, 0, 1, 0], [-1, 1, -1, -1, 1, 1, 0, 0, 0]]
    states = diee_amd.ttt_new(len(boards)); n = len(states)
    for i, b in enumerate(boards):
        states[i]["board"] = b
        states[i]["player"] = -1 if sum(1 for x in b if x) % 2 == 0 else 1
    ocfg, gcfg = cfgs(oracle, 60)
    roots, probs, ostats, _ = oracle.alpha_mcts_parallel(0, states.view(np.uint8).reshape(n, 32), ocfg, _oracle_eval(eng, oracle), None, 5, 2,
                                                         np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), quirks)
    r = eng.alpha_mcts_parallel(states, gcfg, 5, 2, ref_quirks=bool(quirks))
    assert r["probs"].tobytes() == probs.tobytes()
    assert (r["root_visits"] == np.array([x["visits"] for x in roots], dtype=np.float32)).all()
    assert (r["n_children"] == np.array([len(x["children"]) for x in roots])).all()
    for key in ("nn_evals", "expansions", "children", "terminal_hits", "depth_sum", "selections", "max_children"):
        assert r["stats"][key] == ostats.as_dict()[key], key
    ocfg, gcfg = cfgs(oracle, 30)
    ref = oracle.self_play_parallel(0, 8, ocfg, 1.25, 77, _oracle_eval(eng, oracle), None, ref_quirks=quirks, first_game_id=40)
    out = eng.self_play_parallel(8, gcfg, 1.25, 77, ref_quirks=bool(quirks), first_game_id=40)
    assert len(out["outcome"]) == len(ref["outcome"]) > 0 and out["outcome"].tobytes() == ref["outcome"].tobytes()
    assert out["game"].tobytes() == ref["game"].tobytes()
    assert out["state"].tobytes() == ref["state"].tobytes() and out["ps"].tobytes() == ref["ps"].tobytes()


def test_switching_back_restores_the_host_bits(case):
    _, states, _ = case["init"]
    blob = diee_amd.random_weights(0, diee_amd.GAME_TTT)
    eng, fresh = _engine(blob), _engine(blob, "host")
    dp, _ = eng.forward_t(states[:B])
    assert eng.get_option("nn") == "device"
    eng.set_option("nn", "host")
    assert eng.get_option("nn") == "host"
    states64 = np.concatenate([states, states[:11]])
    (p, v), (fp, fv) = eng.forward_t(states64), fresh.forward_t(states64)
    assert len(states64) == 64 and p.tobytes() == fp.tobytes() and v.tobytes() == fv.tobytes()
    assert dp.tobytes() != p[:B].tobytes()                                  # the device path was a different computation
    eng.close(); fresh.close()
