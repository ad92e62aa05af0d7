"""Agent::Mcts for tic-tac-toe restated for the tests (TEST INFRASTRUCTURE; imported by tests only, imports nothing of die-e_amd/).

`mct_search` (src/mcts/simple_mcts.rs:10-39) and `Node` (src/mcts/node.rs) per root, in the reference's control flow -- a list of nodes,
`expandable.pop()`, the `max_by` folds --, on pure-Python rules (src/tictactoe/mod.rs:36-81), np.float32 arithmetic and the oracle's
uniform.  The engine's choices (ln from a table, the RNG counters, the rollout as it was meant when the quirks are off) are the ones
include/diee.h lists for diee_ttt_mcts_vanilla_batch; the engine must match this bit for bit, on the host and on the device.
"""
import math

import numpy as np

from oracle import oracle as orc

TAG_VANILLA = 0xFFFFFFFB
EMPTY_MOVE = 10
COUNTERS = ("iterations", "expansions", "terminal_hits", "dead_end_hits", "rollouts", "rollout_plies", "rollout_decided", "depth_sum")
LINES = ((0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6))


def check_winner(board):                       # mod.rs:59-79: Some(winner), Some(0) on a full board, else None
    for a, b, c in LINES:
        if board[a] != 0 and board[a] == board[b] == board[c]:
            return board[a]
    return None if 0 in board else 0


def valid_moves(board):
    return [i for i in range(9) if board[i] == 0]


def apply_move(board, player, move):
    return board[:move] + (player,) + board[move + 1:], -player


class Node:                                    # node.rs:10-22
    def __init__(self, board, to_move, parent, move):
        self.board, self.to_move, self.parent, self.move = board, to_move, parent, move
        self.children = []
        self.expandable = valid_moves(board)
        self.visits = np.float32(0.0)
        self.value = np.float32(0.0)


def mct_search(board, to_move, iterations, c, round_limit, seed, game_id=0, rnd=0, ref_quirks=True):
    """-> dict(move (EMPTY_MOVE = 10), child_visits, child_values (f32 lists, creation order), stats)"""
    st = dict.fromkeys(COUNTERS, 0)
    board = tuple(int(x) for x in board)
    nodes = [] if check_winner(board) is not None else [Node(board, int(to_move), None, None)]      # simple_mcts.rs:12-14
    player = int(to_move)
    c = np.float32(c)
    ln = [None] + [np.float32(math.log(k)) for k in range(1, iterations + 2)]

    def value_of(w):
        return np.float32(1.0 if w == player else -1.0 if w == -player else 0.0)

    def select_child(i):                       # node.rs:86-96 under Iterator::max_by: the last of equal maxima, NaN is Equal
        best, bu = None, None
        for ci in nodes[i].children:
            n = nodes[ci]
            with np.errstate(all="ignore"):
                u = n.value / n.visits + np.sqrt((c * ln[int(nodes[i].visits)]) / n.visits)
            if best is None or not (bu > u):
                best, bu = ci, u
        return best

    def simulate(b, tm, it):                   # node.rs:176-196
        st["rollouts"] += 1
        for p in range(min(round_limit, 1) if ref_quirks else round_limit):       # Q22: one look at the node's own state, nothing played
            w = check_winner(b)
            if w is not None:
                st["rollout_decided"] += 1
                return value_of(w)
            if ref_quirks:
                break
            mv = valid_moves(b)
            u = orc.lib().or_uniform01(seed, game_id, rnd, TAG_VANILLA, (it << 12) | (1 + p))
            b, tm = apply_move(b, tm, mv[min(int(u * len(mv)), len(mv) - 1)])
            st["rollout_plies"] += 1
        return np.float32(0.0)

    for it in range(iterations if nodes else 0):           # simple_mcts.rs:17-37
        i, depth = 0, 0
        while nodes[i].children and not nodes[i].expandable:       # :88-94
            i, depth = select_child(i), depth + 1
        st["iterations"] += 1
        st["depth_sum"] += depth
        w = check_winner(nodes[i].board)
        if w is not None:                      # :25-30
            st["terminal_hits"] += 1
            result = value_of(w)
        else:                                  # expand, node.rs:118-137
            move = nodes[i].expandable.pop()
            nodes.append(Node(*apply_move(nodes[i].board, nodes[i].to_move, move), i, move))
            nodes[i].children.append(len(nodes) - 1)
            i = len(nodes) - 1
            st["expansions"] += 1
            result = simulate(nodes[i].board, nodes[i].to_move, it)
        while i is not None:                   # backpropagate, simple_mcts.rs:96-103
            nodes[i].visits = nodes[i].visits + np.float32(1.0)
            nodes[i].value = nodes[i].value + result
            i = nodes[i].parent

    ch = nodes[0].children if nodes else []
    best = None                                # :71-86 max_by_key(visits): the last of equal maxima
    for ci in ch:
        if best is None or nodes[ci].visits >= nodes[best].visits:
            best = ci
    return {"move": EMPTY_MOVE if best is None else nodes[best].move, "child_visits": [nodes[i].visits for i in ch],
            "child_values": [nodes[i].value for i in ch], "stats": st}


def mct_search_batch(states, cfg, seed, game_ids=None, rounds=None, ref_quirks=True):
    """the roots one by one -> what Engine.ttt_mct_search returns"""
    n = len(states)
    out = {"moves": np.full(n, EMPTY_MOVE, dtype=np.uint8), "n_children": np.zeros(n, dtype=np.uint32),
           "child_visits": np.zeros((n, 9), dtype=np.float32), "child_values": np.zeros((n, 9), dtype=np.float32),
           "stats": dict.fromkeys(COUNTERS, 0)}
    for i in range(n):
        r = mct_search(states[i]["board"], states[i]["player"], cfg.iterations, cfg.c, cfg.round_limit, seed,
                       int(i if game_ids is None else game_ids[i]), int(0 if rounds is None else rounds[i]), ref_quirks)
        k = len(r["child_visits"])
        out["moves"][i] = r["move"]; out["n_children"][i] = k
        out["child_visits"][i, :k] = r["child_visits"]; out["child_values"][i, :k] = r["child_values"]
        for key in COUNTERS:
            out["stats"][key] += r["stats"][key]
    return out


def assert_same(got, want):
    """every output and every counter, bit for bit"""
    for key in ("moves", "n_children", "child_visits", "child_values"):
        assert got[key].tobytes() == want[key].tobytes(), (key, got[key], want[key])
    for key in COUNTERS:
        assert got["stats"][key] == want["stats"][key], (key, got["stats"], want["stats"])
