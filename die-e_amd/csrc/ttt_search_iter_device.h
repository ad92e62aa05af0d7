// ttt_search_iter_device.h -- the ONE copy of an iteration of the tic-tac-toe device search: what k_ttt_search (ttt_search_kernels.hip, one
// launch per iteration, a game carried through SearchGame) and run_steps (ttt_search_run_device.h: k_ttt_search_run and k_ttt_selfplay_run,
// a game carried in registers) both run between their own ways of handing a game from one iteration to the next.  The two must give the same
// bits (tests/test_ttt_fused_gpu.py): they call the same statements.  The arithmetic is the host's (ttt_host.cpp) operation for operation:
// correctly rounded division and square root, no contraction, sums in ascending cell order.
// A game is a row of 16 lanes: lane j < 9 is child j of the node in hand (descent) or board cell j (expansion, root probabilities); what a
// row agrees on is kept redundantly in all its lanes.  The tree is RunNodes (ttt_search_device.h) in HBM or LDS: the children of a node are
// contiguous, first_child + j in ascending cell order like the host Store, so child j's action and state follow from the parent's state.
// Everything is DIEE_TTT_NO_PK_F32 and nothing but builtins (ttt_net_device.h says why); all stores are plain C++.
#pragma once
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_device.h"

namespace diee {
namespace ttt {

// Node::alpha_ucb, node.rs:98-112 = ucb() of ttt_host.cpp, f32 in this association (sq = sqrt(visits of the parent))
DIEE_TTT_FN float puct(float n, float val, float prior, float sq, float c) {
    const float q = n == 0.f ? 0.f : val / n;
    const float t = sq / (n + 1.0f);
    const float u = c * t;
    const float w = u * prior;
    return q + w;
}

// what a row of 16 lanes knows about its game during the search; every field is the same in all 16 lanes
struct Row {
    int32_t sel;
    uint32_t fresh, n_nodes, depth, sel_state, ever, cnt[kCntCount];     // SearchGame's fields of these names (ttt_search_device.h)
};

DIEE_TTT_FN uint32_t link_first(uint32_t link) { return link & 0xFFFFFu; }
DIEE_TTT_FN uint32_t link_children(uint32_t link) { return (link >> 20) & 0xFu; }
// the cell of set bit number `nth` of `mask` (the action of child `nth`)
DIEE_TTT_FN int nth_cell(uint32_t mask, uint32_t nth) {
    int cell = 0;
    uint32_t seen = 0u;
#pragma unroll
    for (int cidx = 0; cidx < 9; ++cidx) {
        const bool set = ((mask >> cidx) & 1u) != 0u;
        if (set && seen == nth) cell = cidx;
        seen += set ? 1u : 0u;
    }
    return cell;
}

// a diee_ttt_state (cells and player of -1 / 0 / +1) as the packed word of ttt_rules_device.h
DIEE_TTT_FN uint32_t unpack_root(const diee_ttt_state* root) {
    const uint32_t* r = (const uint32_t*)root;
    const uint32_t w0 = r[0], w1 = r[1], w2 = r[2];
    uint32_t state = 0u;
#pragma unroll
    for (int cidx = 0; cidx < 9; ++cidx) {
        const uint32_t w = cidx < 4 ? w0 : cidx < 8 ? w1 : w2;
        state |= pack_cell((int)(signed char)(w >> (8 * (cidx & 3))), cidx);
    }
    if ((signed char)(w2 >> 8) > 0) state |= 1u << 18;
    return state;
}

// The network's three cell words of a state (phase C): lane j < 3 of a valid row gets bytes 4 j .. 4 j + 3 of cells 0 .. 8, player; else 0.
DIEE_TTT_FN uint32_t net_word(bool valid, uint32_t state, int j) {
    uint32_t word = 0u;
    if (valid && j < 3) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int cidx = 4 * j + b;
            const int v = cidx < 9 ? cell_of(state, cidx < 9 ? cidx : 0) : cidx == 9 ? player_of(state) : 0;
            word |= ((uint32_t)v & 0xFFu) << (8 * b);
        }
    }
    return word;
}

// turn_policy_to_probs_tensor (utils.rs:74-84) + alpha_expand_tensor (node.rs:157-174) = expand() of ttt_host.cpp, for the rows whose `go`
// is set (all lanes of the wave come here: the ballot is wave-wide).  Lane j is cell j; `pol` is the policy row of the game's last evaluation.
DIEE_TTT_FN void expand(bool go, uint32_t slab, RunNode* nodes, const float* pol, Row& R, int idx, uint32_t state, int j, int row0) {
    const bool legal = go && j < 9 && ((state >> (2 * j)) & 3u) == 0u;
    const uint32_t mask = row_ballot(legal, row0);
    const uint32_t k = (uint32_t)__builtin_popcount(mask);
    if (!go || R.n_nodes + k > slab) return;                         // (the slab holds every expansion: run_node_bound)
    float sum = 0.f;
#pragma unroll
    for (int cidx = 0; cidx < 9; ++cidx) {                           // ascending cells: the order of expand()'s sum
        const float p = pol[cidx];
        if ((mask >> cidx) & 1u) sum += p;
    }
    if (legal) {
        RunNode* ch = nodes + R.n_nodes + (uint32_t)__builtin_popcount(mask & ((1u << j) - 1u));
        ch->visits = 0.f; ch->value = 0.f; ch->prior = pol[j] / sum; ch->link = 0u;
    }
    if (j == 0) nodes[idx].link = (k ? R.n_nodes : 0u) | (k << 20) | kRunDrained;
    R.n_nodes += k;
    R.cnt[kCntExpansions] += 1u; R.cnt[kCntChildren] += k;
    R.cnt[kCntMaxChildren] = k > R.cnt[kCntMaxChildren] ? k : R.cnt[kCntMaxChildren];
}

// Phase A of iteration 0: the search starts at `root_state`, root visits = 1, the root is expanded with the (noised) policy row `pol`.
DIEE_TTT_FN void start_search(bool valid, uint32_t slab, RunNode* nodes, const float* pol, Row& R, uint32_t root_state, int j, int row0) {
    R.sel = 0; R.fresh = 0u; R.n_nodes = 1u; R.depth = 0u; R.sel_state = root_state; R.ever = 0u;
    if (valid && j == 0) { nodes[0].visits = 1.0f; nodes[0].value = 0.f; nodes[0].prior = 0.f; nodes[0].link = 0u; }
    expand(valid, slab, nodes, pol, R, 0, root_state, j, row0);
}

// Phase A of iteration k >= 1 finishes iteration k - 1.  If somebody selected in it (`any_prev`; a clear word is the reference's `continue`),
// every game that is fresh -- under DIEE_FLAG_REF_QUIRKS (`quirks`) every game, Q14: a stale slot is expanded (a no-op, its node is drained)
// and backpropagated again -- expands sel with the policy row `pol` and backpropagates `value`, same sign at every level, one node per lane:
// `path_node` is lane j's node of root .. sel (read only for j <= R.depth).  A slot that has never selected still holds alpha_mcts.rs:142's 0,
// node 0 of the ONE NodeStore: game 0's root, whoever the slot belongs to; under the quirks it backpropagates the evaluation of that root into
// that root.  Game 0 does so for all of them (`never_prev` of them, `root_value` each, read by game 0's lane 0 only); the others skip their turn.
DIEE_TTT_FN void finish_iteration(bool valid, size_t gi, uint32_t quirks, uint32_t slab, RunNode* nodes, const float* pol, float value, float root_value,
                                  uint32_t any_prev, uint32_t never_prev, int path_node, Row& R, int j, int row0) {
    const bool go = valid && any_prev != 0u && (R.fresh != 0u || quirks != 0u) && (R.ever != 0u || gi == 0);
    const uint32_t link = go ? nodes[R.sel].link : kRunDrained;
    expand(go && (link & kRunDrained) == 0u, slab, nodes, pol, R, R.sel, R.sel_state, j, row0);
    if (go && (uint32_t)j <= R.depth) {                              // backpropagate, simple_mcts.rs:96-103
        RunNode* nd = nodes + path_node;
        float vis = nd->visits + 1.0f, val = nd->value + value;
        if (gi == 0 && j == 0 && quirks != 0u) {                     // slot order: game 0's own first, then the others'
            for (uint32_t i = 0; i < never_prev; ++i) { vis += 1.0f; val += root_value; }
        }
        nd->visits = vis; nd->value = val;
    }
}

// Phase B, alpha_select_leaf_node (alpha_mcts.rs:14-33): the row descends by PUCT from the root to a leaf.  A level is ONE round trip: lane j
// fetches child j whole (16 bytes) and scores it, the choice replays the host's chain `if (!(ub > un)) best = ch` in child order in every lane
// of the row (last of equal maxima, NaN as the reference has it), and the winner's link word comes over with the bpermute that names it; its
// state is the parent's with the best-th empty cell played.  Returns the leaf `cur`, its state and depth `d`, and in lane j <= d the node at
// depth j of root .. cur (`mypath`).  All lanes of the wave come here; a row that is not `valid` stays at the root.
DIEE_TTT_FN void descend(const RunNode* nodes, bool valid, uint32_t root_state, float c, int j, int row0, int& cur, uint32_t& cstate, uint32_t& d,
                         int& mypath) {
    cur = 0; mypath = 0; d = 0u; cstate = root_state;
    uint32_t cfirst, cnc;
    float cvis;
    {
        const u32x4 r = *(const u32x4*)nodes;
        cvis = as_f32(r.x); cfirst = link_first(r.w); cnc = valid ? link_children(r.w) : 0u;
    }
#pragma unroll 1
    for (int lvl = 0; lvl < kPathCap - 1; ++lvl) {
        const bool act = cnc != 0u;
        if (__builtin_amdgcn_ballot_w64(act) == 0) break;            // wave-wide: the lanes stay together for the bpermutes below
        u32x4 ch = u32x4{0u, 0u, 0u, 0u};
        if (act && (uint32_t)j < cnc) ch = *(const u32x4*)(nodes + cfirst + j);
        const float score = puct(as_f32(ch.x), as_f32(ch.y), as_f32(ch.z), __builtin_sqrtf(cvis), c);
        int best = 0;
        float ub = row_getf(score, row0);
#pragma unroll
        for (int jj = 1; jj < 9; ++jj) {                             // Iterator::max_by: the LAST of equal maxima; NaN compares Equal
            const float un = row_getf(score, row0 + jj);
            if ((uint32_t)jj < cnc && !(ub > un)) { best = jj; ub = un; }
        }
        const uint32_t nvis = row_get(ch.x, row0 + best), nlink = row_get(ch.w, row0 + best);
        if (act) {
            cur = (int)cfirst + best; cvis = as_f32(nvis);
            cstate = apply_move(cstate, nth_cell(empty_cells(cstate), (uint32_t)best));
            cfirst = link_first(nlink); cnc = link_children(nlink);
            ++d;
            if ((uint32_t)j == d) mypath = cur;
        }
    }
}

// The end of a selection for a valid row.  A finished game backpropagates +1 / -1 / 0 for the ROOT's player at once (alpha_mcts.rs:157-163),
// one node per lane, fresh = 0, sel untouched; any other leaf becomes sel, fresh = 1.  Returns whether the leaf needs the network: the caller
// then keeps lane j's `mypath` (j <= d) as the path of sel.  (R's fields are set by selects: stores to different fields in the two branches
// get merged into one store through a chosen address, which puts R into scratch.)
DIEE_TTT_FN bool end_selection(RunNode* nodes, uint32_t root_state, int cur, uint32_t cstate, uint32_t d, int mypath, int j, Row& R) {
    R.cnt[kCntSelections] += 1u; R.cnt[kCntDepthSum] += d;
    int winner;
    const bool over = finished(cstate, winner);
    if (over && (uint32_t)j <= d) {
        const int rp = player_of(root_state);
        const float v = winner == rp ? 1.0f : (winner == -rp ? -1.0f : 0.0f);
        RunNode* nd = nodes + mypath;
        nd->visits += 1.0f; nd->value += v;
    }
    R.cnt[kCntTerminalHits] += over ? 1u : 0u; R.fresh = over ? 0u : 1u;
    if (!over) { R.sel = cur; R.sel_state = cstate; R.depth = d; R.ever = 1u; }
    return !over;
}

// The root's row after the last iteration: get_prob_tensor_parallel (utils.rs:42-58), children's visits over their sum in child order.
// Returns lane j's entry of the row (0x7FC00000 for a root without children, 0 for a cell that is no child), `nc` = the root's children,
// `visits` = its visit count.
DIEE_TTT_FN float run_root_row(const RunNode* nodes, bool valid, uint32_t root_state, int j, int row0, uint32_t& nc, float& visits) {
    const u32x4 r = *(const u32x4*)nodes;
    nc = valid ? link_children(r.w) : 0u;
    visits = as_f32(r.x);
    const uint32_t mask = nc ? empty_cells(root_state) : 0u;         // the root's children are its empty cells in ascending order
    const bool mine = j < 9 && ((mask >> j) & 1u) != 0u;
    const float myvis = mine ? nodes[link_first(r.w) + (uint32_t)__builtin_popcount(mask & ((1u << j) - 1u))].visits : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int cidx = 0; cidx < 9; ++cidx) {                           // the row sum over the children in order
        const float v = row_getf(myvis, row0 + cidx);
        if ((mask >> cidx) & 1u) sum += v;
    }
    return nc == 0u ? as_f32(0x7FC00000u) : (mine ? myvis / sum : 0.f);
}

// The diee_stats counters of a workgroup's 16 games, reduced in LDS and added to `counters` once per workgroup.  Called by all 256 threads.
DIEE_TTT_FN void add_counters(uint32_t (&s_cnt)[kB][kCntCount], unsigned long long* counters, bool valid, const Row& R, int tid) {
    if ((tid & 15) == 0) {
#pragma unroll
        for (int i = 0; i < kCntCount; ++i) s_cnt[tid >> 4][i] = valid ? R.cnt[i] : 0u;
    }
    group_barrier();
    if (tid < kCntCount) {
        unsigned long long t = 0;
        for (int g = 0; g < kB; ++g) {
            const unsigned long long v = s_cnt[g][tid];
            t = tid == kCntMaxChildren ? (v > t ? v : t) : t + v;
        }
        if (tid == kCntMaxChildren) __hip_atomic_fetch_max(counters + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_fetch_add(counters + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace ttt
}  // namespace diee
