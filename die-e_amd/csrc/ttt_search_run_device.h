// ttt_search_run_device.h -- the body of k_ttt_search_run (ttt_search_run_kernels.hip, where the design is described) as device functions:
// run_steps is steps k = 0 .. iterations of a workgroup's 16 games, run_root_row the root's row afterwards.  k_ttt_search_run inlines them
// once per launch, k_ttt_selfplay_run (ttt_selfplay_kernels.hip) once per move-step: both kernels execute the same statements, so a game's
// search is the same bits in either.  Everything is DIEE_TTT_NO_PK_F32 and nothing but builtins (ttt_net_device.h says why).
#pragma once
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_device.h"

namespace diee {
namespace ttt {

// Node::alpha_ucb, node.rs:98-112 = ucb() of ttt_host.cpp = puct() of ttt_search_kernels.hip
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
    uint32_t fresh, n_nodes, depth, sel_state, ever, cnt[kCntCount];
};

DIEE_TTT_FN uint32_t link_first(uint32_t link) { return link & 0xFFFFu; }
DIEE_TTT_FN uint32_t link_children(uint32_t link) { return (link >> 16) & 0xFu; }
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

// expand() of ttt_search_kernels.hip on RunNodes, for the rows whose `go` is set (all lanes of the wave come here: the ballot is
// wave-wide).  Lane j is cell j; `pol` is the game's row of s_eval.
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
    if (j == 0) nodes[idx].link = (k ? R.n_nodes : 0u) | (k << 16) | kRunDrained;
    R.n_nodes += k;
    R.cnt[kCntExpansions] += 1u; R.cnt[kCntChildren] += k;
    R.cnt[kCntMaxChildren] = k > R.cnt[kCntMaxChildren] ? k : R.cnt[kCntMaxChildren];
}

// Steps k = 0 .. P.iterations of the search of a workgroup's 16 games (phases C, A, B of ttt_search_run_kernels.hip), called by all 256
// threads.  This row's game is number `gi` of the call, starts at `root_state` and keeps its tree in `nodes`; a row that is not `valid`
// takes part in the evaluations and the barriers and stores nothing.  `noise`: the Dirichlet sample of this search; `any_selected`:
// its P.iterations words in HBM.  R's search fields are set here, R.cnt is added to.  s_any / s_never are the workgroup's two words of
// the iteration in hand; on return every thread has passed a barrier behind the last store to the trees.
DIEE_TTT_FN void run_steps(const SearchParams& P, const float* noise, uint32_t* any_selected, NetLds& S, float (&s_eval)[kB][10], uint32_t& s_any,
                           uint32_t& s_never, RunNode* nodes, bool valid, size_t gi, uint32_t root_state, int tid, Row& R) {
    const int grp = tid >> 4, j = tid & 15, row0 = tid & 48;          // row0: the first lane of this game's row within its wave
    if (tid == 0) { s_any = 0u; s_never = 0u; }
    R.sel = 0; R.fresh = 0u; R.n_nodes = 1u; R.depth = 0u; R.sel_state = root_state; R.ever = 0u;
    int path = 0;                                                    // lane j: the node at depth j of root .. sel
    float root_value = 0.f;                                          // thread b < 16: the evaluation of board b's root
    uint32_t any_prev = 1u, never_prev = 0u;                         // s_any, s_never of the iteration before; step 0 evaluates the roots

#pragma unroll 1
    for (uint32_t k = 0;; ++k) {
        // ---- phase C: the network on the state of sel, stale slots included (alpha_mcts.rs:175-186); k = 0: sel is the root ---------------------
        if (any_prev != 0u) {
            uint32_t word = 0u;
            if (valid && j < 3) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int cidx = 4 * j + b;
                    const int v = cidx < 9 ? cell_of(R.sel_state, cidx < 9 ? cidx : 0) : cidx == 9 ? player_of(R.sel_state) : 0;
                    word |= ((uint32_t)v & 0xFFu) << (8 * b);
                }
            }
            float pol[9], val;
            net_eval(P.net, S, tid, j < 3 ? grp * 3 + j : -1, word, pol, val);
            if (tid < kB) {
                if (k == 0) {
#pragma unroll
                    for (int a = 0; a < 9; ++a) {                    // apply_dirichlet, noise.rs:27-34
                        const float x = P.one_minus_eps * pol[a], y = P.eps * noise[a];
                        pol[a] = x + y;
                    }
                    root_value = val;
                }
#pragma unroll
                for (int a = 0; a < 9; ++a) s_eval[tid][a] = pol[a];
                s_eval[tid][9] = val;
            }
        }
        group_barrier();

        // ---- phase A ------------------------------------------------------------------------------------------------------------------------
        if (tid == 0) { s_any = 0u; s_never = 0u; }                  // (everybody has read them: a barrier ago)
        if (k == 0) {
            if (valid && j == 0) { nodes[0].visits = 1.0f; nodes[0].value = 0.f; nodes[0].prior = 0.f; nodes[0].link = 0u; }
            expand(valid, P.slab, nodes, s_eval[grp], R, 0, root_state, j, row0);
        } else {
            // k_ttt_search's phase A for launch k.  A slot that has never selected names game 0's root: under the quirks game 0 backpropagates
            // for all of them (never_prev of them), the other games skip their turn.
            const bool go = valid && any_prev != 0u && (R.fresh != 0u || P.quirks != 0u) && (R.ever != 0u || gi == 0);
            const uint32_t link = go ? nodes[R.sel].link : kRunDrained;
            expand(go && (link & kRunDrained) == 0u, P.slab, nodes, s_eval[grp], R, R.sel, R.sel_state, j, row0);
            if (go && (uint32_t)j <= R.depth) {                      // backpropagate, simple_mcts.rs:96-103: one node per lane
                RunNode* nd = nodes + path;
                float vis = nd->visits + 1.0f, val = nd->value + s_eval[grp][9];
                if (gi == 0 && j == 0 && P.quirks != 0u) {           // slot order: game 0's own first, then the others'  (thread 0: root_value is game 0's)
                    for (uint32_t i = 0; i < never_prev; ++i) { vis += 1.0f; val += root_value; }
                }
                nd->visits = vis; nd->value = val;
            }
        }
        group_barrier();
        if (k == P.iterations) break;

        // ---- phase B: alpha_select_leaf_node, alpha_mcts.rs:14-33 ------------------------------------------------------------------------
        int cur = 0, mypath = 0;
        uint32_t d = 0u, cstate = root_state, cfirst, cnc;
        float cvis;
        {
            const u32x4 r = *(const u32x4*)nodes;
            cvis = as_f32(r.x); cfirst = link_first(r.w); cnc = valid ? link_children(r.w) : 0u;
        }
#pragma unroll 1
        for (int lvl = 0; lvl < kPathCap - 1; ++lvl) {
            const bool act = cnc != 0u;
            if (__builtin_amdgcn_ballot_w64(act) == 0) break;        // wave-wide: the lanes stay together for the bpermutes below
            u32x4 ch = u32x4{0u, 0u, 0u, 0u};
            if (act && (uint32_t)j < cnc) ch = *(const u32x4*)(nodes + cfirst + j);
            const float score = puct(as_f32(ch.x), as_f32(ch.y), as_f32(ch.z), __builtin_sqrtf(cvis), P.c);
            int best = 0;
            float ub = row_getf(score, row0);
#pragma unroll
            for (int jj = 1; jj < 9; ++jj) {                         // Iterator::max_by: the LAST of equal maxima; NaN compares Equal
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
        bool selected = false;
        if (valid) {
            R.cnt[kCntSelections] += 1u; R.cnt[kCntDepthSum] += d;
            int winner;
            if (finished(cstate, winner)) {                          // alpha_mcts.rs:157-163: +-1 for the ROOT's player
                const int rp = player_of(root_state);
                const float v = winner == rp ? 1.0f : (winner == -rp ? -1.0f : 0.0f);
                if ((uint32_t)j <= d) { RunNode* nd = nodes + mypath; nd->visits += 1.0f; nd->value += v; }
                R.cnt[kCntTerminalHits] += 1u; R.fresh = 0u;
            } else {
                R.sel = cur; R.sel_state = cstate; R.fresh = 1u; R.depth = d; R.ever = 1u;
                if ((uint32_t)j <= d) path = mypath;
                selected = true;
            }
            if (j == 0 && R.ever == 0u && gi != 0) __hip_atomic_fetch_add(&s_never, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (selected && j == 0) s_any = 1u;
        group_barrier();
        any_prev = s_any; never_prev = s_never;
        if (tid == 0 && any_prev != 0u) __hip_atomic_fetch_or(any_selected + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The root's row after run_steps: get_prob_tensor_parallel (utils.rs:42-58).  Returns lane j's entry of the row (NaN for a root without
// children, 0 for a cell that is no child), `nc` = the root's children, `visits` = its visit count.
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

}  // namespace ttt
}  // namespace diee
