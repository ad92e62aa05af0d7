// ttt_search_kernels.hip -- k_ttt_search: alpha_mcts_parallel for tic-tac-toe (src/mcts/alpha_mcts.rs:91-202; ttt_host.cpp: search) on
// gfx950, ONE launch per iteration with the network inside it.  Reached through option "search" = "device" of a tic-tac-toe ctx
// (ttt_search_device.h); the host search stays the default.  A call is iterations + 1 launches on one stream and the host reads nothing
// in between, so an iteration costs a launch instead of two staging copies, a launch, a synchronise and the host's tree walk.
//
// Work split.  As in k_ttt_net a workgroup of 4 wavefronts owns 16 games for the whole launch and no workgroup waits for another.  For the
//   tree phases a game is a row of 16 lanes (4 games per wave): lane j < 9 is child j of the node in hand (selection) or board cell j
//   (expansion, root probabilities).  What a row agrees on (the node in hand, the best child) is kept redundantly in all its lanes; values
//   cross lanes with ds_bpermute inside the row and a ballot shifted down to the row's 16 bits, never through LDS, which the network owns.
// Tree.  HBM only (a path is at most 10 nodes): SearchNode / SearchGame of ttt_search_device.h.  A level of a descent is ONE round trip:
//   lane j fetches child j whole (32 bytes), scores it, and the winner's own child table comes over with the bpermute that names it.
//   A backpropagation is one round trip too: the path root .. leaf is written down during the descent, lane j adds to node path[j].
// Launch k (k = 0 .. iterations), phases divided by workgroup barriers:
//   A, k = 0   evaluate the 16 roots (net_eval), mix the ONE Dirichlet sample x = (1 - eps) p, y = eps noise, x + y (two roundings, then an
//              add), root visits = 1, expand the root.
//   A, k >= 1  finishes iteration k - 1: if any_selected[k - 1] is set (complete: the launch that wrote it has ended), every game that is
//              fresh -- under DIEE_FLAG_REF_QUIRKS every game, Q14: a stale slot is expanded (a no-op, its node is drained) and
//              backpropagated again -- expands sel with the stored policy row and backpropagates the stored value, same sign at every
//              level.  A clear word is the reference's `continue`.  (A slot that has not selected once names node 0 of the reference's one
//              NodeStore, game 0's root: game 0 takes those backpropagations, counted per iteration like the flag: see there.)
//   B, k < iterations   every game descends by PUCT to a leaf.  The arithmetic is the host's ucb() operation for operation (correctly rounded
//              division and square root, no contraction); the nine scores are computed one per lane, the choice replays the host's chain
//              `if (!(ub > un)) best = ch` in child order in every lane of the row (last of equal maxima, NaN as the reference has it).
//              A finished game backpropagates +1 / -1 / 0 for the root's player at once, fresh = 0, sel untouched; any other leaf becomes
//              sel, fresh = 1, and the workgroup contributes one atomic OR to any_selected[k].
//   C, k < iterations   net_eval on the states of sel of the 16 games, stale ones included (the reference evaluates them too), staged
//              straight into the network's cell words; policy row and value go to SearchGame.  (A slot that has not selected once evaluates
//              its own root where the reference evaluates game 0's: nothing reads that row.)
//   k = iterations   after A: root probabilities (children's visits over their sum in child order; 0x7FC00000 for a childless root),
//              n_children, root_visits, and the diee_stats counters reduced in LDS and added once per workgroup.
// Everything is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called (ttt_net_device.h says why); all stores are plain C++.
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_device.h"

namespace diee {
namespace ttt {

namespace {
// Node::alpha_ucb, node.rs:98-112 = ucb() of ttt_host.cpp, f32 in this association (sq = sqrt(visits of the parent))
DIEE_TTT_FN float puct(float n, float val, float prior, float sq, float c) {
    const float q = n == 0.f ? 0.f : val / n;
    const float t = sq / (n + 1.0f);
    const float u = c * t;
    const float w = u * prior;
    return q + w;
}

// what a row of 16 lanes knows about its game during a launch; every field is the same in all 16 lanes
struct Row {
    int32_t sel;
    uint32_t fresh, n_nodes, depth, sel_state, ever, cnt[kCntCount];
};

// turn_policy_to_probs_tensor (utils.rs:74-84) + alpha_expand_tensor (node.rs:157-174) = expand() of ttt_host.cpp, for the rows whose `go`
// is set (all lanes of the wave come here: the ballot is wave-wide).  Lane j is cell j; the policy row is the game's stored one.
DIEE_TTT_FN void expand(bool go, const SearchParams& P, SearchNode* nodes, const SearchGame* G, Row& R, int idx, uint32_t state, uint32_t meta, int j,
                        int row0) {
    const bool legal = go && j < 9 && ((state >> (2 * j)) & 3u) == 0u;
    const uint32_t mask = row_ballot(legal, row0);
    const uint32_t k = (uint32_t)__builtin_popcount(mask);
    if (!go || R.n_nodes + k > P.slab) return;                       // (the slab holds every expansion by construction)
    float sum = 0.f;
#pragma unroll
    for (int cidx = 0; cidx < 9; ++cidx) {                           // ascending cells: the order of expand()'s sum
        const float p = G->policy[cidx];
        if ((mask >> cidx) & 1u) sum += p;
    }
    if (legal) {
        SearchNode* ch = nodes + R.n_nodes + (uint32_t)__builtin_popcount(mask & ((1u << j) - 1u));
        ch->visits = 0.f; ch->value = 0.f; ch->prior = G->policy[j] / sum;
        ch->state = (state | pack_cell(player_of(state), j)) ^ (1u << 18);      // apply_move: the cell takes the player, the player flips
        ch->parent = idx; ch->first_child = -1; ch->meta = (uint32_t)j << 8; ch->pad = 0u;
    }
    if (j == 0) {
        nodes[idx].first_child = k ? (int32_t)R.n_nodes : -1;
        nodes[idx].meta = (meta & 0xFF00u) | k | kMetaDrained;
    }
    R.n_nodes += k;
    R.cnt[kCntExpansions] += 1u; R.cnt[kCntChildren] += k;
    R.cnt[kCntMaxChildren] = k > R.cnt[kCntMaxChildren] ? k : R.cnt[kCntMaxChildren];
}
}  // namespace

template <bool FIRST>
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_search(SearchParams P) {
    __shared__ NetLds S;
    __shared__ uint32_t s_any, s_never;
    __shared__ uint32_t s_cnt[kB][kCntCount];
    const int tid = threadIdx.x, grp = tid >> 4, j = tid & 15, row0 = tid & 48;      // row0: the first lane of this game's row within its wave
    const size_t board0 = (size_t)blockIdx.x * kB, gi = board0 + grp;
    const bool valid = gi < P.n, last = P.k == P.iterations;
    SearchNode* nodes = P.nodes + (valid ? gi : 0) * P.slab;
    SearchGame* G = P.games + (valid ? gi : 0);
    if (tid == 0) { s_any = 0u; s_never = 0u; }

    Row R;
    uint32_t root_state = 0u;
    // ---- phase A ------------------------------------------------------------------------------------------------------------------------
    if (FIRST) {
        uint32_t word = 0u;                                          // a game past n is the empty board, computed and not stored
        if (tid < kB * 3 && board0 + tid / 3 < P.n) word = ((const uint32_t*)P.roots)[(board0 + tid / 3) * 8 + tid % 3];
        float pol[9], val;
        net_eval(P.net, S, tid, tid < kB * 3 ? tid : -1, word, pol, val);
        if (tid < kB && board0 + tid < P.n) {
            SearchGame* g = P.games + board0 + tid;
#pragma unroll
            for (int a = 0; a < 9; ++a) {                            // apply_dirichlet, noise.rs:27-34
                const float x = P.one_minus_eps * pol[a], y = P.eps * P.noise[a];
                g->policy[a] = x + y;
            }
            g->value = val; g->root_value = val;
        }
        group_barrier();
        if (valid) {
            const uint32_t* r = (const uint32_t*)(P.roots + gi);
            const uint32_t w0 = r[0], w1 = r[1], w2 = r[2];
#pragma unroll
            for (int cidx = 0; cidx < 9; ++cidx) {
                const uint32_t w = cidx < 4 ? w0 : cidx < 8 ? w1 : w2;
                root_state |= pack_cell((int)(signed char)(w >> (8 * (cidx & 3))), cidx);
            }
            if ((signed char)(w2 >> 8) > 0) root_state |= 1u << 18;
        }
        R.sel = 0; R.fresh = 0u; R.n_nodes = 1u; R.depth = 0u; R.sel_state = root_state; R.ever = 0u;
#pragma unroll
        for (int i = 0; i < kCntCount; ++i) R.cnt[i] = 0u;
        if (valid && j == 0) {
            nodes[0].visits = 1.0f; nodes[0].value = 0.f; nodes[0].prior = 0.f; nodes[0].state = root_state; nodes[0].parent = -1; nodes[0].pad = 0u;
            G->path[0] = 0;
        }
        expand(valid, P, nodes, G, R, 0, root_state, 0xFF00u, j, row0);
    } else {
        R.sel = G->sel; R.fresh = G->fresh; R.n_nodes = G->n_nodes; R.depth = G->depth; R.sel_state = G->sel_state; R.ever = G->ever;
        R.cnt[kCntExpansions] = G->expansions; R.cnt[kCntChildren] = G->children; R.cnt[kCntMaxChildren] = G->max_children;
        R.cnt[kCntSelections] = G->selections; R.cnt[kCntDepthSum] = G->depth_sum; R.cnt[kCntTerminalHits] = G->terminal_hits;
        root_state = nodes[0].state;
        // A slot that has never selected still holds alpha_mcts.rs:142's 0, node 0 of the ONE NodeStore: game 0's root, whoever the slot
        // belongs to.  Under the quirks it backpropagates the evaluation of that root into that root.  Game 0 does so for all of them:
        // never_selected[k - 1] counts them and is complete like the flag word; the other games skip their turn.
        const bool go = valid && P.any_selected[P.k - 1] != 0u && (R.fresh != 0u || P.quirks != 0u) && (R.ever != 0u || gi == 0);
        const uint32_t meta = go ? nodes[R.sel].meta : kMetaDrained;
        expand(go && (meta & kMetaDrained) == 0u, P, nodes, G, R, R.sel, R.sel_state, meta, j, row0);
        if (go && (uint32_t)j <= R.depth) {                          // backpropagate, simple_mcts.rs:96-103: one node per lane
            SearchNode* nd = nodes + G->path[j];
            float vis = nd->visits + 1.0f, val = nd->value + G->value;
            if (gi == 0 && j == 0 && P.quirks != 0u) {               // slot order: game 0's own first, then the others'
                const uint32_t m = P.never_selected[P.k - 1];
                const float rv = G->root_value;
                for (uint32_t i = 0; i < m; ++i) { vis += 1.0f; val += rv; }
            }
            nd->visits = vis; nd->value = val;
        }
    }
    group_barrier();

    if (!last) {
        // ---- phase B: alpha_select_leaf_node, alpha_mcts.rs:14-33 ------------------------------------------------------------------------
        int cur = 0, mypath = 0;
        uint32_t d = 0u, cstate, cfirst, cnc;
        float cvis;
        {
            const u32x4* p = (const u32x4*)nodes;
            const u32x4 lo = p[0], hi = p[1];
            cvis = as_f32(lo.x); cstate = lo.w; cfirst = hi.y; cnc = valid ? hi.z & 0xFFu : 0u;
        }
#pragma unroll 1
        for (int lvl = 0; lvl < kPathCap - 1; ++lvl) {
            const bool act = cnc != 0u;
            if (__builtin_amdgcn_ballot_w64(act) == 0) break;        // wave-wide: the lanes stay together for the bpermutes below
            u32x4 lo = u32x4{0u, 0u, 0u, 0u}, hi = lo;
            if (act && (uint32_t)j < cnc) {
                const u32x4* p = (const u32x4*)(nodes + cfirst + j);
                lo = p[0]; hi = p[1];
            }
            const float score = puct(as_f32(lo.x), as_f32(lo.y), as_f32(lo.z), __builtin_sqrtf(cvis), P.c);
            int best = 0;
            float ub = row_getf(score, row0);
#pragma unroll
            for (int jj = 1; jj < 9; ++jj) {                         // Iterator::max_by: the LAST of equal maxima; NaN compares Equal
                const float un = row_getf(score, row0 + jj);
                if ((uint32_t)jj < cnc && !(ub > un)) { best = jj; ub = un; }
            }
            const uint32_t nvis = row_get(lo.x, row0 + best), nstate = row_get(lo.w, row0 + best);
            const uint32_t nfirst = row_get(hi.y, row0 + best), nmeta = row_get(hi.z, row0 + best);
            if (act) {
                cur = (int)cfirst + best; cvis = as_f32(nvis); cstate = nstate; cfirst = nfirst; cnc = nmeta & 0xFFu;
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
                if ((uint32_t)j <= d) { SearchNode* nd = nodes + mypath; nd->visits += 1.0f; nd->value += v; }
                R.cnt[kCntTerminalHits] += 1u; R.fresh = 0u;
            } else {
                R.sel = cur; R.sel_state = cstate; R.fresh = 1u; R.depth = d; R.ever = 1u;
                if ((uint32_t)j <= d) G->path[j] = mypath;
                selected = true;
            }
            if (j == 0) {
                G->sel = R.sel; G->fresh = R.fresh; G->n_nodes = R.n_nodes; G->depth = R.depth; G->sel_state = R.sel_state; G->ever = R.ever;
                if (R.ever == 0u && gi != 0) __hip_atomic_fetch_add(&s_never, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                G->expansions = R.cnt[kCntExpansions]; G->children = R.cnt[kCntChildren]; G->max_children = R.cnt[kCntMaxChildren];
                G->selections = R.cnt[kCntSelections]; G->depth_sum = R.cnt[kCntDepthSum]; G->terminal_hits = R.cnt[kCntTerminalHits];
            }
        }
        if (selected && j == 0) s_any = 1u;
        group_barrier();
        if (tid == 0 && s_any != 0u) __hip_atomic_fetch_or(P.any_selected + P.k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0 && s_never != 0u) __hip_atomic_fetch_add(P.never_selected + P.k, s_never, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

        // ---- phase C: the network on the state of sel, stale slots included (alpha_mcts.rs:175-186) -----------------------------------------
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
        if (tid < kB && board0 + tid < P.n) {
            SearchGame* g = P.games + board0 + tid;
#pragma unroll
            for (int a = 0; a < 9; ++a) g->policy[a] = pol[a];
            g->value = val;
        }
    } else {
        // ---- the results: get_prob_tensor_parallel (utils.rs:42-58), the root's counts, the statistics -----------------------------------------
        const u32x4* p = (const u32x4*)nodes;
        const u32x4 lo = p[0], hi = p[1];
        const uint32_t nc = valid ? hi.z & 0xFFu : 0u;
        const uint32_t mask = nc ? empty_cells(root_state) : 0u;     // the root's children are its empty cells in ascending order
        const bool mine = j < 9 && ((mask >> j) & 1u) != 0u;
        const float myvis = mine ? nodes[hi.y + (uint32_t)__builtin_popcount(mask & ((1u << j) - 1u))].visits : 0.f;
        float sum = 0.f;
#pragma unroll
        for (int cidx = 0; cidx < 9; ++cidx) {                       // the row sum over the children in order
            const float v = row_getf(myvis, row0 + cidx);
            if ((mask >> cidx) & 1u) sum += v;
        }
        if (valid && j < 9) P.probs[gi * 9 + j] = nc == 0u ? as_f32(0x7FC00000u) : (mine ? myvis / sum : 0.f);
        if (j == 0) {
            if (valid) { P.n_children[gi] = nc; P.root_visits[gi] = as_f32(lo.x); }
#pragma unroll
            for (int i = 0; i < kCntCount; ++i) s_cnt[grp][i] = valid ? R.cnt[i] : 0u;
        }
        group_barrier();
        if (tid < kCntCount) {
            unsigned long long t = 0;
            for (int g = 0; g < kB; ++g) {
                const unsigned long long v = s_cnt[g][tid];
                t = tid == kCntMaxChildren ? (v > t ? v : t) : t + v;
            }
            if (tid == kCntMaxChildren) __hip_atomic_fetch_max(P.counters + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else __hip_atomic_fetch_add(P.counters + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

void launch_ttt_search(hipStream_t st, const SearchParams& P) {
    if (P.n == 0) return;
    const uint32_t groups = P.n / kB + (P.n % kB != 0);
    if (P.k == 0) hipLaunchKernelGGL(k_ttt_search<true>, dim3(groups), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(k_ttt_search<false>, dim3(groups), dim3(256), 0, st, P);
}

}  // namespace ttt
}  // namespace diee
