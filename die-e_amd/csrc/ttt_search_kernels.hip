// ttt_search_kernels.hip -- k_ttt_search: alpha_mcts_parallel for tic-tac-toe (src/mcts/alpha_mcts.rs:91-202; ttt_host.cpp: search) on
// gfx950, ONE launch per iteration with the network inside it.  Reached through option "search" = "device" of a tic-tac-toe ctx
// (ttt_search_device.h); the host search stays the default.  A call is iterations + 1 launches on one stream and the host reads nothing
// in between, so an iteration costs a launch instead of two staging copies, a launch, a synchronise and the host's tree walk.
//
// Work split.  As in k_ttt_net a workgroup of 4 wavefronts owns 16 games for the whole launch and no workgroup waits for another.  For the
//   tree phases a game is a row of 16 lanes (4 games per wave); values cross lanes with ds_bpermute inside the row and a ballot shifted down
//   to the row's 16 bits, never through LDS, which the network owns.
// Tree.  HBM only (a path is at most 10 nodes): RunNode / SearchGame of ttt_search_device.h.  A level of a descent and a backpropagation are
//   ONE round trip each: the path root .. leaf is written down during the descent (SearchGame::path), lane j adds to node path[j].
// The iteration itself is ttt_search_iter_device.h's, shared with k_ttt_search_run; this kernel loads a game's Row from SearchGame, calls the
// pieces and stores the Row back.  Launch k (k = 0 .. iterations), phases divided by workgroup barriers:
//   A, k = 0   evaluate the 16 roots (net_eval), mix the ONE Dirichlet sample x = (1 - eps) p, y = eps noise, x + y (two roundings, then an
//              add), start_search.
//   A, k >= 1  finish_iteration for iteration k - 1: any_selected[k - 1] and never_selected[k - 1] are complete, the launch that wrote them
//              has ended; policy row and value are the ones phase C of that launch stored.
//   B, k < iterations   descend, end_selection; a workgroup in which a game selected contributes one atomic OR to any_selected[k], and the
//              games other than game 0 that have not selected once are added to never_selected[k].
//   C, k < iterations   net_eval on the states of sel of the 16 games, stale ones included (the reference evaluates them too,
//              alpha_mcts.rs:175-186); policy row and value go to SearchGame.  (A slot that has not selected once evaluates its own root
//              where the reference evaluates game 0's: nothing reads that row.)
//   k = iterations   after A: run_root_row, n_children, root_visits, add_counters.
// Everything is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called (ttt_net_device.h says why); all stores are plain C++.
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_device.h"
#include "ttt_search_iter_device.h"

namespace diee {
namespace ttt {

template <bool FIRST>
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_search(SearchParams P) {
    __shared__ NetLds S;
    __shared__ uint32_t s_any, s_never;
    __shared__ uint32_t s_cnt[kB][kCntCount];
    const int tid = threadIdx.x, grp = tid >> 4, j = tid & 15, row0 = tid & 48;      // row0: the first lane of this game's row within its wave
    const size_t board0 = (size_t)blockIdx.x * kB, gi = board0 + grp;
    const bool valid = gi < P.n, last = P.k == P.iterations;
    RunNode* nodes = P.nodes + (valid ? gi : 0) * P.slab;
    SearchGame* G = P.games + (valid ? gi : 0);
    if (tid == 0) { s_any = 0u; s_never = 0u; }

    Row R;
    uint32_t root_state;
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
        root_state = valid ? unpack_root(P.roots + gi) : 0u;
#pragma unroll
        for (int i = 0; i < kCntCount; ++i) R.cnt[i] = 0u;
        if (valid && j == 0) { G->root_state = root_state; G->path[0] = 0; }
        start_search(valid, P.slab, nodes, G->policy, R, root_state, j, row0);
    } else {
        R.sel = G->sel; R.fresh = G->fresh; R.n_nodes = G->n_nodes; R.depth = G->depth; R.sel_state = G->sel_state; R.ever = G->ever;
        R.cnt[kCntExpansions] = G->expansions; R.cnt[kCntChildren] = G->children; R.cnt[kCntMaxChildren] = G->max_children;
        R.cnt[kCntSelections] = G->selections; R.cnt[kCntDepthSum] = G->depth_sum; R.cnt[kCntTerminalHits] = G->terminal_hits;
        root_state = G->root_state;
        const int path_node = (uint32_t)j <= R.depth ? G->path[j] : 0;
        const uint32_t never_prev = gi == 0 && j == 0 && P.quirks != 0u ? P.never_selected[P.k - 1] : 0u;
        finish_iteration(valid, gi, P.quirks, P.slab, nodes, G->policy, G->value, G->root_value, P.any_selected[P.k - 1], never_prev, path_node, R, j,
                         row0);
    }
    group_barrier();

    if (!last) {
        // ---- phase B ---------------------------------------------------------------------------------------------------------------------
        int cur, mypath;
        uint32_t d, cstate;
        descend(nodes, valid, root_state, P.c, j, row0, cur, cstate, d, mypath);
        bool selected = false;
        if (valid) {
            selected = end_selection(nodes, root_state, cur, cstate, d, mypath, j, R);
            if (selected && (uint32_t)j <= d) G->path[j] = mypath;
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

        // ---- phase C ---------------------------------------------------------------------------------------------------------------------
        float pol[9], val;
        net_eval(P.net, S, tid, j < 3 ? grp * 3 + j : -1, net_word(valid, R.sel_state, j), pol, val);
        if (tid < kB && board0 + tid < P.n) {
            SearchGame* g = P.games + board0 + tid;
#pragma unroll
            for (int a = 0; a < 9; ++a) g->policy[a] = pol[a];
            g->value = val;
        }
    } else {
        // ---- the results -----------------------------------------------------------------------------------------------------------------
        uint32_t nc;
        float root_visits;
        const float prob = run_root_row(nodes, valid, root_state, j, row0, nc, root_visits);
        if (valid && j < 9) P.probs[gi * 9 + j] = prob;
        if (valid && j == 0) { P.n_children[gi] = nc; P.root_visits[gi] = root_visits; }
        add_counters(s_cnt, P.counters, valid, R, tid);
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
