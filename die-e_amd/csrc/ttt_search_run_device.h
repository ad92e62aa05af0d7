// ttt_search_run_device.h -- the body of k_ttt_search_run (ttt_search_run_kernels.hip, where the design is described) as a device function:
// run_steps is steps k = 0 .. iterations of a workgroup's 16 games, out of the pieces of ttt_search_iter_device.h (whose run_root_row gives the
// root's row afterwards).  k_ttt_search_run inlines it once per launch, k_ttt_selfplay_run (ttt_selfplay_kernels.hip) once per move-step: both
// kernels execute the same statements, so a game's search is the same bits in either.  Everything is DIEE_TTT_NO_PK_F32 and nothing but
// builtins (ttt_net_device.h says why).
#pragma once
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_device.h"
#include "ttt_search_iter_device.h"

namespace diee {
namespace ttt {

// Steps k = 0 .. P.iterations of the search of a workgroup's 16 games (phases C, A, B of ttt_search_run_kernels.hip), called by all 256
// threads.  This row's game is number `gi` of the call, starts at `root_state` and keeps its tree in `nodes`; a row that is not `valid`
// takes part in the evaluations and the barriers and stores nothing.  `noise`: the Dirichlet sample of this search; `any_selected`:
// its P.iterations words in HBM.  R's search fields are set here, R.cnt is added to.  s_any / s_never are the workgroup's two words of
// the iteration in hand; on return every thread has passed a barrier behind the last store to the trees.
DIEE_TTT_FN void run_steps(const SearchParams& P, const float* noise, uint32_t* any_selected, NetLds& S, float (&s_eval)[kB][10], uint32_t& s_any,
                           uint32_t& s_never, RunNode* nodes, bool valid, size_t gi, uint32_t root_state, int tid, Row& R) {
    const int grp = tid >> 4, j = tid & 15, row0 = tid & 48;          // row0: the first lane of this game's row within its wave
    if (tid == 0) { s_any = 0u; s_never = 0u; }
    R.sel_state = root_state;                                        // step 0 evaluates the root
    int path = 0;                                                    // lane j: the node at depth j of root .. sel
    float root_value = 0.f;                                          // thread b < 16: the evaluation of board b's root
    uint32_t any_prev = 1u, never_prev = 0u;                         // s_any, s_never of the iteration before; step 0 evaluates the roots

#pragma unroll 1
    for (uint32_t k = 0;; ++k) {
        // ---- phase C: the network on the state of sel, stale slots included (alpha_mcts.rs:175-186); k = 0: sel is the root ---------------------
        if (any_prev != 0u) {
            float pol[9], val;
            net_eval(P.net, S, tid, j < 3 ? grp * 3 + j : -1, net_word(valid, R.sel_state, j), pol, val);
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
        if (k == 0) start_search(valid, P.slab, nodes, s_eval[grp], R, root_state, j, row0);
        else finish_iteration(valid, gi, P.quirks, P.slab, nodes, s_eval[grp], s_eval[grp][9], root_value, any_prev, never_prev, path, R, j, row0);
        group_barrier();
        if (k == P.iterations) break;

        // ---- phase B ------------------------------------------------------------------------------------------------------------------------
        int cur, mypath;
        uint32_t d, cstate;
        descend(nodes, valid, root_state, P.c, j, row0, cur, cstate, d, mypath);
        bool selected = false;
        if (valid) {
            selected = end_selection(nodes, root_state, cur, cstate, d, mypath, j, R);
            if (selected && (uint32_t)j <= d) path = mypath;
            if (j == 0 && R.ever == 0u && gi != 0) __hip_atomic_fetch_add(&s_never, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (selected && j == 0) s_any = 1u;
        group_barrier();
        any_prev = s_any; never_prev = s_never;
        if (tid == 0 && any_prev != 0u) __hip_atomic_fetch_or(any_selected + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace ttt
}  // namespace diee
