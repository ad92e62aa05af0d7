// ttt_search_run_kernels.hip -- k_ttt_search_run: the device search of ttt_search_kernels.hip as ONE launch.  Reached through option
// "search_fused" = "1" of a tic-tac-toe ctx whose "search" is "device" (ttt_search_device.h); k_ttt_search stays the default.  A call of
// k_ttt_search is iterations + 1 dependent launches of ~30 us that carry every game through HBM; here a workgroup keeps its 16 games for
// the whole search and the host enqueues one kernel.
//
// Why one launch is enough.  Without DIEE_FLAG_REF_QUIRKS a game reads nothing of another game: an iteration is finished only for a slot
//   that is fresh, and a fresh slot has selected, so the batch-wide any_selected word is implied.  With the quirks the coupling is two words
//   per iteration, any_selected and never_selected; with at most 16 roots both belong to one workgroup and are LDS words here.  The host
//   sends every other call (quirks and more than 16 roots) to k_ttt_search, and a call of more workgroups than the device has CUs: this
//   kernel's registers hold it to one workgroup per CU, so such a call would run in passes where k_ttt_search co-schedules two (measured).
// Work split.  k_ttt_search's: ceil(n / 16) workgroups of 4 wavefronts, a game is a row of 16 lanes for the tree phases (lane j = child j
//   or cell j), values cross lanes with ds_bpermute and row ballots.  No workgroup waits for another.
// Where a game lives.  Row (sel, fresh, n_nodes, depth, sel_state, ever, the counters) and the path (lane j keeps the node at depth j) stay
//   in registers from the first step to the last; SearchGame is not used.  The policy row and value that an evaluation hands to the next
//   phase A go through s_eval, 16 x 10 floats of LDS.
// Tree.  k_ttt_search's RunNodes, a slab of run_node_bound(iterations) per game.  LDS_TREE: the 16 slabs are dynamic LDS behind the network's
//   62 KB (iterations <= kRunLdsIters); else they lie in HBM (P.nodes).
// Step k = 0 .. iterations (run_steps of ttt_search_run_device.h: k_ttt_selfplay_run of ttt_selfplay_kernels.hip inlines it too), phases
// divided by workgroup barriers, with the meaning of k_ttt_search's launch k and the same pieces of ttt_search_iter_device.h:
//   C  net_eval on the states of sel of the 16 games (k = 0: the roots; the ONE Dirichlet sample is mixed in), policy and value to s_eval.
//      Skipped, uniformly over the workgroup, when none of its games selected in the iteration before: without the quirks nothing reads
//      a stale row, with them (one workgroup) this is the reference's `continue`.
//   A  k = 0: start_search.  k >= 1: finish_iteration, any_selected / never_selected of iteration k - 1 being the workgroup's own words.
//   B  k < iterations: descend, end_selection.  A workgroup that selected ORs any_selected[k] in HBM: the host derives nn_evals from those
//      words after the kernel has ended; the kernel never reads them.
//   after A of step `iterations`: run_root_row, n_children, root_visits, add_counters, as k_ttt_search writes them.
// Everything is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called (ttt_net_device.h says why); all stores are plain C++;
// every loop is bounded by iterations, kPathCap or the 16 games of a workgroup.  The build must show 0 bytes of scratch.
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_device.h"
#include "ttt_search_run_device.h"

namespace diee {
namespace ttt {

static_assert(sizeof(NetLds) == 62400, "kRunLdsBytes of ttt_search_device.h counts on it");

template <bool LDS_TREE>
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_search_run(SearchParams P) {
    __shared__ NetLds S;
    __shared__ float s_eval[kB][10];                                 // a game's last evaluation: policy row, value
    __shared__ uint32_t s_cnt[kB][kCntCount];
    __shared__ uint32_t s_any, s_never;                              // of the iteration in hand: somebody selected | games other than game 0 that never have
    extern __shared__ __attribute__((aligned(16))) unsigned char s_tree[];
    const int tid = threadIdx.x, grp = tid >> 4, j = tid & 15, row0 = tid & 48;      // row0: the first lane of this game's row within its wave
    const size_t board0 = (size_t)blockIdx.x * kB, gi = board0 + grp;
    const bool valid = gi < P.n;
    RunNode* nodes;
    if constexpr (LDS_TREE) nodes = (RunNode*)s_tree + (size_t)grp * P.slab;
    else nodes = P.nodes + (valid ? gi : 0) * P.slab;

    const uint32_t root_state = valid ? unpack_root(P.roots + gi) : 0u;      // a game past n is the empty board, computed and not stored
    Row R;
#pragma unroll
    for (int i = 0; i < kCntCount; ++i) R.cnt[i] = 0u;
    run_steps(P, P.noise, P.any_selected, S, s_eval, s_any, s_never, nodes, valid, gi, root_state, tid, R);

    // ---- the results ------------------------------------------------------------------------------------------------------------------------
    uint32_t nc;
    float root_visits;
    const float prob = run_root_row(nodes, valid, root_state, j, row0, nc, root_visits);
    if (valid && j < 9) P.probs[gi * 9 + j] = prob;
    if (valid && j == 0) { P.n_children[gi] = nc; P.root_visits[gi] = root_visits; }
    add_counters(s_cnt, P.counters, valid, R, tid);
}

hipError_t launch_ttt_search_run(hipStream_t st, const SearchParams& P, bool lds_tree, bool first) {
    if (P.n == 0) return hipSuccess;
    const uint32_t groups = P.n / kB + (P.n % kB != 0);
    if (!lds_tree) {
        hipLaunchKernelGGL(k_ttt_search_run<false>, dim3(groups), dim3(256), 0, st, P);
        return hipGetLastError();
    }
    if (first) {                                                     // LDS beyond the static 64 KB has to be asked for
        const hipError_t e = hipFuncSetAttribute((const void*)k_ttt_search_run<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLdsBytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ttt_search_run<true>, dim3(groups), dim3(256), (size_t)kB * P.slab * sizeof(RunNode), st, P);
    return hipGetLastError();
}

}  // namespace ttt
}  // namespace diee
