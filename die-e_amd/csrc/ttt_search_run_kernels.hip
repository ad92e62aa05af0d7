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
// Tree.  RunNode, 16 bytes: visits, value, prior and one link word; a level of a descent is one 16-byte load per lane, and the child's state
//   is derived: child j is the j-th empty cell of the parent's state.  A game's slab is run_node_bound(iterations) nodes.  LDS_TREE: the 16
//   slabs are dynamic LDS behind the network's 62 KB (iterations <= kRunLdsIters); else they lie in HBM (P.nodes).
// Step k = 0 .. iterations, phases divided by workgroup barriers, with the meaning of k_ttt_search's launch k:
//   C  net_eval on the states of sel of the 16 games (k = 0: the roots; the ONE Dirichlet sample is mixed in), policy and value to s_eval.
//      Skipped, uniformly over the workgroup, when none of its games selected in the iteration before: without the quirks nothing reads
//      a stale row, with them (one workgroup) this is the reference's `continue`.
//   A  k = 0: root visits = 1, expand the root.  k >= 1: finish iteration k - 1 as k_ttt_search does, any_selected / never_selected of that
//      iteration being the workgroup's own words.
//   B  k < iterations: descend by PUCT (puct() and the chain `if (!(ub > un))` of k_ttt_search, operation for operation), backpropagate
//      a finished game at once, else the leaf becomes sel.  A workgroup that selected ORs any_selected[k] in HBM: the host derives nn_evals
//      from those words after the kernel has ended; the kernel never reads them.
//   after A of step `iterations`: root probabilities, n_children, root_visits, the counters, as k_ttt_search writes them.
// Everything is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called (ttt_net_device.h says why); all stores are plain C++;
// every loop is bounded by iterations, kPathCap or the 16 games of a workgroup.  The build must show 0 bytes of scratch.
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_device.h"

namespace diee {
namespace ttt {

namespace {
static_assert(sizeof(NetLds) == 62400, "kRunLdsBytes of ttt_search_device.h counts on it");

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
}  // namespace

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
    else nodes = (RunNode*)P.nodes + (valid ? gi : 0) * P.slab;
    if (tid == 0) { s_any = 0u; s_never = 0u; }

    uint32_t root_state = 0u;                                        // a game past n is the empty board, computed and not stored
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
    Row R;
    R.sel = 0; R.fresh = 0u; R.n_nodes = 1u; R.depth = 0u; R.sel_state = root_state; R.ever = 0u;
#pragma unroll
    for (int i = 0; i < kCntCount; ++i) R.cnt[i] = 0u;
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
                        const float x = P.one_minus_eps * pol[a], y = P.eps * P.noise[a];
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
        if (tid == 0 && any_prev != 0u) __hip_atomic_fetch_or(P.any_selected + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // ---- the results: get_prob_tensor_parallel (utils.rs:42-58), the root's counts, the statistics -------------------------------------------------
    const u32x4 r = *(const u32x4*)nodes;
    const uint32_t nc = valid ? link_children(r.w) : 0u;
    const uint32_t mask = nc ? empty_cells(root_state) : 0u;         // the root's children are its empty cells in ascending order
    const bool mine = j < 9 && ((mask >> j) & 1u) != 0u;
    const float myvis = mine ? nodes[link_first(r.w) + (uint32_t)__builtin_popcount(mask & ((1u << j) - 1u))].visits : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int cidx = 0; cidx < 9; ++cidx) {                           // the row sum over the children in order
        const float v = row_getf(myvis, row0 + cidx);
        if ((mask >> cidx) & 1u) sum += v;
    }
    if (valid && j < 9) P.probs[gi * 9 + j] = nc == 0u ? as_f32(0x7FC00000u) : (mine ? myvis / sum : 0.f);
    if (j == 0) {
        if (valid) { P.n_children[gi] = nc; P.root_visits[gi] = as_f32(r.x); }
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
