// ttt_arena_run_kernels.hip -- k_ttt_arena_run: a whole tic-tac-toe arena call (play::<TicTacToe>, versus.rs:160-318, as Engine::arena of
// ttt_host.cpp restates it) as ONE search-and-play launch.  Reached through diee_ttt_arena while the hosting ctx's "search" is "device" and
// its "search_fused" is "2" (ttt_arena_device.h), for Model and Random players without DIEE_FLAG_REF_QUIRKS; the round loop of
// ttt_arena_device.cpp (a split, two searches and two moves per round, a synchronise in between) stays the path of every other call.
//
// Why one launch is enough.  Without the quirks a game reads nothing of another: the search is per game (ttt_search_run_kernels.hip), the
//   network is row-independent, and the one thing the games of a search share, its Dirichlet sample, is drawn by the host from
//   (seed, 2 * round + side) before anything runs: the eighteen rows come with the kernel's arguments.  Every live game takes exactly one
//   turn per round (a skipped turn flips the player too), so the side of game i in round r is (i >= n / 2) ^ (r & 1): nothing has to be
//   split or compacted.  A game without skipped turns ends within nine rounds; the host replays a call that needs more on the round loop.
// Work split.  The family's: workgroups of 4 wavefronts, a game is a row of 16 lanes, lane j < 9 is cell j, values cross lanes with
//   ds_bpermute and row ballots.  No workgroup waits for another.  The two halves of the call are mapped separately, ceil(h / 16) +
//   ceil((n - h) / 16) workgroups with h = n / 2, so a workgroup's 16 games are all on ONE side in any round: the network (p1's or p2's
//   packed weights) and the agent are workgroup-uniform, and the workgroups of the two sides run side by side where the round loop runs
//   the sides in turn.  A workgroup keeps its games from the empty board to their retirement.
// Round r = 0 .. rounds - 1, side = half ^ (r & 1):
//   search  Model: run_steps of ttt_search_run_device.h, the statements k_ttt_search_run executes, on the 16 games' current states over the
//           side's NetParams with noise row 2 r + side; the tree (LDS behind the network's 62 KB up to kRunLdsIters iterations, HBM above)
//           is built anew; then run_root_row.  A game that has retired or lies outside its half is an inert row.  Random: no search and no
//           evaluation at all.  A workgroup adds its live games to live[2 r + side] and ORs any_selected[2 r + side][k] for the host's
//           statistics; the kernel reads neither.
//   move    model_move / random_move and play_turn of ttt_arena_move_device.h, the statements k_ttt_arena_move executes, with the uniform of
//           (seed, game, r, kTagSample, 0); a retiring game stores winner, round and side.
//   totals  the turn's counts and the search's counters are reduced over the 16 rows (in NetLds::head: the network is done with it) into
//           the workgroup's two per-player blocks in LDS.
//   exit    a workgroup whose games have all retired leaves the loop.
// Across rounds a game is two words of LDS (state word, live bit), not registers: the search sits at 256 VGPRs.  After the loop a workgroup
//   stores its games' states and adds its totals and the games it leaves alive to HBM once.
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), LDS_TREE false | true:
//   256 | 256 VGPRs, 71 | 66 AGPRs, 106 SGPRs (16 | 17 spilled to VGPR lanes), 0 bytes of scratch, 63272 | 63280 bytes of static LDS, one
//   wave per SIMD: one workgroup per CU, as k_ttt_search_run and k_ttt_selfplay_run.
// draw_uniform and det_powf are bg_device.h's own, the functions the host path calls (two real calls, as in ttt_arena_kernels.hip); everything
// else is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called; all stores are plain C++.
#include <hip/hip_runtime.h>

#include "bg_device.h"
#include "ttt_arena_device.h"
#include "ttt_arena_move_device.h"
#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_run_device.h"

namespace diee {
namespace ttt {

namespace {
// a turn's counts, then the search's counters (ttt_search_device.h): a workgroup's totals of one player
enum { kArPlies = kCntCount, kArMoves, kArRetired, kArWins1, kArWins2, kArDraws, kArCount };
enum { kGwState, kGwLive, kGwCount };
// NetLds, s_eval, the two words of the iteration, the games and the totals: within the 1280 bytes kRunLdsBytes leaves beside the network and the tree
static_assert(sizeof(NetLds) == 62400 && kB * 10 * 4 + 8 + kB * kGwCount * 4 + 2 * kArCount * 4 <= 1280, "kRunLdsBytes of ttt_search_device.h counts on it");
static_assert(kB * kArCount <= kB * kHeadFloats, "the reduction of a round borrows NetLds::head");
static_assert(kArCount <= 64, "a thread per total");
}  // namespace

template <bool LDS_TREE>
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_arena_run(ArParams P) {
    __shared__ NetLds S;
    __shared__ float s_eval[kB][10];                                 // a game's last evaluation: policy row, value
    __shared__ uint32_t s_any, s_never;                              // run_steps' words of the iteration in hand
    __shared__ uint32_t s_game[kB][kGwCount];                        // what a game carries from round to round
    __shared__ uint32_t s_tot[2][kArCount];                          // the workgroup's totals per player
    extern __shared__ __attribute__((aligned(16))) unsigned char s_tree[];
    const int tid = threadIdx.x, grp = tid >> 4, j = tid & 15, row0 = tid & 48;
    const uint32_t h = P.sp.n / 2u, groups0 = (h + (uint32_t)kB - 1u) / (uint32_t)kB;
    const uint32_t half = blockIdx.x < groups0 ? 0u : 1u;            // :172-174: the second half starts after a skip_turn, side 1 to move
    const uint32_t g = half ? h + (blockIdx.x - groups0) * (uint32_t)kB + (uint32_t)grp : blockIdx.x * (uint32_t)kB + (uint32_t)grp;
    const bool valid = g < (half ? P.sp.n : h);
    RunNode* nodes;
    if constexpr (LDS_TREE) nodes = (RunNode*)s_tree + (size_t)grp * P.sp.slab;
    else nodes = P.sp.nodes + (size_t)(valid ? g : 0u) * P.sp.slab;

    if (j == 0) {                                                    // TicTacToe::new, mod.rs:28-30
        s_game[grp][kGwState] = half << 18; s_game[grp][kGwLive] = valid ? 1u : 0u;
        if (valid) { P.retired_round[g] = kArenaNone; P.winner[g] = 0; P.retired_side[g] = -1; }
    }
    if (tid < 2 * kArCount) s_tot[tid / kArCount][tid % kArCount] = 0u;
    uint32_t* red = (uint32_t*)S.head;
    Row R;
    group_barrier();

#pragma unroll 1
    for (uint32_t r = 0; r < P.rounds; ++r) {                        // versus.rs:191
        uint32_t n_live = 0u;
#pragma unroll
        for (int b = 0; b < kB; ++b) n_live += s_game[b][kGwLive];
        if (n_live == 0u) break;                                     // the same in every thread
        const uint32_t side = half ^ (r & 1u), step = 2u * r + side;
        if (tid == 0) __hip_atomic_fetch_add(P.head->live + step, n_live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t st = s_game[grp][kGwState];
        const bool live = s_game[grp][kGwLive] != 0u;
#pragma unroll
        for (int i = 0; i < kCntCount; ++i) R.cnt[i] = 0u;

        // ---- get_actions_for_player, :270-318 -------------------------------------------------------------------------------------------
        int move;
        if (P.agents[side] == DIEE_AGENT_MODEL) {                    // a fresh tree every search, the Dirichlet sample of (seed, step)
            SearchParams Q = P.sp;
            Q.net = side ? P.nets[1] : P.nets[0];
            run_steps(Q, P.noise[step], P.any_selected + (size_t)step * P.sp.iterations, S, s_eval, s_any, s_never, nodes, live, g, st, tid, R);
            uint32_t nc;
            float root_visits;
            const float prob = run_root_row(nodes, live, st, j, row0, nc, root_visits);
            move = model_move(prob, nc, P.inv_t, draw_uniform(P.seed, g, r, kTagSample, 0u), row0);
        } else {
            move = random_move(st, draw_uniform(P.seed, g, r, kTagSample, 0u), j, row0);
        }

        // ---- the body of play()'s loop over the side's games, :220-266 ----------------------------------------------------------------------
        if (j == 0) {
            uint32_t cnt[kArCount];
#pragma unroll
            for (int i = 0; i < kArCount; ++i) cnt[i] = i < kCntCount ? R.cnt[i] : 0u;
            if (live) {
                bool moved, retired;
                int w;
                s_game[grp][kGwState] = play_turn(st, move, r, P.round_limit, moved, retired, w);
                cnt[kArPlies] = 1u; cnt[kArMoves] = moved ? 1u : 0u;
                if (retired) {
                    P.winner[g] = (int8_t)w; P.retired_round[g] = r; P.retired_side[g] = (int8_t)side;
                    s_game[grp][kGwLive] = 0u;
                    cnt[kArRetired] = 1u; cnt[kArWins1] = w < 0 ? 1u : 0u; cnt[kArWins2] = w > 0 ? 1u : 0u; cnt[kArDraws] = w == 0 ? 1u : 0u;
                }
            }
#pragma unroll
            for (int i = 0; i < kArCount; ++i) red[grp * kArCount + i] = cnt[i];
        }
        group_barrier();
        if (tid < kArCount) {
            uint32_t t = 0u;
            for (int b = 0; b < kB; ++b) {
                const uint32_t v = red[b * kArCount + tid];
                t = tid == kCntMaxChildren ? (v > t ? v : t) : t + v;
            }
            const uint32_t was = s_tot[side][tid];
            s_tot[side][tid] = tid == kCntMaxChildren ? (t > was ? t : was) : was + t;
        }
        group_barrier();                                             // (red and the games are read before the next round writes them)
    }

    // ---- what the call leaves: the games' states, the totals and the games left alive, once per workgroup ----------------------------------
    if (valid && j == 0) P.state[g] = s_game[grp][kGwState];
    if (tid == 0) {
        uint32_t alive = 0u;
        for (int b = 0; b < kB; ++b) alive += s_game[b][kGwLive];
        if (alive) __hip_atomic_fetch_add(&P.head->alive, alive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < 2 * kArCount) {
        const int s = tid / kArCount, i = tid % kArCount;
        const unsigned long long v = s_tot[s][i];
        unsigned long long* mine = P.head->totals + (size_t)s * kTaPlayerWords;
        unsigned long long* to;
        switch (i) {
            case kCntExpansions: to = mine + kTaExpansions; break;
            case kCntChildren: to = mine + kTaChildren; break;
            case kCntMaxChildren: to = mine + kTaMaxChildren; break;
            case kCntSelections: to = mine + kTaSelections; break;
            case kCntDepthSum: to = mine + kTaDepthSum; break;
            case kCntTerminalHits: to = mine + kTaTerminal; break;
            case kArPlies: to = mine + kTaPlies; break;
            case kArMoves: to = mine + kTaMoves; break;
            case kArRetired: to = mine + kTaRetired; break;
            case kArWins1: to = P.head->totals + kTaWins1; break;
            case kArWins2: to = P.head->totals + kTaWins2; break;
            default: to = P.head->totals + kTaDraws; break;
        }
        if (i == kCntMaxChildren) __hip_atomic_fetch_max(to, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (v) __hip_atomic_fetch_add(to, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

hipError_t launch_ttt_arena_run(hipStream_t st, const ArParams& P, bool lds_tree, bool first) {
    if (P.sp.n == 0) return hipSuccess;
    const uint32_t groups = arena_run_groups(P.sp.n);
    if (!lds_tree) {
        hipLaunchKernelGGL(k_ttt_arena_run<false>, dim3(groups), dim3(256), 0, st, P);
        return hipGetLastError();
    }
    if (first) {                                                     // LDS beyond the static 64 KB has to be asked for
        const hipError_t e = hipFuncSetAttribute((const void*)k_ttt_arena_run<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLdsBytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ttt_arena_run<true>, dim3(groups), dim3(256), (size_t)kB * P.sp.slab * sizeof(RunNode), st, P);
    return hipGetLastError();
}

}  // namespace ttt
}  // namespace diee
