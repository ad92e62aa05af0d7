// ttt_selfplay_kernels.hip -- k_ttt_selfplay_run: a whole tic-tac-toe self-play call (self_play_parallel, alpha_parallel.rs:101-231, as
// Engine::self_play of ttt_host.cpp restates it) as ONE search-and-play launch, and the two kernels that deliver its records.  Reached through
// option "search_fused" = "2" of a ctx whose "search" is "device" (ttt_selfplay_device.h), for calls without DIEE_FLAG_REF_QUIRKS; the host loop
// over one search per move-step stays the path of every other call.
//
// Why one launch is enough.  Without the quirks a game reads nothing of another: the search is per game (ttt_search_run_kernels.hip), the
//   network is row-independent, and the one thing the games of a move-step share, its Dirichlet sample, is drawn by the host from
//   (seed, move-step) before anything runs: the nine rows come with the kernel's arguments.  A game ends within nine move-steps.
// Work split.  k_ttt_search_run's: ceil(n_games / 16) workgroups of 4 wavefronts, a game is a row of 16 lanes, lane j < 9 is cell j, values
//   cross lanes with ds_bpermute and row ballots.  No workgroup waits for another.  A workgroup keeps its 16 games for the whole call.
// Move-step s = 0 .. steps - 1, three parts:
//   search  run_steps of ttt_search_run_device.h, the statements k_ttt_search_run executes, on the 16 games' current states with noise row
//           s; the tree (LDS behind the network's 62 KB up to kRunLdsIters iterations, HBM above) is built anew.  A game that has retired
//           or lies past n_games is an inert row.  A workgroup adds its live games to live[s] and ORs any_selected[s][k] for the host's
//           statistics; the kernel reads neither.
//   play    the body of self_play's loop for the row's game, statement by statement: the round-limit flush (outcomes 0, no `continue`); a root
//           without children skips its turn; lane j raises probs[j] to 1 / temperature (det_powf, not renormalised), every lane replays
//           weighted_select (weighted_pick of ttt_rules_device.h, shared with k_ttt_arena_move) with the uniform of (seed, game id, round,
//           kTagSample, 0); the fragment (player, raised row, planes) goes to the game's area in HBM, [game][9]; the move is checked and
//           applied, the board judged, a finished game flushes unless the round limit already did, and retires.  A flush is one SpGame: the
//           move-step, the fragments delivered, zero outcomes or the winner.
//   exit    a workgroup whose games have all retired leaves the loop.
// Across move-steps a game is seven words of LDS (state word, round, live bit, fragments, three counts), not registers: the search sits at
//   256 VGPRs.  The build must show 0 bytes of scratch and one workgroup per CU, as for k_ttt_search_run.
// Delivery.  The host loop's order is: flushes by move-step, within a move-step by ascending game, within a game in play order; a game flushes
//   at most once.  k_ttt_sp_offsets, ONE workgroup of 1024: per move-step a thread takes a game, the fragments of the games that flushed in
//   it (0 .. 9: four bit planes) are prefix-summed with wave ballots and an LDS prefix over the waves, the carry runs on over chunks and
//   move-steps: each flushed game's first row and the total nf.  k_ttt_sp_gather: 64 lanes per game copy its fragments to the compact
//   arrays and compute the outcomes (alpha_parallel.rs:216-217).  The host copies nf rows.
// draw_uniform and det_powf are bg_device.h's own, the functions the host path calls (two real calls, as in ttt_arena_kernels.hip); everything
// else is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called; all stores are plain C++.
#include <hip/hip_runtime.h>

#include "bg_device.h"
#include "ttt_net_device.h"
#include "ttt_rules_device.h"
#include "ttt_search_run_device.h"
#include "ttt_selfplay_device.h"

namespace diee {
namespace ttt {

namespace {
enum { kGwState, kGwRound, kGwLive, kGwFrags, kGwPlies, kGwGames, kGwIllegal, kGwCount };
// NetLds, s_eval, the two words of the iteration and the games: within the 1280 bytes kRunLdsBytes leaves beside the network and the tree
static_assert(sizeof(NetLds) == 62400 && kB * 10 * 4 + 8 + kB * kGwCount * 4 <= 1280, "kRunLdsBytes of ttt_search_device.h counts on it");
static_assert(kB * kSpCntCount <= kB * kHeadFloats, "the last reduction borrows NetLds::head");
}  // namespace

template <bool LDS_TREE>
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_selfplay_run(SpParams P) {
    __shared__ NetLds S;
    __shared__ float s_eval[kB][10];                                 // a game's last evaluation: policy row, value
    __shared__ uint32_t s_any, s_never;                              // run_steps' words of the iteration in hand
    __shared__ uint32_t s_game[kB][kGwCount];                        // what a game carries from move-step to move-step
    extern __shared__ __attribute__((aligned(16))) unsigned char s_tree[];
    const int tid = threadIdx.x, grp = tid >> 4, j = tid & 15, row0 = tid & 48;
    const size_t gi = (size_t)blockIdx.x * kB + grp;
    const bool valid = gi < P.sp.n;
    RunNode* nodes;
    if constexpr (LDS_TREE) nodes = (RunNode*)s_tree + (size_t)grp * P.sp.slab;
    else nodes = P.sp.nodes + (valid ? gi : 0) * P.sp.slab;

    if (j == 0) {                                                    // TicTacToe::new, mod.rs:28-30: the empty board, -1 to move
#pragma unroll
        for (int i = 0; i < kGwCount; ++i) s_game[grp][i] = i == kGwLive && valid ? 1u : 0u;
        if (valid) { SpGame m; m.flush_step = kSpNone; m.n_flushed = 0u; m.kind = kSpZero; m.winner = 0; P.games[gi] = m; }
    }
    Row R;
#pragma unroll
    for (int i = 0; i < kCntCount; ++i) R.cnt[i] = 0u;
    group_barrier();

#pragma unroll 1
    for (uint32_t s = 0; s < P.steps; ++s) {                         // alpha_parallel.rs:129
        uint32_t n_live = 0u;
#pragma unroll
        for (int g = 0; g < kB; ++g) n_live += s_game[g][kGwLive];
        if (n_live == 0u) break;                                     // the same in every thread
        if (tid == 0) __hip_atomic_fetch_add(P.head->live + s, n_live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t st = s_game[grp][kGwState];
        const bool live = s_game[grp][kGwLive] != 0u;

        // ---- search: a fresh tree every move-step (:137), the Dirichlet sample of (seed, s) -------------------------------------------------
        run_steps(P.sp, P.noise[s], P.any_selected + (size_t)s * P.sp.iterations, S, s_eval, s_any, s_never, nodes, live, gi, st, tid, R);
        uint32_t nc;
        float root_visits;
        const float prob = run_root_row(nodes, live, st, j, row0, nc, root_visits);

        // ---- play: the body of the loop over the live games, :168-224 ---------------------------------------------------------------------
        uint32_t round = s_game[grp][kGwRound], frags = s_game[grp][kGwFrags];
        const double u = draw_uniform(P.seed, P.first_game_id + (uint32_t)gi, round, kTagSample, 0u);        // :192
        const float w = det_powf(live && nc != 0u && j < 9 ? prob : 0.f, P.inv_t);                            // :165, not renormalised (Q17)
        double total;
        const int a = weighted_pick(w, u, row0, total);
        if (live) {
            bool removed = false, flushed = false;
            if (round >= P.round_limit) {                            // :172-180, no `continue`: what is recorded below is not delivered
                if (j == 0) { SpGame m; m.flush_step = s; m.n_flushed = frags; m.kind = kSpZero; m.winner = 0; P.games[gi] = m; }
                removed = true; flushed = true;
            }
            uint32_t illegal = 0u;
            if (nc == 0u) {                                          // :183-189
                st ^= 1u << 18;
            } else {
                if (frags < kSpMaxSteps) {                           // :195-199 (one fragment per move-step: always)
                    SpFrag* f = P.frags + gi * kSpMaxSteps + frags;
                    if (j < 9) {
                        const int cell = cell_of(st, j);
                        f->ps[j] = w;
#pragma unroll
                        for (int c = 0; c < 3; ++c) f->planes[c * 9 + j] = cell == c - 1 ? 1.0f : 0.0f;
                    }
                    if (j == 0) f->player = player_of(st);
                    frags += 1u;
                }
                illegal = ((st >> (2 * a)) & 3u) != 0u ? 1u : 0u;    // :202-210 decode, assert legal, apply: the cell takes the player
                st = apply_move(st & ~(3u << (2 * a)), a);
                int winner;
                if (finished(st, winner)) {                          // :215-223
                    if (!flushed && j == 0) { SpGame m; m.flush_step = s; m.n_flushed = frags; m.kind = kSpWinner; m.winner = winner; P.games[gi] = m; }
                    removed = true;
                }
            }
            if (j == 0) {
                s_game[grp][kGwState] = st; s_game[grp][kGwRound] = round + 1u; s_game[grp][kGwFrags] = frags;     // :213
                s_game[grp][kGwPlies] += 1u; s_game[grp][kGwIllegal] += illegal;
                if (removed) { s_game[grp][kGwLive] = 0u; s_game[grp][kGwGames] += 1u; }
            }
        }
        group_barrier();
    }

    // ---- the statistics: the search's counters and the driver's, once per workgroup --------------------------------------------------------
    uint32_t* red = (uint32_t*)S.head;                               // (the network is done with it: a barrier ago)
    if (j == 0) {
#pragma unroll
        for (int i = 0; i < kCntCount; ++i) red[grp * kSpCntCount + i] = R.cnt[i];
        red[grp * kSpCntCount + kSpPlies] = s_game[grp][kGwPlies];
        red[grp * kSpCntCount + kSpGames] = s_game[grp][kGwGames];
        red[grp * kSpCntCount + kSpIllegal] = s_game[grp][kGwIllegal];
    }
    group_barrier();
    if (tid < kSpCntCount) {
        unsigned long long t = 0;
        for (int g = 0; g < kB; ++g) {
            const unsigned long long v = red[g * kSpCntCount + tid];
            t = tid == kCntMaxChildren ? (v > t ? v : t) : t + v;
        }
        if (tid == kCntMaxChildren) __hip_atomic_fetch_max(P.head->counters + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (t) __hip_atomic_fetch_add(P.head->counters + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// each flushed game's first output row in the order (move-step, game), and nf
__global__ __launch_bounds__(1024) DIEE_TTT_NO_PK_F32 void k_ttt_sp_offsets(SpParams P) {
    __shared__ uint32_t s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0u;                                             // rows before this chunk: the same in every thread
    for (uint32_t s = 0; s < P.steps; ++s) {
        for (uint32_t c0 = 0; c0 < P.sp.n; c0 += 1024u) {
            const uint32_t g = c0 + (uint32_t)tid;
            uint32_t v = 0u;
            bool keep = false;
            if (g < P.sp.n) {
                const SpGame m = P.games[g];
                keep = m.flush_step == s;
                v = keep ? m.n_flushed : 0u;
            }
            uint32_t before = 0u, in_wave = 0u;                      // v <= 9: four bit planes, a ballot each
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(((v >> b) & 1u) != 0u);
                before += (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull)) << b;
                in_wave += (uint32_t)__builtin_popcountll(bal) << b;
            }
            if (lane == 0) s_wave[wave] = in_wave;
            group_barrier();
            uint32_t off = carry, all = 0u;
            for (int w = 0; w < 16; ++w) { const uint32_t t = s_wave[w]; off += w < wave ? t : 0u; all += t; }
            if (keep) P.first_row[g] = off + before;
            carry += all;
            group_barrier();                                         // (s_wave is read before the next chunk writes it)
        }
    }
    if (tid == 0) P.head->nf = carry;
}

// the fragments of the flushed games -> the compact arrays; outcome: alpha_parallel.rs:216-217
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_sp_gather(SpParams P) {
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6), t = threadIdx.x & 63u;
    if (g >= P.sp.n) return;
    const SpGame m = P.games[g];
    if (m.flush_step == kSpNone) return;
    const size_t nf = P.head->nf, first = P.first_row[g];
    uint32_t* state = (uint32_t*)P.rec;
    uint32_t* ps = state + nf * PLANES;
    uint32_t* game = ps + nf * A;
    int8_t* outcome = (int8_t*)(game + nf);
    const uint32_t n = m.n_flushed < kSpMaxSteps ? m.n_flushed : kSpMaxSteps;
    for (uint32_t f = 0; f < n; ++f) {
        const uint32_t* src = (const uint32_t*)(P.frags + (size_t)g * kSpMaxSteps + f);
        const size_t row = first + f;
        if (row >= nf) return;                                       // (never: the offsets count these very fragments)
        if (t < (uint32_t)A) ps[row * A + t] = src[t];
        else if (t < (uint32_t)(A + PLANES)) state[row * PLANES + (t - A)] = src[t];
        else if (t == (uint32_t)(A + PLANES)) {
            const int player = (int)src[t];
            outcome[row] = (int8_t)(m.kind == kSpZero ? 0 : m.winner == player ? 1 : m.winner == -player ? -1 : 0);
            game[row] = P.first_game_id + g;
        }
    }
}

hipError_t launch_ttt_selfplay(hipStream_t st, const SpParams& P, bool lds_tree, bool first) {
    if (P.sp.n == 0) return hipSuccess;
    const uint32_t groups = P.sp.n / kB + (P.sp.n % kB != 0);
    if (!lds_tree) {
        hipLaunchKernelGGL(k_ttt_selfplay_run<false>, dim3(groups), dim3(256), 0, st, P);
    } else {
        if (first) {                                                 // LDS beyond the static 64 KB has to be asked for
            const hipError_t e = hipFuncSetAttribute((const void*)k_ttt_selfplay_run<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLdsBytes);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_ttt_selfplay_run<true>, dim3(groups), dim3(256), (size_t)kB * P.sp.slab * sizeof(RunNode), st, P);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ttt_sp_offsets, dim3(1), dim3(1024), 0, st, P);
    hipLaunchKernelGGL(k_ttt_sp_gather, dim3(P.sp.n / 4 + (P.sp.n % 4 != 0)), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace ttt
}  // namespace diee
