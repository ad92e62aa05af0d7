// ttt_arena_kernels.hip -- the round logic of the tic-tac-toe arena (play::<TicTacToe>, src/versus.rs:160-318; ttt_host.cpp: Engine::arena states
// the same rules on the host) on gfx950.  Reached through diee_ttt_arena while option "search" of the hosting ctx is "device"
// (ttt_arena_device.h).  The searches are the family's own, k_ttt_search and k_ttt_vanilla, enqueued on roots these kernels leave on the
// device; what is here is what the Python driver did between them: split the live games by side, sample or pick a move per game, apply it,
// judge the board, retire the game, keep the call's totals.  No workgroup waits for another, all stores are plain C++.
//
// State.  One packed word per game (ttt_rules_device.h) in HBM, beside it winner, retired round and side; retired_round == kArenaNone is
//   "alive".  The live list holds the live games in ascending index.
// k_ttt_arena_split, ONE workgroup of 1024 threads per round: a thread takes a game of the live list, the 16 waves ballot "alive", "alive
//   and side -1 to move", "alive and side +1 to move", a prefix over the waves' counts in LDS places every game: the live list is
//   compacted in place (the games the last round retired drop out) and each side's list is written as (game id, round) pairs -- the keys
//   k_ttt_vanilla reads, the ids k_ttt_arena_move reads -- with its states unpacked to diee_ttt_state, the roots both searches read.  Lists
//   longer than 1024 go in chunks with the counts carried.  Stable, so a list is in ascending game index: Q14 couples the slots of a search.
// k_ttt_arena_move<agent>, the family's split: a workgroup of 256 owns 16 games of the side's list, a game is a row of 16 lanes, lane j < 9
//   is cell j; what the row agrees on is computed redundantly in all its lanes and crosses lanes with ds_bpermute.
//   Model    lane j raises its entry of the search's row to 1 / temperature (det_powf; NaN and entries <= 0 give 0), every lane replays the
//            sequential f64 sum of the nine in cell order, then the running sum against u * total: the first cell that exceeds it, of
//            rounding's leftovers the last non-zero one.  A root without children or a zero total skips the turn.
//   Random   the row's ballot of empty cells; the min(int(u * count), count - 1)-th set bit.
//   Mcts     the move k_ttt_vanilla left in its VanillaOut; 10 skips the turn.
//   (model_move, random_move and play_turn of ttt_arena_move_device.h: k_ttt_arena_run of ttt_arena_run_kernels.hip calls them too)
//   then lane 0 applies the move, looks for a winner or a full board, applies the round limit, retires the game; a skipped turn only flips
//   the player.  The turn's counts (and an Mcts search's per-game counters) are reduced over the 16 rows in LDS and added once per
//   workgroup to the call's totals; workgroup 0 of a Model turn also adds the search's counters and the rows it evaluated, (1 + the
//   any_selected words that are set) * n, so nothing of a search is read by the host.
//   u = draw_uniform(seed, game, round, kTagSample, 0).  draw_uniform and det_powf are bg_device.h's own, the functions the host path
//   calls: they carry no target attribute, so here they are two real calls (f64 and integer arithmetic, nothing that could pair up).
// Everything else is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called (ttt_net_device.h says why).
#include <hip/hip_runtime.h>

#include "bg_device.h"
#include "ttt_arena_device.h"
#include "ttt_arena_move_device.h"
#include "ttt_net_device.h"
#include "ttt_rules_device.h"

namespace diee {
namespace ttt {

namespace {
enum { kRedPlies, kRedMoves, kRedRetired, kRedWins1, kRedWins2, kRedDraws, kRedSelections, kRedExpansions, kRedTerminal, kRedDepthSum, kRedOverflow,
       kRedCount };

DIEE_TTT_FN void total_add(unsigned long long* p, unsigned long long v) {
    if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace

// versus.rs:166-189: TicTacToe::new for every game, the second half after a skip_turn (side +1 to move); the live list, the totals
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_arena_init(ArenaGames G) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < (uint32_t)kTaWords) G.totals[g] = 0ull;
    if (g < 3u) G.counts[g] = g == 2u ? G.n_games : 0u;
    if (g >= G.n_games) return;
    G.state[g] = g < G.n_games / 2 ? 0u : 1u << 18;                       // :172-174
    G.retired_round[g] = kArenaNone; G.winner[g] = 0; G.retired_side[g] = -1;
    G.live[g] = g;
}

// versus.rs:195-196, and the retire compaction of the round before
__global__ __launch_bounds__(1024) DIEE_TTT_NO_PK_F32 void k_ttt_arena_split(ArenaGames G, uint32_t n_live, uint32_t round) {
    __shared__ uint32_t s_wave[3][16];
    __shared__ uint32_t s_carry[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3) s_carry[tid] = 0u;
    group_barrier();
    for (uint32_t c0 = 0; c0 < n_live; c0 += 1024u) {
        const uint32_t i = c0 + (uint32_t)tid;
        uint32_t g = 0u, st = 0u;
        bool keep = false;
        if (i < n_live) {
            g = G.live[i];
            keep = G.retired_round[g] == kArenaNone;
            st = G.state[g];
        }
        const bool second = player_of(st) > 0;
        const unsigned long long bal[3] = {__builtin_amdgcn_ballot_w64(keep), __builtin_amdgcn_ballot_w64(keep && !second),
                                           __builtin_amdgcn_ballot_w64(keep && second)};
        if (lane == 0)
            for (int k = 0; k < 3; ++k) s_wave[k][wave] = (uint32_t)__builtin_popcountll(bal[k]);
        group_barrier();                                                  // (also: every read of live[c0 ..] is done before it is written)
        uint32_t pos[3];
        for (int k = 0; k < 3; ++k) {
            uint32_t off = s_carry[k];
            for (int w = 0; w < wave; ++w) off += s_wave[k][w];
            pos[k] = off + (uint32_t)__builtin_popcountll(bal[k] & ((1ull << lane) - 1ull));
        }
        if (keep) {
            G.live[pos[0]] = g;                                           // pos[0] <= i
            const size_t at = (size_t)(second ? G.n_games : 0u) + pos[second ? 2 : 1];
            G.keys[2 * at] = g; G.keys[2 * at + 1] = round;
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < 9; ++c) w[c >> 2] |= ((uint32_t)cell_of(st, c) & 0xFFu) << (8 * (c & 3));
            w[2] |= ((uint32_t)player_of(st) & 0xFFu) << 8;
            u32x4* r = (u32x4*)(G.roots + at);
            r[0] = u32x4{w[0], w[1], w[2], 0u}; r[1] = u32x4{0u, 0u, 0u, 0u};
        }
        group_barrier();
        if (tid < 3) { uint32_t t = 0u; for (int w = 0; w < 16; ++w) t += s_wave[tid][w]; s_carry[tid] += t; }
        group_barrier();
    }
    if (tid == 0) { G.counts[0] = s_carry[1]; G.counts[1] = s_carry[2]; }
}

// get_actions_for_player (versus.rs:270-318) and the body of play()'s per-game loop (:220-266) for the side that just searched (Model,
// Mcts) or is about to pick (Random)
template <int AGENT>
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_arena_move(ArenaGames G, ArenaMove M) {
    __shared__ uint32_t s_red[kB][kRedCount];
    __shared__ uint32_t s_set;
    const int tid = threadIdx.x, grp = tid >> 4, j = tid & 15, row0 = tid & 48;        // row0: the first lane of this game's row within its wave
    const size_t gi = (size_t)blockIdx.x * kB + grp;
    const bool valid = gi < M.n;
    const size_t slot = valid ? gi : 0;                                                // a row past n reads slot 0 and stores nothing
    const uint32_t g = G.keys[2 * ((size_t)M.side * G.n_games + slot)];
    uint32_t st = G.state[g];
    if (tid == 0) s_set = 0u;

    uint32_t red[kRedCount];
#pragma unroll
    for (int i = 0; i < kRedCount; ++i) red[i] = 0u;
    int move = kEmptyMove;
    if (AGENT == DIEE_AGENT_MCTS) {                                                    // :303-306
        const VanillaOut* O = M.vout + slot;
        move = (int)O->move;
        red[kRedSelections] = O->cnt[kVcIterations]; red[kRedExpansions] = O->cnt[kVcExpansions]; red[kRedTerminal] = O->cnt[kVcTerminal];
        red[kRedDepthSum] = O->cnt[kVcDepthSum]; red[kRedOverflow] = O->overflow;
    } else {
        const double u = draw_uniform(M.seed, g, M.round, kTagSample, 0u);
        if (AGENT == DIEE_AGENT_MODEL) move = model_move(j < 9 ? M.probs[slot * 9 + (size_t)j] : 0.f, M.n_children[slot], M.inv_t, u, row0);      // :279-299
        else move = random_move(st, u, j, row0);                                       // :308-317
    }
    if (valid && j == 0) {
        bool moved, retired;
        int w;
        G.state[g] = play_turn(st, move, M.round, M.round_limit, moved, retired, w);   // :225-237
        red[kRedPlies] = 1u;
        red[kRedMoves] = moved ? 1u : 0u;
        if (retired) {
            G.winner[g] = (int8_t)w; G.retired_round[g] = M.round; G.retired_side[g] = (int8_t)M.side;
            red[kRedRetired] = 1u;
            red[w < 0 ? kRedWins1 : w > 0 ? kRedWins2 : kRedDraws] = 1u;
        }
    }
    if (j == 0) {
#pragma unroll
        for (int i = 0; i < kRedCount; ++i) s_red[grp][i] = valid ? red[i] : 0u;
    }
    group_barrier();
    if (tid < kRedCount) {
        unsigned long long t = 0;
        for (int r = 0; r < kB; ++r) t += s_red[r][tid];
        unsigned long long* mine = G.totals + (size_t)M.side * kTaPlayerWords;
        switch (tid) {
            case kRedPlies: total_add(mine + kTaPlies, t); break;
            case kRedMoves: total_add(mine + kTaMoves, t); break;
            case kRedRetired:
                total_add(mine + kTaRetired, t);
                if (t) __hip_atomic_fetch_sub(G.counts + 2, (uint32_t)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            case kRedWins1: total_add(G.totals + kTaWins1, t); break;
            case kRedWins2: total_add(G.totals + kTaWins2, t); break;
            case kRedDraws: total_add(G.totals + kTaDraws, t); break;
            case kRedSelections: total_add(mine + kTaSelections, t); break;
            case kRedExpansions: total_add(mine + kTaExpansions, t); break;
            case kRedTerminal: total_add(mine + kTaTerminal, t); break;
            case kRedDepthSum: total_add(mine + kTaDepthSum, t); break;
            default: total_add(G.totals + kTaOverflow, t); break;
        }
    }
    if (AGENT == DIEE_AGENT_MODEL && blockIdx.x == 0) {                                // the search's own counters -> this player's totals
        for (uint32_t k0 = 0; k0 < M.iterations; k0 += 256u) {
            const uint32_t k = k0 + (uint32_t)tid;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(k < M.iterations && M.any_selected[k < M.iterations ? k : 0u] != 0u);
            if ((tid & 63) == 0 && bal) __hip_atomic_fetch_add(&s_set, (uint32_t)__builtin_popcountll(bal), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        group_barrier();
        unsigned long long* mine = G.totals + (size_t)M.side * kTaPlayerWords;
        if (tid == 0) total_add(mine + kTaNnEvals, (1ull + s_set) * M.n);              // the roots, then one per iteration somebody selected in
        if (tid < kCntCount) {
            const unsigned long long v = M.counters[tid];
            switch (tid) {
                case kCntExpansions: total_add(mine + kTaExpansions, v); break;
                case kCntChildren: total_add(mine + kTaChildren, v); break;
                case kCntMaxChildren: __hip_atomic_fetch_max(mine + kTaMaxChildren, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;
                case kCntSelections: total_add(mine + kTaSelections, v); break;
                case kCntDepthSum: total_add(mine + kTaDepthSum, v); break;
                default: total_add(mine + kTaTerminal, v); break;
            }
        }
    }
}

void launch_ttt_arena_init(hipStream_t st, const ArenaGames& G) {
    const uint32_t n = G.n_games > (uint32_t)kTaWords ? G.n_games : (uint32_t)kTaWords;
    hipLaunchKernelGGL(k_ttt_arena_init, dim3(n / 256 + (n % 256 != 0)), dim3(256), 0, st, G);
}
void launch_ttt_arena_split(hipStream_t st, const ArenaGames& G, uint32_t n_live, uint32_t round) {
    hipLaunchKernelGGL(k_ttt_arena_split, dim3(1), dim3(1024), 0, st, G, n_live, round);
}
void launch_ttt_arena_move(hipStream_t st, const ArenaGames& G, const ArenaMove& M, int agent) {
    if (M.n == 0) return;
    const dim3 groups(M.n / kB + (M.n % kB != 0));
    if (agent == DIEE_AGENT_MODEL) hipLaunchKernelGGL(k_ttt_arena_move<DIEE_AGENT_MODEL>, groups, dim3(256), 0, st, G, M);
    else if (agent == DIEE_AGENT_MCTS) hipLaunchKernelGGL(k_ttt_arena_move<DIEE_AGENT_MCTS>, groups, dim3(256), 0, st, G, M);
    else hipLaunchKernelGGL(k_ttt_arena_move<DIEE_AGENT_RANDOM>, groups, dim3(256), 0, st, G, M);
}

}  // namespace ttt
}  // namespace diee
