// arena_kernels.hip -- the arena (play() / get_actions_for_player, src/versus.rs:160-318) on the device for gfx950.
//
// The searches are the engine's own (mcts_run on the slots k_arena_gather fills); what is here is the arena's round logic, which is
// not self-play's: no records, a skipped turn bypasses the winner and round-limit check, and the limit is on the call's round
// counter.  None of these kernels waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bg_device.h"
#include "launch.h"
#include "mcts_device.h"
#include "search_types.h"
#include "wave_ops.h"

namespace diee {

// versus.rs:166-189: Backgammon::new for every game, the second half after a skip_turn (side +1 to move), the opening dice of
// (seed, game, 0, kTagInitRoll); the live list and the per-game words
__global__ void k_arena_init(Arena A, unsigned long long seed) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < AW_COUNT) A.words[g] = g == AW_LIVE ? A.n_games : 0u;
    if (g >= A.n_games) return;
    BgState s;
    // Backgammon::new, backgammon_logic.rs:80-94
    s.w[0] = 0x00000002u; s.w[1] = 0xFD00FB00u; s.w[2] = 0x05000000u; s.w[3] = 0x000000FBu;
    s.w[4] = 0x00050003u; s.w[5] = 0xFE000000u; s.w[6] = 0u;
    int d0, d1;
    draw_dice(seed, g, 0u, kTagInitRoll, 0u, d0, d1);
    const uint32_t player = g < A.n_games / 2 ? 0xFFu : 0x01u;      // :172-174
    s.w[7] = (uint32_t)d0 | ((uint32_t)d1 << 8) | (player << 16);
    store_state(&A.state[g], s);
    store_state(&A.initial[g], s);
    A.alive[g] = 1; A.winner[g] = 0; A.retired_round[g] = kNone; A.retired_side[g] = -1;
    A.live[g] = g;
}

// versus.rs:195-196: the live games by side to move, stable in ascending game index (Q14 couples the slots of a search, so the order
// is part of the result).  One block, like k_compact_live: the live list is compacted in place (the games the last round retired
// drop out) and its survivors go to the two sides' lists; words[AW_COUNT0], [AW_COUNT0 + 1], [AW_LIVE] = the counts and their sum.
__global__ __launch_bounds__(1024) void k_arena_split(Arena A, uint32_t n_live) {
    __shared__ uint32_t wsum[3][16];
    __shared__ uint32_t carry[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3) carry[tid] = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_live; c0 += 1024) {
        const uint32_t i = c0 + tid;
        uint32_t g = 0;
        bool keep = false, second = false;
        if (i < n_live) {
            g = A.live[i];
            keep = A.alive[g] != 0;
            if (keep) second = (int)(int8_t)((A.state[g].w[7] >> 16) & 0xffu) != -1;
        }
        const unsigned long long bal[3] = {__ballot(keep), __ballot(keep && !second), __ballot(keep && second)};
        if (lane == 0)
            for (int j = 0; j < 3; ++j) wsum[j][wave] = (uint32_t)__popcll(bal[j]);
        __syncthreads();
        uint32_t pos[3];
        for (int j = 0; j < 3; ++j) {
            uint32_t off = carry[j];
            for (int w = 0; w < wave; ++w) off += wsum[j][w];
            pos[j] = off + (uint32_t)__popcll(bal[j] & ((1ull << lane) - 1ull));
        }
        __syncthreads();                                        // all reads of live[c0..] done before writes
        if (keep) {
            A.live[pos[0]] = g;
            A.list[(second ? A.n_games : 0u) + pos[second ? 2 : 1]] = g;
        }
        __syncthreads();
        if (tid < 3) { uint32_t t = 0; for (int w = 0; w < 16; ++w) t += wsum[tid][w]; carry[tid] += t; }
        __syncthreads();
    }
    if (tid == 0) { A.words[AW_COUNT0] = carry[1]; A.words[AW_COUNT0 + 1] = carry[2]; A.words[AW_LIVE] = carry[0]; }
}

// the list of the side about to search -> slots (what k_gather_roots does for self-play): one batch spanning the n slots, the RNG
// keys of versus.rs' search call (game ids = game index, rounds = the call's round counter)
__global__ void k_arena_gather(Arena A, Slots S, Segs G, uint32_t side, uint32_t n, uint32_t round) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    const uint32_t g = A.list[(size_t)side * A.n_games + slot];
    store_state(&S.roots[slot], load_state(&A.state[g]));
    S.game_id[slot] = g;
    S.round[slot] = round;
    S.seg[slot] = 0;
    if (slot == 0) { G.first_slot[0] = 0; G.end_slot[0] = n; }
}

// get_actions_for_player (versus.rs:270-318) and the body of play()'s per-game loop (:220-266) for one game of the side that just
// searched (Model) or is about to pick (Random), by one wave
__global__ __launch_bounds__(64) void k_arena_move(Tree T, Arena A, uint32_t n, ArenaParams P, uint32_t* overflow, const uint32_t* mcts_play) {
    __shared__ float row[1352];
    __shared__ WaveScratch sc;
    const uint32_t slot = blockIdx.x;
    if (slot >= n) return;
    const int lane = threadIdx.x;
    const uint32_t g = A.list[(size_t)P.side * A.n_games + slot];
    BgState s = load_state(&A.state[g]);
    uint32_t play = pack_play(kNoMove, kNoMove, kNoMove, kNoMove);      // EMPTY_MOVE
    if (P.agent == 2u) {                                        // Agent::Mcts, :303-306: mct_search's answer (vanilla_kernels.hip)
        play = mcts_play[slot];
    } else if (P.agent != 0u) {                                 // Agent::Model, :279-306
        const size_t base = (size_t)slot * T.node_cap;
        const uint32_t k = meta_nch(T.meta[base]), fc = T.first_child[base];
        if (k != 0) {                                           // :292 root.children.is_empty() -> EMPTY_MOVE
            double total = 0.0;
            const uint32_t code = sample_root_move(T, base, k, fc, row, lane, P.inv_temperature, P.seed, g, P.round, &total);
            if (total > 0.0) play = bg_decode_dev(st_roll(s, 0), st_roll(s, 1), st_player(s), code);     // (an all-zero row -> EMPTY_MOVE too, :286-293)
        }
    } else {                                                    // Agent::Random, :308-317
        int k = bg_legal_plays_wave(s, &sc, lane, overflow);
        if (k > kMaxPlays) { if (lane == 0) atomicOr(overflow, 1u); k = 0; }      // never silent: DIEE_ERR_CAPACITY
        if (k > 0) {
            const double u = draw_uniform(P.seed, g, P.round, kTagSample, 0u);
            int idx = (int)(u * (double)k);
            if (idx > k - 1) idx = k - 1;
            play = sc.play[idx];
        }
    }
    if (lane != 0) return;
    int d0, d1;
    draw_dice(P.seed, g, P.round, kTagMoveRoll, 0u, d0, d1);
    atomicAdd(&A.words[AW_TURNS0 + P.side], 1u);
    ArenaTurn rec{};                                          // Turn { roll, action, player }, versus.rs:21-26, + what makes it replayable
    if (P.log) {
        rec.play[0] = (int8_t)play_f1(play); rec.play[1] = (int8_t)play_t1(play); rec.play[2] = (int8_t)play_f2(play); rec.play[3] = (int8_t)play_t2(play);
        rec.roll[0] = (uint8_t)st_roll(s, 0); rec.roll[1] = (uint8_t)st_roll(s, 1);
        rec.next_roll[0] = (uint8_t)d0; rec.next_roll[1] = (uint8_t)d1;
        rec.player = (int8_t)st_player(s); rec.agent = (uint8_t)P.agent; rec.second = (uint8_t)st_second(s); rec.retired = 0;
    }
    if (play_f1(play) == kNoMove) {                             // :225-228 skip_turn; continue (no winner / round-limit check)
        bg_skip_dev(s, d0, d1);
        store_state(&A.state[g], s);
        if (P.log) P.log[g] = rec;
        return;
    }
    bg_apply_dev(s, play, d0, d1);                              // :230
    store_state(&A.state[g], s);
    atomicAdd(&A.words[AW_MOVES0 + P.side], 1u);
    const int w = bg_winner_dev(s);
    if (w != 0 || P.round + 1 >= P.round_limit) {               // :233-237 (round_count was incremented at :219)
        A.alive[g] = 0; A.winner[g] = (int8_t)w;
        A.retired_round[g] = P.round; A.retired_side[g] = (int8_t)P.side;
        atomicAdd(&A.words[w < 0 ? AW_WINS1 : w > 0 ? AW_WINS2 : AW_DRAWS], 1u);
        atomicAdd(&A.words[AW_RETIRED0 + P.side], 1u);
        rec.retired = 1;
    }
    if (P.log) P.log[g] = rec;                                  // g < n_games = the records of a row
}

// ---- host launchers -----------------------------------------------------------------------------
void launch_arena_init(hipStream_t st, const Arena& A, unsigned long long seed) {
    const uint32_t n = A.n_games > (uint32_t)AW_COUNT ? A.n_games : (uint32_t)AW_COUNT;
    hipLaunchKernelGGL(k_arena_init, dim3((n + 255) / 256), dim3(256), 0, st, A, seed);
}
void launch_arena_split(hipStream_t st, const Arena& A, uint32_t n_live) {
    hipLaunchKernelGGL(k_arena_split, dim3(1), dim3(1024), 0, st, A, n_live);
}
void launch_arena_gather(hipStream_t st, const Arena& A, const Slots& S, const Segs& G, uint32_t side, uint32_t n, uint32_t round) {
    if (!n) return;
    hipLaunchKernelGGL(k_arena_gather, dim3((n + 255) / 256), dim3(256), 0, st, A, S, G, side, n, round);
}
void launch_arena_move(hipStream_t st, const Tree& T, const Arena& A, uint32_t n, const ArenaParams& P, uint32_t* overflow,
                       const uint32_t* mcts_play) {
    if (!n) return;
    hipLaunchKernelGGL(k_arena_move, dim3(n), dim3(64), 0, st, T, A, n, P, overflow, mcts_play);
}

}  // namespace diee
