// ttt_arena_move_device.h -- a turn of the tic-tac-toe arena on a row of 16 lanes (lane j < 9 is cell j): get_actions_for_player
// (versus.rs:270-318) for a Model and a Random player and the body of play()'s per-game loop (:220-266), the ONE copy that k_ttt_arena_move
// (ttt_arena_kernels.hip, a turn per launch) and k_ttt_arena_run (ttt_arena_run_kernels.hip, a game per launch) both call, so a turn is the
// same statements in either.  draw_uniform and det_powf are bg_device.h's own, the functions the host path calls.
#pragma once
#include <hip/hip_runtime.h>

#include "bg_device.h"
#include "ttt_rules_device.h"

namespace diee {
namespace ttt {

constexpr int kEmptyMove = 10;                                                        // TicTacToe::EMPTY_MOVE: the turn is skipped

// :279-299.  `prob`: lane j's entry of the search's row (NaN, the row of a childless root, and entries <= 0 give 0), `nc` the root's children,
// u = draw_uniform(seed, game, round, kTagSample, 0).  All lanes of the wave come here.
DIEE_TTT_FN int model_move(float prob, uint32_t nc, float inv_t, double u, int row0) {
    const float w = det_powf(prob > 0.f ? prob : 0.f, inv_t);
    double total;
    const int pick = weighted_pick(w, u, row0, total);
    return nc != 0u && total > 0.0 ? pick : kEmptyMove;                               // :286-293: else EMPTY_MOVE
}

// :308-317: the min(int(u * count), count - 1)-th empty cell of the row's ballot.  All lanes of the wave come here.
DIEE_TTT_FN int random_move(uint32_t st, double u, int j, int row0) {
    const uint32_t mask = row_ballot(j < 9 && cell_of(st, j < 9 ? j : 0) == 0, row0);
    const int count = __builtin_popcount(mask);
    int idx = (int)(u * (double)count);
    idx = idx > count - 1 ? count - 1 : idx;
    int move = kEmptyMove, seen = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const bool set = (mask >> c) & 1u;
        if (set && seen == idx) move = c;
        seen += set ? 1 : 0;
    }
    return move;
}

// :225-237 for one game: a skipped turn only flips the player and is judged for nothing; else the move is applied, the board judged and the
// round limit applied (round_count was incremented at :219).  Returns the new state; `moved`, `retired` and `winner` (0 unless retired).
DIEE_TTT_FN uint32_t play_turn(uint32_t st, int move, uint32_t round, uint32_t round_limit, bool& moved, bool& retired, int& winner) {
    moved = move < 9; retired = false; winner = 0;
    if (!moved) return st ^ (1u << 18);                                               // :225-228 skip_turn; continue
    st = apply_move(st, move);                                                        // :230
    int w;
    const bool over = finished(st, w);
    if (over || round + 1u >= round_limit) { retired = true; winner = w; }            // :233-237
    return st;
}

}  // namespace ttt
}  // namespace diee
