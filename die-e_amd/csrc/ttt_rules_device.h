// ttt_rules_device.h -- the tic-tac-toe rules on a packed state word and the row-of-16-lanes helpers, shared by the device search
// (ttt_search_iter_device.h) and the arena kernels (ttt_arena_kernels.hip).  The word: 2 bits per cell (0 empty, 1 = +1, 3 = -1) in
// bits 0 .. 17, bit 18 = the player to move is +1.  Everything is DIEE_TTT_NO_PK_F32 and nothing but builtins, so it inlines into the
// kernels of the family (ttt_net_device.h says why).
#pragma once
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"

namespace diee {
namespace ttt {

#define DIEE_TTT_FN __device__ __forceinline__ DIEE_TTT_NO_PK_F32

DIEE_TTT_FN int cell_of(uint32_t st, int j) { return (int)(st << (30 - 2 * j)) >> 30; }                 // -1 / 0 / +1
DIEE_TTT_FN int player_of(uint32_t st) { return (st >> 18) & 1u ? 1 : -1; }
DIEE_TTT_FN uint32_t pack_cell(int v, int j) { return ((uint32_t)v & 3u) << (2 * j); }
DIEE_TTT_FN uint32_t empty_cells(uint32_t st) {                                                      // bit j: cell j is empty
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) m |= ((st >> (2 * j)) & 3u) == 0u ? 1u << j : 0u;
    return m;
}
// apply_move (mod.rs:46-49): the cell takes the player, the player flips
DIEE_TTT_FN uint32_t apply_move(uint32_t st, int j) { return (st | pack_cell(player_of(st), j)) ^ (1u << 18); }
__device__ __forceinline__ constexpr int line_cell(int l, int i) { return l < 3 ? 3 * l + i : l < 6 ? l - 3 + 3 * i : l == 6 ? 4 * i : 2 + 2 * i; }
// check_winner (mod.rs:60-81): the first complete line in the order rows, columns, 0-4-8, 2-4-6; else a full board is a draw
DIEE_TTT_FN bool finished(uint32_t st, int& winner) {
    bool found = false;
    winner = 0;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const int a = cell_of(st, line_cell(l, 0));
        if (!found && a != 0 && a == cell_of(st, line_cell(l, 1)) && a == cell_of(st, line_cell(l, 2))) { winner = a; found = true; }
    }
    return found || (st & 0x15555u) == 0x15555u;
}

DIEE_TTT_FN float as_f32(uint32_t u) { return __builtin_bit_cast(float, u); }      // by value: a vector element is no operand for the builtin
DIEE_TTT_FN uint32_t row_get(uint32_t v, int src_lane) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v); }
DIEE_TTT_FN float row_getf(float v, int src_lane) { return as_f32(row_get(__builtin_bit_cast(uint32_t, v), src_lane)); }
DIEE_TTT_FN uint32_t row_ballot(bool p, int row0) { return (uint32_t)(__builtin_amdgcn_ballot_w64(p) >> row0) & 0xFFFFu; }

// weighted_select of ttt_host.cpp (alphazero.rs:129-137, rand's WeightedIndex over f64) on a row: lane j < 9 brings the weight of cell j
// (the other lanes 0), every lane replays the sequential f64 sum of the nine in cell order, then the running sum against u * total: the
// first cell that exceeds it, of rounding's leftovers the last non-zero one.  All lanes of the wave come here.
DIEE_TTT_FN int weighted_pick(float w, double u, int row0, double& total) {
    total = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) total += (double)row_getf(w, row0 + c);
    const double thr = u * total;
    double cum = 0.0;
    int pick = -1, last_nz = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const float wc = row_getf(w, row0 + c);
        if (wc != 0.f) last_nz = c;
        cum += (double)wc;
        if (pick < 0 && cum > thr) pick = c;
    }
    return pick < 0 ? last_nz : pick;
}

}  // namespace ttt
}  // namespace diee
