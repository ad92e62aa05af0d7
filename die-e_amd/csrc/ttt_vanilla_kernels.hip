// ttt_vanilla_kernels.hip -- k_ttt_vanilla: Agent::Mcts for tic-tac-toe (mct_search, src/mcts/simple_mcts.rs:10-39; Node::expand / simulate,
// src/mcts/node.rs:118-137,176-196; ttt_host.cpp: vanilla_search_host) on gfx950.  Reached through diee_ttt_mcts_vanilla_batch while option
// "search" of the ctx is "device" (ttt_vanilla_device.h); the host search stays the default.  There is no network to wait for, so a WHOLE
// iteration -- selection, one expansion, the rollout, the backpropagation -- stays inside the kernel and a launch runs up to
// kVanillaItersPerLaunch of them per game; a call is ceil(iterations / that) launches on one stream and the host reads nothing in between.
//
// Work split.  A workgroup of 4 wavefronts owns 16 games, a game is a row of 16 lanes (4 games per wave), no workgroup waits for another and
//   no row waits for another: the kernel has no workgroup barrier.  What a row agrees on (the node in hand, its visits, the board of the
//   rollout) is kept redundantly in all its lanes; values cross lanes with ds_bpermute inside the row, never through memory.
// Tree.  Nodes of 48 bytes (ttt_vanilla_device.h) in a slab of min(iterations + 1, 986410) per game.  Children are created one per visit
//   and are not contiguous, so a node carries their indices.  The slab is in LDS (template LDS = true) when the whole search is one launch
//   and a game needs at most kVanillaLdsNodes nodes, in HBM otherwise, where it carries over from launch to launch together with the game's
//   VanillaGame record.  Both placements run the same code on the same words and give the same bits.
// An iteration of one row:
//   select   every lane holds the node in hand (index, visits, value, meta).  Per level lane j < created reads child index j, then that
//            child's first 16 bytes, and scores it: value / visits + sqrt((c * ln[parent visits]) / visits), fp32, correctly rounded division
//            and square root, no contraction, ln from the host's table.  The nine scores go round the row by bpermute and every lane replays
//            the fold `if (!(best > u)) best = child` in creation order (last of equal maxima, NaN compares Equal); the winner's words come
//            over with the bpermute that names it.  Lane d keeps what it saw of the node at depth d: the path is never written down.
//   expand   the selected node is no finished game: its next child takes the empty cell number count - 1 - created in ascending order.
//   rollout  lane p of the row draws the Philox block of ply p (counter iteration << 12 | 1 + p): all uniforms of the rollout are there
//            before it starts.  A rollout from a child ends after at most 8 plies (the ninth look finds a full board), each ply is "take
//            the k-th empty cell, test the eight lines" on registers.  Under DIEE_FLAG_REF_QUIRKS nothing is played (Q22).
//   backpropagate   stores only: lane j <= d writes visits + 1 and value + result to the node it kept; lane d also appends the child's
//            index and lane d + 1 writes the new node, born with visits 1 and the result as its value.
//   One fence per iteration orders these stores before the next descent's loads of the same row.
// The launch that reaches `iterations` writes the answers: the root's most visited child (the last created of equal ones), the children's
// statistics in creation order and the game's counters, one VanillaOut per game; the host adds the counters up.
// Everything is compiled under DIEE_TTT_NO_PK_F32 with nothing but builtins called (ttt_net_device.h says why); all stores are plain C++.
#include <hip/hip_runtime.h>

#include "ttt_net_device.h"
#include "ttt_vanilla_device.h"

namespace diee {
namespace ttt {

namespace {
#define DIEE_TTT_FN __device__ __forceinline__ DIEE_TTT_NO_PK_F32
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr uint32_t kOccupied = 0x15555u;          // the low bit of every cell
constexpr uint32_t kPlayerBit = 1u << 18;
constexpr uint32_t kTagVanillaTtt = 0xFFFFFFFBu;  // TAG_VANILLA of bg_device.h

DIEE_TTT_FN float as_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
DIEE_TTT_FN uint32_t as_u32(float f) { return __builtin_bit_cast(uint32_t, f); }
DIEE_TTT_FN uint32_t row_get(uint32_t v, int src_lane) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v); }
DIEE_TTT_FN float row_getf(float v, int src_lane) { return as_f32(row_get(as_u32(v), src_lane)); }

DIEE_TTT_FN int player_of(uint32_t st) { return st & kPlayerBit ? 1 : -1; }
DIEE_TTT_FN uint32_t empty_cells(uint32_t st) {                                    // bit j: cell j is empty
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) m |= ((st >> (2 * j)) & 1u) << j;
    return ~m & 0x1FFu;
}
DIEE_TTT_FN int kth_cell(uint32_t mask, int k) {                                   // the k-th set bit from below (0 if there is none)
    int cell = 0, seen = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const bool set = (mask >> j) & 1u;
        if (set && seen == k) cell = j;
        seen += set ? 1 : 0;
    }
    return cell;
}
// apply_move (mod.rs:46-49): the cell takes the player to move (+1 = 1, -1 = 3), the player flips
DIEE_TTT_FN uint32_t apply_move(uint32_t st, int cell) { return (st | ((st & kPlayerBit ? 1u : 3u) << (2 * cell))) ^ kPlayerBit; }
// one line: `m` holds both bits of its three cells; all three +1 = their low bits alone, all three -1 = all six bits
DIEE_TTT_FN void line(uint32_t st, uint32_t m, bool& found, int& winner) {
    const uint32_t v = st & m;
    if (!found && (v == (m & kOccupied) || v == m)) { winner = v == m ? -1 : 1; found = true; }
}
// check_winner (mod.rs:60-81): the first complete line in the order rows, columns, 0-4-8, 2-4-6; else a full board is a draw
DIEE_TTT_FN bool finished(uint32_t st, int& winner) {
    bool found = false;
    winner = 0;
    line(st, 0x0003Fu, found, winner); line(st, 0x00FC0u, found, winner); line(st, 0x3F000u, found, winner);
    line(st, 0x030C3u, found, winner); line(st, 0x0C30Cu, found, winner); line(st, 0x30C30u, found, winner);
    line(st, 0x30303u, found, winner); line(st, 0x03330u, found, winner);
    return found || (st & kOccupied) == kOccupied;
}
DIEE_TTT_FN float result_for(int winner, int player) { return winner == player ? 1.0f : (winner == -player ? -1.0f : 0.0f); }

// draw_uniform (bg_device.h) of the counter (game, round, TAG_VANILLA, ord), spelled out: Philox4x32-10, the high 53 bits of words 3:2
DIEE_TTT_FN double uniform_of(unsigned long long seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint64_t x = ((uint64_t)c3 << 32) | c2;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

// A row's stores of one iteration become visible to its loads of the next: lanes of one wavefront, so ordering the wave's own memory
// operations is all it takes.
DIEE_TTT_FN __attribute__((convergent)) void row_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
}  // namespace

template <bool LDS>
__global__ __launch_bounds__(256) DIEE_TTT_NO_PK_F32 void k_ttt_vanilla(VanillaParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tree[LDS ? kB * kVanillaLdsNodes * kVNodeWords : 4];
    const int tid = threadIdx.x, grp = tid >> 4, j = tid & 15, row0 = tid & 48;        // row0: the first lane of this game's row within its wave
    const size_t gi = (size_t)blockIdx.x * kB + grp;
    const bool valid = gi < P.n;
    const size_t g = valid ? gi : 0;                                                   // a row past n reads game 0 and stores nothing
    uint32_t* tree = LDS ? s_tree + grp * (kVanillaLdsNodes * kVNodeWords) : P.nodes + g * P.slab * kVNodeWords;
    const uint32_t cap = LDS ? kVanillaLdsNodes : P.slab;

    uint32_t root_state = 0u;
    {
        const uint32_t* r = (const uint32_t*)(P.roots + g);
        const uint32_t w0 = r[0], w1 = r[1], w2 = r[2];
#pragma unroll
        for (int cidx = 0; cidx < 9; ++cidx) {
            const uint32_t w = cidx < 4 ? w0 : cidx < 8 ? w1 : w2;
            root_state |= ((uint32_t)(int)(signed char)(w >> (8 * (cidx & 3))) & 3u) << (2 * cidx);
        }
        if ((signed char)(w2 >> 8) > 0) root_state |= kPlayerBit;
    }
    int root_winner;
    const bool run = valid && !finished(root_state, root_winner);                      // a finished root runs no iteration (simple_mcts.rs:12-14)
    const int player = player_of(root_state);
    const uint32_t game = P.keys[2 * g], round = P.keys[2 * g + 1];

    uint32_t used = 1u, overflow = 0u, cnt[kVcCount];
#pragma unroll
    for (int i = 0; i < kVcCount; ++i) cnt[i] = 0u;
    if (P.it0 == 0u) {
        if (valid && j == 0) *(u32x4*)tree = u32x4{0u, 0u, root_state, 0u};
    } else if (!LDS) {
        const VanillaGame* G = P.games + g;
        used = G->used & 0x7FFFFFFFu; overflow = G->used >> 31;
#pragma unroll
        for (int i = 0; i < kVcCount; ++i) cnt[i] = G->cnt[i];
    }
    row_sync();

#pragma unroll 1
    for (uint32_t it = P.it0; it < P.it1; ++it) {
        // ---- select (simple_mcts.rs:88-94): down while the node has children and no unexpanded move ---------------------------------------
        uint32_t cur = 0u, d = 0u, cvis, cmeta, mynode = 0u, myvis;
        float cval, myval;
        {
            const u32x4 h = *(const u32x4*)tree;
            cvis = h.x; cval = as_f32(h.y); cmeta = h.z;
        }
        myvis = cvis; myval = cval;
#pragma unroll 1
        for (int lvl = 0; lvl < 9; ++lvl) {
            const uint32_t nc = cmeta >> kVCreatedShift;
            const bool act = run && nc != 0u && nc == (uint32_t)__builtin_popcount(empty_cells(cmeta));
            if (__builtin_amdgcn_ballot_w64(act) == 0) break;        // wave-wide: the lanes stay together for the bpermutes below
            uint32_t ci = 0u;
            u32x4 h = u32x4{0u, 0u, 0u, 0u};
            if (act && (uint32_t)j < nc) {
                ci = tree[cur * kVNodeWords + 3u + (uint32_t)j];
                ci = ci < used ? ci : used - 1u;                     // (an index is below `used` by construction)
                h = *(const u32x4*)(tree + ci * kVNodeWords);
            }
            const uint32_t lk = cvis <= P.iterations ? cvis : P.iterations + 1u;
            const float cl = P.c * P.ln[act ? lk : 1u];
            const float v = (float)h.x;
            const float q = as_f32(h.y) / v;
            const float e = __builtin_sqrtf(cl / v);
            const float score = q + e;
            int best = 0;
            float ub = row_getf(score, row0);
#pragma unroll
            for (int jj = 1; jj < 9; ++jj) {                         // Iterator::max_by: the LAST of equal maxima; NaN compares Equal
                const float un = row_getf(score, row0 + jj);
                if ((uint32_t)jj < nc && !(ub > un)) { best = jj; ub = un; }
            }
            const uint32_t ncur = row_get(ci, row0 + best), nvis = row_get(h.x, row0 + best);
            const uint32_t nval = row_get(h.y, row0 + best), nmeta = row_get(h.z, row0 + best);
            if (act) {
                cur = ncur; cvis = nvis; cval = as_f32(nval); cmeta = nmeta;
                ++d;
                if ((uint32_t)j == d) { mynode = cur; myvis = cvis; myval = cval; }
            }
        }
        const uint32_t state = cmeta & kVStateMask, nc = cmeta >> kVCreatedShift;
        int winner;
        const bool fin = finished(state, winner);
        const bool hit = run && fin, grow = run && !fin;
        if (run) { cnt[kVcIterations] += 1u; cnt[kVcDepthSum] += d; }

        // ---- expand (node.rs:118-137): expandable_moves.pop() is the highest empty cell not yet taken -----------------------------------------
        const uint32_t em = empty_cells(state);
        const uint32_t child = apply_move(state, kth_cell(em, __builtin_popcount(em) - 1 - (int)nc));

        // ---- simulate (node.rs:176-196) from the child -----------------------------------------------------------------------------------
        float res = hit ? result_for(winner, player) : 0.0f;
        if (P.quirks != 0u) {                                        // Q22: the loop looks at the node's own state and plays nothing
            int w0;
            if (finished(child, w0) && grow && P.round_limit > 0u) { res = result_for(w0, player); cnt[kVcDecided] += 1u; }
        } else {
            const uint64_t ub = __builtin_bit_cast(uint64_t, uniform_of(P.seed, game, round, kTagVanillaTtt, (it << 12) | (1u + (uint32_t)j)));
            const uint32_t ulo = (uint32_t)ub, uhi = (uint32_t)(ub >> 32);
            uint32_t sim = child;
            bool live = grow;
#pragma unroll
            for (int p = 0; p < 9; ++p) {                            // a child has at most 8 empty cells: look p = 8 finds a full board at the latest
                const uint64_t up = ((uint64_t)row_get(uhi, row0 + p) << 32) | row_get(ulo, row0 + p);
                int w1;
                const bool f1 = finished(sim, w1);
                live = live && (uint32_t)p < P.round_limit;
                if (live && f1) { res = result_for(w1, player); cnt[kVcDecided] += 1u; live = false; }
                if (live) {
                    const uint32_t e1 = empty_cells(sim);
                    const int k1 = __builtin_popcount(e1);
                    int idx = (int)(__builtin_bit_cast(double, up) * (double)k1);
                    idx = idx > k1 - 1 ? k1 - 1 : idx;
                    sim = apply_move(sim, kth_cell(e1, idx));
                    cnt[kVcPlies] += 1u;
                }
            }
        }

        // ---- backpropagate (simple_mcts.rs:96-103): the same sign at every level; stores only ------------------------------------------------
        if (hit) {
            cnt[kVcTerminal] += 1u;
            if ((uint32_t)j <= d) *(u32x2*)(tree + mynode * kVNodeWords) = u32x2{myvis + 1u, as_u32(myval + res)};
        }
        if (grow && used >= cap) overflow = 1u;                      // (the slab holds a node per iteration by construction)
        else if (grow) {
            const uint32_t ci = used++;
            cnt[kVcExpansions] += 1u; cnt[kVcRollouts] += 1u;
            if ((uint32_t)j <= d) *(u32x2*)(tree + mynode * kVNodeWords) = u32x2{myvis + 1u, as_u32(myval + res)};
            if ((uint32_t)j == d) {
                tree[mynode * kVNodeWords + 2u] = cmeta + (1u << kVCreatedShift);
                tree[mynode * kVNodeWords + 3u + nc] = ci;
            }
            if ((uint32_t)j == d + 1u) *(u32x4*)(tree + ci * kVNodeWords) = u32x4{1u, as_u32(res), child, 0u};
        }
        row_sync();
    }

    if (P.it1 < P.iterations) {
        if (!LDS && valid && j == 0) {
            VanillaGame* G = P.games + g;
            G->used = used | overflow << 31;
#pragma unroll
            for (int i = 0; i < kVcCount; ++i) G->cnt[i] = cnt[i];
        }
        return;
    }
    // ---- the answer (simple_mcts.rs:71-86): the root's most visited child, the last created of equal ones ---------------------------------------
    const uint32_t nc = valid ? (*(const u32x4*)tree).z >> kVCreatedShift : 0u;
    uint32_t vis = 0u, cstate = root_state;
    float val = 0.0f;
    if ((uint32_t)j < nc) {
        uint32_t ci = tree[3u + (uint32_t)j];
        ci = ci < used ? ci : used - 1u;
        const u32x4 h = *(const u32x4*)(tree + ci * kVNodeWords);
        vis = h.x; val = as_f32(h.y); cstate = h.z & kVStateMask;
    }
    const uint32_t mine = (uint32_t)__builtin_ctz((empty_cells(root_state) & ~empty_cells(cstate)) | 0x200u);    // the cell the child filled
    int best = 0;
    uint32_t bv = row_get(vis, row0);
#pragma unroll
    for (int jj = 1; jj < 9; ++jj) {
        const uint32_t vv = row_get(vis, row0 + jj);
        if ((uint32_t)jj < nc && vv >= bv) { best = jj; bv = vv; }
    }
    const uint32_t move = row_get(mine, row0 + best);
    if (valid) {
        VanillaOut* O = P.out + gi;
        if (j < 9) { O->child_visits[j] = (float)vis; O->child_values[j] = val; }
        if (j == 0) {
            O->move = nc != 0u ? move : 10u;
            O->n_children = nc; O->overflow = overflow; O->pad = 0u;
#pragma unroll
            for (int i = 0; i < kVcCount; ++i) O->cnt[i] = cnt[i];
        }
    }
}

void launch_ttt_vanilla(hipStream_t st, const VanillaParams& P) {
    if (P.n == 0) return;
    const uint32_t groups = P.n / kB + (P.n % kB != 0);
    if (P.nodes == nullptr) hipLaunchKernelGGL(k_ttt_vanilla<true>, dim3(groups), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(k_ttt_vanilla<false>, dim3(groups), dim3(256), 0, st, P);
}

}  // namespace ttt
}  // namespace diee
