// vanilla_kernels.hip -- Agent::Mcts (mct_search, src/mcts/simple_mcts.rs:10-39; Node, src/mcts/node.rs) on the device for gfx950:
// vanilla UCB1 search with random rollouts, one wavefront per game.
//
// The search is the reference's, iteration by iteration (select, expand one child, simulate, backpropagate); how it is stored is not:
// a game's tree is a slab of iterations + 1 nodes in HBM (search_types.h, Vanilla), a node's play list is not kept -- it is a function of
// the node's state and is enumerated again when the node is expanded (bg_legal_plays_wave) --, and a rollout ply is one more such
// enumeration on a state held in registers.  The engine's choices where the reference leaves the agent open (a root or a node without a
// legal play, ln from a host-built table, the rollout as it was meant when DIEE_FLAG_REF_QUIRKS is off) are listed in include/diee.h.
// A launch runs at most Vanilla::budget iterations per game and leaves everything it knows in the slab; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bg_device.h"
#include "launch.h"
#include "mcts_device.h"
#include "search_iter_device.h"
#include "search_types.h"
#include "wave_ops.h"

namespace diee {

namespace {

// draw_dice and draw_uniform of ONE counter (seed, game, round, kTagVanilla, ord): the same bits as the two calls, one Philox block
struct VanillaDraw { int d0, d1; double u; };
__device__ __forceinline__ VanillaDraw vanilla_draw(unsigned long long seed, uint32_t game, uint32_t round, uint32_t ord) {
    uint32_t o[4];
    philox4x32((uint32_t)seed, (uint32_t)(seed >> 32), game, round, kTagVanilla, ord, o);
    VanillaDraw d;
    d.d0 = 1 + (int)(((uint64_t)o[0] * 6ull) >> 32);
    d.d1 = 1 + (int)(((uint64_t)o[1] * 6ull) >> 32);
    const uint64_t x = ((uint64_t)o[3] << 32) | o[2];
    d.u = (double)(x >> 11) * (1.0 / 9007199254740992.0);
    return d;
}

// ucb (node.rs:86-96) over the children of one node, one child per lane and 64 links of the list per pass: the child among those of
// index above `floor` with the largest score, the last created of equal ones; *lastnan = the last created child whose score is NaN
__device__ __forceinline__ Best vanilla_level(const Vanilla& V, size_t base, uint32_t head, float cl, int floor, int lane, int* lastnan) {
    Best b{0.0f, -1};
    int ln = -1;
    uint32_t cur = head;
    while (cur != kVanillaUnknown) {
        uint32_t mine = kVanillaUnknown;
        for (int q = 0; q < 64 && cur != kVanillaUnknown; ++q) {     // (uniform: every lane follows the same links)
            if (lane == q) mine = cur;
            cur = V.next[base + cur];
        }
        if (mine != kVanillaUnknown && (int)mine > floor) {
            const float v = (float)V.visits[base + mine], w = V.value[base + mine];
            const float q = w / v;
            const float e = sqrtf(cl / v);
            const float s = q + e;
            if (s != s) ln = ln > (int)mine ? ln : (int)mine;
            else if (b.j < 0 || s > b.s || (s == b.s && (int)mine > b.j)) { b.s = s; b.j = (int)mine; }
        }
    }
    *lastnan = wave_allmax_i32(ln);
    return b;
}

}  // namespace

// Node::new for the roots (node.rs:24-41): a root that is a finished game, or has no legal play, runs no iteration (EMPTY_MOVE)
__global__ __launch_bounds__(64) void k_vanilla_init(Vanilla V, uint32_t n) {
    __shared__ WaveScratch sc;
    const uint32_t slot = blockIdx.x;
    if (slot >= n) return;
    const int lane = threadIdx.x;
    const size_t base = (size_t)slot * V.node_cap;
    const BgState s = load_state(&V.roots[slot]);
    int k = 0;
    if (bg_winner_dev(s) == 0) {
        k = bg_legal_plays_wave(s, &sc, lane, V.overflow);
        if (k > kMaxPlays) { if (lane == 0) atomicOr(V.overflow, 1u); k = 0; }      // never silent: DIEE_ERR_CAPACITY
    }
    if (lane != 0) return;
    store_state(&V.state[base], s);
    V.parent[base] = kVanillaUnknown; V.nplays[base] = (uint32_t)k; V.ncreated[base] = 0; V.visits[base] = 0; V.value[base] = 0.0f;
    V.play[base] = pack_play(kNoMove, kNoMove, kNoMove, kNoMove); V.head[base] = kVanillaUnknown; V.next[base] = kVanillaUnknown;
    V.done[slot] = k > 0 ? 0u : kVanillaUnknown;
    V.used[slot] = 1;
}

// up to V.budget iterations of mct_search (simple_mcts.rs:17-37) for one game
__global__ __launch_bounds__(64) void k_vanilla(Vanilla V, uint32_t n) {
    __shared__ WaveScratch sc;
    const uint32_t slot = blockIdx.x;
    if (slot >= n) return;
    const int lane = threadIdx.x;
    uint32_t it = V.done[slot];
    if (it == kVanillaUnknown || it >= V.iterations) return;
    const size_t base = (size_t)slot * V.node_cap;
    const uint32_t end = V.iterations - it > V.budget ? it + V.budget : V.iterations;
    const uint32_t game = V.game_id[slot], round = V.round[slot];
    const int player = st_player(load_state(&V.state[base]));
    uint32_t used = V.used[slot];
    uint32_t cn[VC_COUNT];
#pragma unroll
    for (int i = 0; i < VC_COUNT; ++i) cn[i] = 0;
    bool full = false;                                          // a capacity flag was raised: the call fails, the game stops
    for (; it < end && !full; ++it) {
        // select (simple_mcts.rs:88-94): down while the node has children and no unexpanded play
        uint32_t node = 0, depth = 0;
        uint32_t nc = V.ncreated[base], np = V.nplays[base];
        while (nc != 0 && nc == np) {
            const float cl = V.c * V.ln[V.visits[base + node]];
            const uint32_t head = V.head[base + node];
            int lastnan;
            Best b = vanilla_level(V, base, head, cl, -1, lane, &lastnan);
            if (lastnan >= 0) {                                 // NaN compares Equal: the fold restarts behind the last one
                int none;
                b = vanilla_level(V, base, head, cl, lastnan, lane, &none);
            }
            b = wave_best(b);
            node = (uint32_t)(b.j >= 0 ? b.j : lastnan);
            ++depth;
            nc = V.ncreated[base + node]; np = V.nplays[base + node];
        }
        ++cn[VC_ITERATIONS];
        cn[VC_DEPTH_SUM] += depth;
        const BgState s = load_state(&V.state[base + node]);
        uint32_t from = node;
        float res = 0.0f;
        const int w = bg_winner_dev(s);
        if (w != 0) {                                           // simple_mcts.rs:25-30
            res = w == player ? 1.0f : -1.0f;
            ++cn[VC_TERMINAL];
        } else {
            const int k = bg_legal_plays_wave(s, &sc, lane, V.overflow);
            if (k > kMaxPlays || (k > 0 && (nc >= (uint32_t)k || used >= V.node_cap))) {
                if (lane == 0) atomicOr(V.overflow, k > kMaxPlays ? 1u : 2u);
                full = true;
                break;
            }
            if (np == kVanillaUnknown && lane == 0) V.nplays[base + node] = (uint32_t)k;
            BgState sim = s;
            if (k == 0) {
                ++cn[VC_DEAD_END];                              // no child: the rollout's first ply is this node's skip
            } else {                                            // expand (node.rs:118-137): expandable_moves.pop()
                const uint32_t pl = sc.play[(uint32_t)k - 1u - nc];
                const VanillaDraw d = vanilla_draw(V.seed, game, round, it << 12);
                bg_apply_dev(sim, pl, d.d0, d.d1);
                const uint32_t ci = used++;
                if (lane == 0) {
                    const size_t c = base + ci;
                    store_state(&V.state[c], sim);
                    V.parent[c] = node; V.nplays[c] = kVanillaUnknown; V.ncreated[c] = 0; V.visits[c] = 0; V.value[c] = 0.0f;
                    V.play[c] = pl; V.head[c] = kVanillaUnknown; V.next[c] = V.head[base + node];
                    V.head[base + node] = ci; V.ncreated[base + node] = nc + 1;
                }
                from = ci;
                ++cn[VC_EXPANSIONS];
            }
            // simulate (node.rs:176-196)
            ++cn[VC_ROLLOUTS];
            if (V.quirks) {                                     // Q22: the loop looks at the node's own state and plays nothing
                const int w0 = bg_winner_dev(sim);
                if (V.round_limit > 0 && w0 != 0) { res = w0 == player ? 1.0f : -1.0f; ++cn[VC_DECIDED]; }
            } else {
                for (uint32_t p = 0; p < V.round_limit; ++p) {
                    const int w1 = bg_winner_dev(sim);
                    if (w1 != 0) { res = w1 == player ? 1.0f : -1.0f; ++cn[VC_DECIDED]; break; }
                    const int k1 = bg_legal_plays_wave(sim, &sc, lane, V.overflow);
                    if (k1 > kMaxPlays) { if (lane == 0) atomicOr(V.overflow, 1u); full = true; break; }
                    const VanillaDraw d = vanilla_draw(V.seed, game, round, (it << 12) | (1u + p));
                    if (k1 > 0) {
                        int idx = (int)(d.u * (double)k1);
                        if (idx > k1 - 1) idx = k1 - 1;
                        bg_apply_dev(sim, sc.play[idx], d.d0, d.d1);
                    } else {
                        bg_skip_dev(sim, d.d0, d.d1);
                    }
                    ++cn[VC_PLIES];
                }
                if (full) break;
            }
        }
        // backpropagate (simple_mcts.rs:96-103): the same sign at every level
        __syncthreads();                                        // the new child's record
        for (uint32_t i = from; i != kVanillaUnknown; i = V.parent[base + i])
            if (lane == 0) { V.visits[base + i] += 1u; V.value[base + i] += res; }
        __syncthreads();
    }
    if (lane != 0) return;
    V.done[slot] = full ? kVanillaUnknown : it;
    V.used[slot] = used;
#pragma unroll
    for (int i = 0; i < VC_COUNT; ++i) V.counters[(size_t)slot * VC_COUNT + i] += cn[i];
}

// the answer (simple_mcts.rs:71-86): the root's most visited child, the last created of equal ones; the children's statistics in creation order
__global__ void k_vanilla_result(Vanilla V, uint32_t n, uint32_t* n_children, float* child_visits, float* child_values, uint32_t cap) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    const size_t base = (size_t)slot * V.node_cap;
    const uint32_t nc = V.ncreated[base];
    uint32_t play = pack_play(kNoMove, kNoMove, kNoMove, kNoMove), best_v = 0, best_i = 0;
    uint32_t j = nc;                                            // the list starts at the child created last
    for (uint32_t cur = V.head[base]; cur != kVanillaUnknown && j > 0; cur = V.next[base + cur]) {
        --j;
        const uint32_t v = V.visits[base + cur];
        if (best_i == 0 || v > best_v || (v == best_v && cur > best_i)) { best_v = v; best_i = cur; play = V.play[base + cur]; }
        if (j < cap) {
            if (child_visits) child_visits[(size_t)slot * cap + j] = (float)v;
            if (child_values) child_values[(size_t)slot * cap + j] = V.value[base + cur];
        }
    }
    V.out_play[slot] = play;
    if (n_children) n_children[slot] = nc;
}

// the list of the arena's side about to search -> the roots and RNG keys of its search (game ids = game index, rounds = the call's round)
__global__ void k_vanilla_gather(Arena A, uint32_t side, uint32_t n, uint32_t round, BgState* roots, uint32_t* game_id, uint32_t* rounds) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    const uint32_t g = A.list[(size_t)side * A.n_games + slot];
    store_state(&roots[slot], load_state(&A.state[g]));
    game_id[slot] = g;
    rounds[slot] = round;
}

// ---- host launchers -----------------------------------------------------------------------------
void launch_vanilla_init(hipStream_t st, const Vanilla& V, uint32_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_vanilla_init, dim3(n), dim3(64), 0, st, V, n);
}
void launch_vanilla(hipStream_t st, const Vanilla& V, uint32_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_vanilla, dim3(n), dim3(64), 0, st, V, n);
}
void launch_vanilla_result(hipStream_t st, const Vanilla& V, uint32_t n, uint32_t* n_children, float* child_visits, float* child_values,
                           uint32_t cap) {
    if (!n) return;
    hipLaunchKernelGGL(k_vanilla_result, dim3((n + 63) / 64), dim3(64), 0, st, V, n, n_children, child_visits, child_values, cap);
}
void launch_vanilla_gather(hipStream_t st, const Arena& A, uint32_t side, uint32_t n, uint32_t round, BgState* roots, uint32_t* game_id,
                           uint32_t* rounds) {
    if (!n) return;
    hipLaunchKernelGGL(k_vanilla_gather, dim3((n + 255) / 256), dim3(256), 0, st, A, side, n, round, roots, game_id, rounds);
}

}  // namespace diee
