// selfplay_kernels.hip -- the bookkeeping of self-play around a move-step's search (search_types.h, Games): the games of a call and their
// records, the live list, slot refill, output delivery.  Reference: self_play_parallel, src/alphazero/alpha_parallel.rs:101-231.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bg_device.h"
#include "launch.h"
#include "mcts_device.h"
#include "search_types.h"

namespace diee {

// ---- self-play -----------------------------------------------------------------------------------
// alpha_parallel.rs:103-111: T::new() + roll_die for every game of every batch
__global__ void k_init_games(Games Gm, Segs G, uint32_t n) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    uint32_t seg = 0;
    while (seg + 1 < G.n && g >= G.game0[seg + 1]) ++seg;
    BgState s;
    // Backgammon::new, backgammon_logic.rs:80-94
    s.w[0] = 0x00000002u; s.w[1] = 0xFD00FB00u; s.w[2] = 0x05000000u; s.w[3] = 0x000000FBu;
    s.w[4] = 0x00050003u; s.w[5] = 0xFE000000u; s.w[6] = 0u;
    int d0, d1;
    draw_dice(G.seed[seg], G.first_id[seg] + (g - G.game0[seg]), 0u, kTagInitRoll, 0u, d0, d1);
    s.w[7] = (uint32_t)d0 | ((uint32_t)d1 << 8) | (0xFFu << 16);
    store_state(&Gm.state[g], s);
    Gm.rounds[g] = 0; Gm.nfrags[g] = 0; Gm.alive[g] = 1; Gm.winner[g] = 0;
    Gm.ev_a_count[g] = kNone; Gm.ev_b_count[g] = kNone; Gm.ev_a_step[g] = 0; Gm.ev_b_step[g] = 0;
    Gm.live[g] = g; Gm.seg[g] = (uint8_t)seg;
}

// live games -> slots; the live list is ascending in the game index, so the slots of a batch are contiguous: the
// slot whose predecessor belongs to another batch is the batch's first (the reference's index 0), likewise its end
__global__ void k_gather_roots(Games Gm, Slots S, Segs G, uint32_t n_live) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_live) return;
    const uint32_t g = Gm.live[slot];
    const uint32_t seg = Gm.seg[g];
    store_state(&S.roots[slot], load_state(&Gm.state[g]));
    S.game_id[slot] = G.first_id[seg] + (g - G.game0[seg]);
    S.round[slot] = Gm.rounds[g];
    S.seg[slot] = seg;
    if (slot == 0 || Gm.seg[Gm.live[slot - 1]] != seg) G.first_slot[seg] = slot;
    if (slot + 1 == n_live || Gm.seg[Gm.live[slot + 1]] != seg) G.end_slot[seg] = slot + 1;
}

// the body of the per-game loop of self_play_parallel, alpha_parallel.rs:168-224
__global__ __launch_bounds__(64) void k_play_move(Tree T, Games Gm, Segs G, uint32_t n_live, uint32_t step, PlayParams P) {
    __shared__ float row[1352];
    const uint32_t slot = blockIdx.x;
    if (slot >= n_live) return;
    const int lane = threadIdx.x;
    const uint32_t g = Gm.live[slot];
    const size_t base = (size_t)slot * T.node_cap;
    const uint32_t k = meta_nch(T.meta[base]), fc = T.first_child[base];
    BgState s = load_state(&Gm.state[g]);
    const uint32_t round = Gm.rounds[g];
    const uint32_t seg = Gm.seg[g];
    const uint32_t gid = G.first_id[seg] + (g - G.game0[seg]);
    const unsigned long long seed = G.seed[seg];
    unsigned long long* cnt = Gm.counters + (size_t)seg * CNT_COUNT;
    bool removed = false, flushed = false;
    if (round >= P.round_limit) {                               // :172-180 (no `continue`)
        if (lane == 0) { Gm.ev_a_count[g] = Gm.nfrags[g]; Gm.ev_a_step[g] = step; }
        removed = true; flushed = true;
    }
    if (k == 0) {                                               // :183-189 skip_turn
        if (lane == 0) {
            int d0, d1;
            draw_dice(seed, gid, round, kTagMoveRoll, 0u, d0, d1);
            bg_skip_dev(s, d0, d1);
            store_state(&Gm.state[g], s);
            Gm.rounds[g] = round + 1;
            if (removed) { Gm.alive[g] = 0; atomicAdd(&cnt[CNT_GAMES], 1ull); }
            atomicAdd(&cnt[CNT_PLIES], 1ull);
        }
        return;
    }
    // get_prob_tensor_parallel row (:164), pow_(1/T) (:165) and weighted_select_tensor_idx (:200): the chain the arena's move kernel shares
    const uint32_t code = sample_root_move(T, base, k, fc, row, lane, P.inv_temperature, seed, gid, round);
    // MemoryFragment{outcome: player, ps, state} (:195-199)
    const uint32_t nf = Gm.nfrags[g];
    const size_t fi = (size_t)(Gm.area ? Gm.area[g] : g) * Gm.frag_cap + nf;
    for (int a = lane; a < 1352; a += 64) Gm.frag_ps[fi * 1352 + a] = row[a];
    for (int t = lane; t < 144; t += 64) Gm.frag_planes[fi * 144 + t] = bg_plane_dev(s, t / 24, t % 24);
    if (lane == 0) {
        Gm.frag_player[fi] = (int8_t)st_player(s);
        Gm.nfrags[g] = nf + 1;
        // decode + apply_move (:202-210); legality of decode(code) is checked when the root is expanded
        const uint32_t play = bg_decode_dev(st_roll(s, 0), st_roll(s, 1), st_player(s), code);
        int d0, d1;
        draw_dice(seed, gid, round, kTagMoveRoll, 0u, d0, d1);
        bg_apply_dev(s, play, d0, d1);
        store_state(&Gm.state[g], s);
        Gm.rounds[g] = round + 1;                               // :213
        atomicAdd(&cnt[CNT_PLIES], 1ull);
        const int w = bg_winner_dev(s);
        if (w != 0) {                                           // :215-223
            if (!(flushed && !P.quirks)) { Gm.ev_b_count[g] = nf + 1; Gm.ev_b_step[g] = step; }
            Gm.winner[g] = (int8_t)w;
            removed = true;
        }
        if (removed) { Gm.alive[g] = 0; atomicAdd(&cnt[CNT_GAMES], 1ull); }
    }
}

// stable compaction of the live list (one block); n_live_out[0] = games alive, [1 + b] = alive in batch b
__global__ __launch_bounds__(1024) void k_compact_live(Games Gm, uint32_t n_live, uint32_t n_segs, uint32_t* n_live_out) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    __shared__ uint32_t per_seg[kMaxSegments];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    if (tid < (int)kMaxSegments) per_seg[tid] = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_live; c0 += 1024) {
        const uint32_t i = c0 + tid;
        uint32_t g = 0;
        bool keep = false;
        if (i < n_live) { g = Gm.live[i]; keep = Gm.alive[g] != 0; }
        if (keep) atomicAdd(&per_seg[Gm.seg[g]], 1u);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = carry;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const uint32_t pos = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();                                        // all reads of live[c0..] done before writes
        if (keep) Gm.live[pos] = g;
        __syncthreads();
        if (tid == 0) { uint32_t t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; carry += t; }
        __syncthreads();
    }
    if (tid == 0) n_live_out[0] = carry;
    if (tid < (int)n_segs) n_live_out[1 + tid] = per_seg[tid];
}

// ---- slot refill (diee_self_play_refill) ------------------------------------------------------------------------------------------
// At most `width` games are in flight; a retired game's slot is taken, in the next move-step, by the next unstarted game.  Every unstarted
// index is above every live one, so appending keeps the live list ascending (k_gather_roots needs that).  The fragments of a game live in
// record area Gm.area[g]; fr = { count, stack[width] } holds the areas nobody owns.
// k_refill_release (one block; behind k_deliver_scan, before k_compact_live drops them from the list): the areas of this step's retired games,
// in the live list's order
__global__ __launch_bounds__(1024) void k_refill_release(Games Gm, uint32_t n_live, uint32_t* __restrict__ fr, uint32_t fr_cap) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = fr[0];
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_live; c0 += 1024) {
        const uint32_t i = c0 + tid;
        uint32_t g = 0;
        bool dead = false;
        if (i < n_live) { g = Gm.live[i]; dead = Gm.alive[g] == 0; }
        const unsigned long long bal = __ballot(dead);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = carry;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const uint32_t pos = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (dead && pos < fr_cap) fr[1 + pos] = Gm.area[g];
        __syncthreads();
        if (tid == 0) { uint32_t t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; carry += t; }
        __syncthreads();
    }
    if (tid == 0) fr[0] = carry < fr_cap ? carry : fr_cap;
}
// k_refill_admit (one block; behind k_compact_live, which left the games alive in n_live_out[0]): games next, next + 1, ... join the live list
// until `width` are in flight or none is left, each on an area off the stack.  The host derives the same count from the same three numbers.
__global__ __launch_bounds__(1024) void k_refill_admit(Games Gm, const uint32_t* __restrict__ n_live_out, uint32_t width, uint32_t next,
                                                       uint32_t total, uint32_t* __restrict__ fr) {
    const uint32_t c = n_live_out[0], fn = fr[0];
    uint32_t add = width > c ? width - c : 0u;
    if (add > total - next) add = total - next;
    if (add > fn) add = fn;                                     // (every game in flight owns one of `width` areas: fn == width - c)
    __syncthreads();                                            // fr[0] read by all before it changes
    for (uint32_t i = threadIdx.x; i < add; i += 1024) {
        const uint32_t g = next + i;
        Gm.live[c + i] = g;
        Gm.area[g] = fr[fn - i];                                // stack[fn - 1 - i]
    }
    if (threadIdx.x == 0) fr[0] = fn - add;
}

// ---- output delivery (alpha_parallel.rs:172-180, :215-223: `all_memories.append(...)` in the step a game is removed) ----
// One block lists the flushes of this move-step in the live list's order (ascending game, hence batch-major; the round-limit
// flush of a game before its win flush) and gives each the row it starts at in its batch's output of the step.  Runs behind
// k_play_move, before k_compact_live drops the removed games from the list.  summary: DeliverSummary.
__global__ __launch_bounds__(1024) void k_deliver_scan(Games Gm, Segs G, uint32_t n_live, uint32_t step, DeliverEvent* __restrict__ ev,
                                                       uint32_t* __restrict__ summary) {
    __shared__ uint32_t wrow[16], wev[16];
    __shared__ uint32_t carry_rows, carry_ev;
    __shared__ uint32_t seg_base[kMaxSegments], seg_rows[kMaxSegments], seg_ev0[kMaxSegments], seg_nev[kMaxSegments];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { carry_rows = 0; carry_ev = 0; }
    if (tid < (int)kMaxSegments) { seg_base[tid] = 0; seg_rows[tid] = 0; seg_ev0[tid] = kNone; seg_nev[tid] = 0; }
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_live; c0 += 1024) {
        const uint32_t i = c0 + tid;
        uint32_t g = 0, seg = 0, ca = 0, cb = 0;
        if (i < n_live) {
            g = Gm.live[i]; seg = Gm.seg[g];
            const uint32_t a = Gm.ev_a_count[g], b = Gm.ev_b_count[g];
            if (a != kNone && Gm.ev_a_step[g] == step) ca = a;
            if (b != kNone && Gm.ev_b_step[g] == step) cb = b;
        }
        const uint32_t nr = ca + cb, ne = (ca ? 1u : 0u) + (cb ? 1u : 0u);
        uint32_t pr = nr, pe = ne;                              // inclusive scans inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t xr = __shfl_up(pr, d, 64), xe = __shfl_up(pe, d, 64);
            if (lane >= d) { pr += xr; pe += xe; }
        }
        if (lane == 63) { wrow[wave] = pr; wev[wave] = pe; }
        __syncthreads();
        uint32_t off_r = carry_rows, off_e = carry_ev;
        for (int w = 0; w < wave; ++w) { off_r += wrow[w]; off_e += wev[w]; }
        const uint32_t row0 = off_r + pr - nr;                  // rows delivered by the slots before this one (all batches)
        uint32_t e = off_e + pe - ne;
        if (i < n_live && i == G.first_slot[seg]) seg_base[seg] = row0;
        if (ca) { ev[e] = DeliverEvent{g, ca, row0, seg}; ++e; }
        if (cb) ev[e] = DeliverEvent{g, 0x80000000u | cb, row0 + ca, seg};
        __syncthreads();
        if (tid == 0) { uint32_t tr = 0, te = 0; for (int w = 0; w < 16; ++w) { tr += wrow[w]; te += wev[w]; } carry_rows += tr; carry_ev += te; }
        __syncthreads();
    }
    const uint32_t n_ev = carry_ev;
    for (uint32_t e = tid; e < n_ev; e += 1024) {               // rows relative to the batch's first this step
        DeliverEvent d = ev[e];
        d.row0 -= seg_base[d.seg];
        ev[e] = d;
        atomicAdd(&seg_rows[d.seg], d.kind_count & 0x7FFFFFFFu);
        atomicMin(&seg_ev0[d.seg], e);
        atomicAdd(&seg_nev[d.seg], 1u);
    }
    __syncthreads();
    if (tid < (int)G.n) {
        summary[DeliverSummary::rows(G.n, tid)] = seg_rows[tid];
        summary[DeliverSummary::ev0(G.n, tid)] = seg_nev[tid] ? seg_ev0[tid] : 0u;
        summary[DeliverSummary::nev(G.n, tid)] = seg_nev[tid];
    }
}

// rows [r0, r1) of one batch's output of the step -> staging rows [0, r1 - r0): ps and planes as the game recorded them,
// outcome relabelled (:216-217: +1 where the fragment's mover won, -1 where the opponent did; 0 for a round-limit flush),
// the originating game id.  ev = the batch's n_ev events (ascending row0).
__global__ __launch_bounds__(256) void k_deliver_copy(Games Gm, Segs G, const DeliverEvent* __restrict__ ev, uint32_t n_ev, uint32_t r0,
                                                      uint32_t r1, DeliverOut out) {
    for (uint32_t r = r0 + blockIdx.x; r < r1; r += gridDim.x) {
        uint32_t lo = 0, hi = n_ev;                             // last event with row0 <= r
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (ev[mid].row0 <= r) lo = mid; else hi = mid; }
        const DeliverEvent d = ev[lo];
        const uint32_t fr = r - d.row0;
        const size_t s = (size_t)(Gm.area ? Gm.area[d.g] : d.g) * Gm.frag_cap + fr, o = (size_t)(r - r0);
        for (int a = threadIdx.x; a < 1352 / 4; a += 256)
            reinterpret_cast<float4*>(out.ps + o * 1352)[a] = reinterpret_cast<const float4*>(Gm.frag_ps + s * 1352)[a];
        if (threadIdx.x < 144 / 4)
            reinterpret_cast<float4*>(out.planes + o * 144)[threadIdx.x] = reinterpret_cast<const float4*>(Gm.frag_planes + s * 144)[threadIdx.x];
        if (threadIdx.x == 0) {
            const int pl = Gm.frag_player[s], w = Gm.winner[d.g];
            out.outcome[o] = (d.kind_count >> 31) == 0 ? (int8_t)0 : (int8_t)(w == pl ? 1 : (w == -pl ? -1 : 0));
            out.game[o] = G.first_id[d.seg] + (d.g - G.game0[d.seg]);
        }
    }
}

// ---- host launchers -----------------------------------------------------------------------------
void launch_init_games(hipStream_t st, const Games& Gm, const Segs& G, uint32_t n) {
    hipLaunchKernelGGL(k_init_games, dim3((n + 255) / 256), dim3(256), 0, st, Gm, G, n);
}
void launch_gather_roots(hipStream_t st, const Games& Gm, const Slots& S, const Segs& G, uint32_t n_live) {
    hipLaunchKernelGGL(k_gather_roots, dim3((n_live + 255) / 256), dim3(256), 0, st, Gm, S, G, n_live);
}
void launch_play_move(hipStream_t st, const Tree& T, const Games& Gm, const Segs& G, uint32_t n_live, uint32_t step, const PlayParams& P) {
    hipLaunchKernelGGL(k_play_move, dim3(n_live), dim3(64), 0, st, T, Gm, G, n_live, step, P);
}
void launch_compact_live(hipStream_t st, const Games& Gm, uint32_t n_live, uint32_t n_segs, uint32_t* n_live_out) {
    hipLaunchKernelGGL(k_compact_live, dim3(1), dim3(1024), 0, st, Gm, n_live, n_segs, n_live_out);
}
void launch_refill_release(hipStream_t st, const Games& Gm, uint32_t n_live, uint32_t* fr, uint32_t fr_cap) {
    hipLaunchKernelGGL(k_refill_release, dim3(1), dim3(1024), 0, st, Gm, n_live, fr, fr_cap);
}
void launch_refill_admit(hipStream_t st, const Games& Gm, const uint32_t* n_live_out, uint32_t width, uint32_t next, uint32_t total, uint32_t* fr) {
    hipLaunchKernelGGL(k_refill_admit, dim3(1), dim3(1024), 0, st, Gm, n_live_out, width, next, total, fr);
}
void launch_deliver_scan(hipStream_t st, const Games& Gm, const Segs& G, uint32_t n_live, uint32_t step, DeliverEvent* ev, uint32_t* summary) {
    hipLaunchKernelGGL(k_deliver_scan, dim3(1), dim3(1024), 0, st, Gm, G, n_live, step, ev, summary);
}
void launch_deliver_copy(hipStream_t st, const Games& Gm, const Segs& G, const DeliverEvent* ev, uint32_t n_ev, uint32_t r0, uint32_t r1,
                         const DeliverOut& out) {
    if (r1 <= r0 || !n_ev) return;
    hipLaunchKernelGGL(k_deliver_copy, dim3(std::min<uint32_t>(r1 - r0, 8192u)), dim3(256), 0, st, Gm, G, ev, n_ev, r0, r1, out);
}

}  // namespace diee
