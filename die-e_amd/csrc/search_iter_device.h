// search_iter_device.h -- the ONE copy of a search iteration on a staged tree: what k_tail (lockstep, at most 16 games) and k_free
// (free-running, 17 ... 800 games) of mcts_kernels.hip both run between their own ways of waiting for network rows.  The arithmetic is
// select_slot's / expand_body's (k_expand, mcts_kernels.hip), operation for operation, in the same order per node; the bit-exact suites
// (tests/test_tail_gpu.py, tests/test_free_gpu.py) hold all of it to the oracle.  The tree is reached through an accessor (TreeLds, TreeF):
//   StagedStats                     T, base (the arena in HBM); vis(i) val(i) pri(i); set_stats(i, visits, value); add(i, v)
//   Hdr, hdr(i), nch(h), fc(h)      a node's header: children, first child; h.bits() the expanded / finished-game bits (kDrained, kMetaTerminal,
//                                   kMetaWinnerPlus, in Tree::meta's positions); leaf_meta(i, h) the whole of Tree::meta[i]
//   set_header(i, meta, first_child)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bg_device.h"
#include "mcts_device.h"
#include "nn_device.h"
#include "search_types.h"
#include "wave_ops.h"

namespace diee {

// alpha_ucb (node.rs:98-112): q + (c * (sqrt(N_parent) / (n + 1))) * p, f32, in this association (sq = sqrt(N_parent))
__device__ __forceinline__ float puct_score(float vis, float val, float pr, float sq, float c) {
    const float q = vis == 0.0f ? 0.0f : val / vis;
    const float t = sq / (vis + 1.0f);
    const float u = c * t;
    const float w = u * pr;
    return q + w;
}
// the same rule for a prediction (k_free's virtual descents), not the search: the hardware's approximate reciprocal will do
__device__ __forceinline__ float puct_score_approx(float vis, float val, float pr, float sq, float c) {
    const float q = vis == 0.0f ? 0.0f : val * __builtin_amdgcn_rcpf(vis);
    return q + (c * (sq * __builtin_amdgcn_rcpf(vis + 1.0f))) * pr;
}

struct Best { float s; int j; };
__device__ __forceinline__ Best better(Best a, Best b) {      // later index wins ties (Iterator::max_by)
    if (b.j < 0) return a;
    if (a.j < 0) return b;
    if (a.s > b.s || (a.s == b.s && a.j > b.j)) return a;
    return b;
}

// the best of the wave in every lane; `better` is a symmetric total order, so the pairing order is free (wave_ops.h)
__device__ __forceinline__ Best wave_best(Best b) {
    Best o;
    o.s = dpp_f32<kDppXor1>(b.s); o.j = dpp_i32<kDppXor1>(b.j); b = better(b, o);
    o.s = dpp_f32<kDppXor2>(b.s); o.j = dpp_i32<kDppXor2>(b.j); b = better(b, o);
    o.s = dpp_f32<kDppHalfMirror>(b.s); o.j = dpp_i32<kDppHalfMirror>(b.j); b = better(b, o);
    o.s = dpp_f32<kDppMirror>(b.s); o.j = dpp_i32<kDppMirror>(b.j); b = better(b, o);
    const int si = __builtin_bit_cast(int, b.s);
    Best r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        r[q].s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(si, 16 * q));
        r[q].j = __builtin_amdgcn_readlane(b.j, 16 * q);
    }
    return better(better(r[0], r[1]), better(r[2], r[3]));
}

// a game's statistics through LDS: nodes below `cap` live there (and in HBM, written through), the others in HBM alone
struct StagedStats {
    const Tree& T; size_t base; uint32_t cap;
    float *lvis, *lval, *lpri;
    __device__ __forceinline__ float vis(uint32_t i) const { return i < cap ? lvis[i] : T.visits[base + i]; }
    __device__ __forceinline__ float val(uint32_t i) const { return i < cap ? lval[i] : T.value[base + i]; }
    __device__ __forceinline__ float pri(uint32_t i) const { return i < cap ? lpri[i] : T.prior[base + i]; }
    __device__ __forceinline__ void set_stats(uint32_t i, float nv, float nw) const {
        if (i < cap) { lvis[i] = nv; lval[i] = nw; }
        T.visits[base + i] = nv; T.value[base + i] = nw;
    }
    __device__ __forceinline__ void add(uint32_t i, float v) const { set_stats(i, vis(i) + 1.0f, val(i) + v); }      // visits += 1, value += v (simple_mcts.rs:96-103, one node)
};

// a finished game's value: +-1 for the ROOT's player (alpha_mcts.rs:157-163), from the header's bits
__device__ __forceinline__ float finished_value(uint32_t bits, int root_player) {
    return ((bits & kMetaWinnerPlus) ? 1 : -1) == root_player ? 1.0f : -1.0f;
}

// One level of select_alpha (alpha_mcts.rs:14-33) over the k children at fcn: the index of the last of the equal maxima; NaN compares
// Equal, so the sequential fold restarts after a NaN -- only children after the last NaN compete, and with nothing behind it that NaN wins.
template <class TreeX>
__device__ __forceinline__ uint32_t select_level(const TreeX& X, uint32_t fcn, uint32_t k, float sq, float c, int lane) {
    Best b{0.0f, -1};
    int lastnan = -1;
    for (uint32_t j = lane; j < k; j += 64) {
        const uint32_t ci = fcn + j;
        const float sc_ = puct_score(X.vis(ci), X.val(ci), X.pri(ci), sq, c);
        if (sc_ != sc_) lastnan = (int)j;
        else if (b.j < 0 || !(b.s > sc_)) { b.s = sc_; b.j = (int)j; }
    }
    lastnan = wave_allmax_i32(lastnan);
    if (lastnan >= 0) {
        b.s = 0.0f; b.j = -1;
        for (uint32_t j = lane; j < k; j += 64) {
            if ((int)j <= lastnan) continue;
            const uint32_t ci = fcn + j;
            const float sc_ = puct_score(X.vis(ci), X.val(ci), X.pri(ci), sq, c);
            if (b.j < 0 || !(b.s > sc_)) { b.s = sc_; b.j = (int)j; }
        }
    }
    b = wave_best(b);
    return (uint32_t)(b.j >= 0 ? b.j : lastnan);
}

// the slot's counters to and from registers (SC_ILLEGAL is only ever bumped by atomics in memory: it is not written back)
__device__ __forceinline__ void load_counters(const Slots& S, uint32_t slot, uint32_t (&cn)[SC_COUNT]) {
    static_assert(SC_COUNT == 8, "two 16-byte loads");
    const uint4 a = ((const uint4*)(S.slot_cnt + slot * SC_COUNT))[0], b = ((const uint4*)(S.slot_cnt + slot * SC_COUNT))[1];
    cn[0] = a.x; cn[1] = a.y; cn[2] = a.z; cn[3] = a.w; cn[4] = b.x; cn[5] = b.y; cn[6] = b.z; cn[7] = b.w;
}
__device__ __forceinline__ void store_counters(const Slots& S, uint32_t slot, const uint32_t (&cn)[SC_COUNT]) {
    uint32_t* p = S.slot_cnt + slot * SC_COUNT;
    ((uint4*)p)[0] = make_uint4(cn[0], cn[1], cn[2], cn[3]);
    static_assert(SC_ILLEGAL == 6 && SC_NN_ROWS == 7, "word 6 stays in memory");
    p[4] = cn[4]; p[5] = cn[5]; p[7] = cn[7];
}

// What a slot carries from launch to launch (the record select_slot / k_tail / k_free leave in HBM), in registers from one iteration to the
// next.  `lst`, the selected leaf's state, is the kernel's to request (behind its staging of the tree); the counters are the kernel's to store.
struct SlotRecord {
    uint32_t seg, seg_first, seg_end, gid, rnd;
    unsigned long long seed, evals;
    float rv0, sel_value;
    uint32_t used, leaf, sel, leaf_meta, plen;
    uint32_t pnode;                                         // lane d: the node at depth d of the last real selection's path
    bool lterm;
    int root_player;
    uint32_t cn[SC_COUNT];
    BgState lst;
    __device__ __forceinline__ void load(const Tree& T, const Slots& S, const Segs& G, uint32_t slot, int lane) {
        seg = G.n == 1 ? 0u : S.seg[slot];
        seg_first = G.first_slot[seg]; seg_end = G.end_slot[seg];
        seed = G.seed[seg];
        gid = S.game_id[slot]; rnd = S.round[slot];
        rv0 = S.root_value0[seg];
        evals = S.counters[(size_t)seg * CNT_COUNT + CNT_NN_EVALS];
        used = T.used[slot];
        lterm = S.leaf_term[slot] != 0;
        leaf = S.leaf[slot]; sel = S.sel[slot]; leaf_meta = S.leaf_meta[slot];
        sel_value = S.sel_value[slot];
        plen = S.path_len[slot];
        pnode = S.path[(size_t)slot * kPathCap + lane];
        load_counters(S, slot, cn);
        const BgState rs = load_state(&T.state[(size_t)slot * T.node_cap]);
        root_player = st_player(rs);
    }
    // the record for the next launch (and for whoever reads the slot after the search)
    __device__ __forceinline__ void store(const Tree& T, const Slots& S, uint32_t slot, int lane) const {
        if (lane == 0) {
            S.leaf_term[slot] = lterm ? 1 : 0; S.leaf[slot] = leaf; S.sel[slot] = sel; S.leaf_meta[slot] = leaf_meta;
            S.sel_value[slot] = sel_value; S.path_len[slot] = (uint8_t)plen;
            T.used[slot] = used;
            if (slot == seg_first) S.counters[(size_t)seg * CNT_COUNT + CNT_NN_EVALS] = evals;
            store_state(&S.eval_states[slot], lst);
        }
        if ((uint32_t)lane < plen) S.path[(size_t)slot * kPathCap + lane] = pnode;
    }
};

// the value of an evaluated row at a launch's take-in: the value head's FC + tanh by ONE lane (what a virtual descent that ends on the node adds)
__device__ __forceinline__ float row_value(const float* h, const float* wv) {
    float dot = 0.0f;
    for (int i = 0; i < 72; ++i) dot += h[i] * wv[i];
    return tanhf(dot + wv[72]);
}
// A leaf's network row -- 22 logits per lane, the value features -- as requested BEFORE it is needed: the round trip to where the tower launch
// left it passes while the wave would wait anyway
struct NetRowLoaded { ValueHeadIn vh; float lg[22]; };

// backpropagate (simple_mcts.rs:96-103, same sign at every level) over the recorded root-to-leaf path -- lane d updates the node at depth d:
// every node is touched once, by one lane, the same bits -- or, for a selection deeper than the record holds (len == 0), by one lane
// walking the parents up from `from`
template <class TreeX>
__device__ __forceinline__ void backprop_selection(const TreeX& X, uint32_t len, uint32_t my_node, uint32_t from, float v, int lane) {
    if (len) { if ((uint32_t)lane < len) X.add(my_node, v); }
    else if (lane == 0) { for (uint32_t i = from; i != kNone; i = X.T.parent[X.base + i]) X.add(i, v); }
}

// ---- iteration `it` of one game (expand_body<false, 0>'s operations, in its order) ----
// the LDS scratch of an expansion (lgs may lie over the dedup keys of ws: the play enumeration is done with them by then)
struct IterScratch { WaveScratch* ws; float* lgs; float* raw; uint16_t* code; };
// ifl: the iteration's flag words (any_selected, stale-initial count), (1, 0) where the game does not need them.
// on_child(cl, prior, meta): node cl was created in HBM; the kernel's own LDS copy of it is the kernel's to write.
template <class TreeX, class OnChild>
__device__ __forceinline__ void search_iteration(const Slots& S, SlotRecord& R, const TreeX& X, const NetRowLoaded& pre, const IterScratch& sc,
                                                 uint2 ifl, uint32_t it, uint32_t slot, int lane, bool quirks, OnChild&& on_child) {
    const Tree& T = X.T;
    if (ifl.x == 0u) return;                                // alpha_mcts.rs:170-172 `continue`
    float v = 0.0f;
    if (slot == R.seg_first) R.evals += (unsigned long long)(R.seg_end - R.seg_first);
    if (R.lterm) {
        // the stale slot is backpropagated with its own value again (Q14)
        if (quirks && R.sel != kNone) backprop_selection(X, R.plen, R.pnode, R.sel, R.sel_value, lane);
    } else {
        v = value_head_eval(pre.vh, lane);
        R.sel_value = v;
    }
    const uint32_t m0 = R.lterm ? 0u : R.leaf_meta;
    if (!R.lterm && !(m0 & kDrained)) {
        int k = bg_legal_plays_wave(R.lst, sc.ws, lane, S.overflow);
        if (k > kMaxPlays) { if (lane == 0) atomicOr(S.overflow, 1u); k = 0; }     // never silent: DIEE_ERR_CAPACITY
        const int r0 = st_roll(R.lst, 0), r1 = st_roll(R.lst, 1);
        float smM, smInv;
        softmax_reduce(pre.lg, lane, smM, smInv);
#pragma unroll
        for (int q = 0; q < 22; ++q) sc.lgs[lane + 64 * q] = pre.lg[q];
        __syncthreads();
        for (int j = lane; j < k; j += 64) {
            const uint32_t cd = bg_encode_dev(r0, r1, sc.ws->play[j]);
            sc.raw[j] = softmax_prob(sc.lgs[cd], smM, smInv); sc.code[j] = (uint16_t)cd;
        }
        __syncthreads();
        // row sum, sequential in play order (the oracle's order): every lane runs the same chain on values broadcast from their lanes
        float pr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pr[r] = lane + 64 * r < k ? sc.raw[lane + 64 * r] : 0.0f;
        float sum = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kr = k - 64 * r < 64 ? k - 64 * r : 64;                    // uniform
            for (int j = 0; j < kr; ++j) sum += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pr[r]), j));
        }
        const uint32_t first = R.used;
        if (first + (uint32_t)k > T.node_cap) {
            if (lane == 0) atomicOr(S.overflow, 2u);
        } else {
            const uint32_t e = it + 1u;
            for (int j = lane; j < k; j += 64) {
                const uint32_t cl = first + (uint32_t)j;
                const size_t ci = X.base + cl;
                BgState cs = R.lst;
                int d0, d1;
                draw_dice(R.seed, R.gid, R.rnd, e, (uint32_t)j, d0, d1);      // child dice frozen at creation (Q9), keyed by the GAME's iteration
                bg_apply_dev(cs, sc.ws->play[j], d0, d1);
                store_state(&T.state[ci], cs);
                const float prj = sc.raw[j] / sum;
                const uint32_t cm = (uint32_t)sc.code[j] | meta_terminal_bits(cs);
                T.visits[ci] = 0.0f; T.value[ci] = 0.0f; T.prior[ci] = prj;
                T.parent[ci] = R.leaf; T.first_child[ci] = 0; T.meta[ci] = cm;
                on_child(cl, prj, cm);
            }
            const uint32_t nmeta = kDrained | ((uint32_t)k << 16) | (m0 & kMetaKeep);
            if (lane == 0) X.set_header(R.leaf, nmeta, first);
            R.used = first + (uint32_t)k;
            R.cn[SC_EXPANSIONS] += 1; R.cn[SC_CHILDREN] += (uint32_t)k;
            if ((uint32_t)k > R.cn[SC_MAX_CHILDREN]) R.cn[SC_MAX_CHILDREN] = (uint32_t)k;
        }
        __syncthreads();
    }
    if (!R.lterm) backprop_selection(X, R.plen, R.pnode, R.leaf, v, lane);
    if (quirks && slot == R.seg_first && ifl.y != 0u && lane == 0) {
        // slots still holding the initial 0 index re-backpropagate node 0 = this root with the NN value of its state (Q14)
        float rvis = X.vis(0), rval = X.val(0);
        for (uint32_t i = 0; i < ifl.y; ++i) { rvis += 1.0f; rval += R.rv0; }
        X.set_stats(0, rvis, rval);
    }
    __syncthreads();
}

// The end of a selection: the descent stands on `node` (header h) at `depth`, lane d holding the node of depth d in `mine`.  The path length,
// the counters and either the finished game's +-1 with its backpropagation (returns true; the record keeps the last real selection) or the
// new leaf in the record, its state requested (returns false).  R.sel and the iteration's flag words are the kernel's to publish.
template <class TreeX>
__device__ __forceinline__ bool end_selection(const Slots& S, SlotRecord& R, const TreeX& X, uint32_t node, uint32_t depth, uint32_t mine,
                                              const typename TreeX::Hdr& h, int lane) {
    const uint32_t npl = depth < S.path_cap ? depth + 1u : 0u;              // 0: deeper than the record holds
    R.cn[SC_SELECTIONS] += 1; R.cn[SC_DEPTH_SUM] += depth;
    if (h.bits() & kMetaTerminal) {
        backprop_selection(X, npl, mine, node, finished_value(h.bits(), R.root_player), lane);
        R.cn[SC_TERMINAL] += 1;
        R.lterm = true;
        return true;
    }
    R.lterm = false; R.leaf = node; R.plen = npl; R.pnode = mine;
    R.leaf_meta = X.leaf_meta(node, h);
    R.lst = load_state(&X.T.state[X.base + node]);          // in flight while the kernel publishes the selection
    return false;
}

// A virtual descent: the search's own selection rule (last of equal maxima) run ahead on a scratch copy of visits / value (vvis / vval, nodes
// below nu; everything else of the tree is read in place) to find the rows worth evaluating next.  Heuristic only: which rows a launch carries
// beside the demanded ones never shows in a result -- so EXACT = false (k_free) takes the hardware's approximate reciprocal and square root.
struct VirtualDescent { uint32_t node, depth, mine, bits; };
template <bool EXACT, class TreeX>
__device__ __forceinline__ VirtualDescent virtual_descent(const TreeX& X, const float* vvis, const float* vval, uint32_t nu, float c, int lane) {
    VirtualDescent d{0u, 0u, lane == 0 ? 0u : kNone, 0u};
    for (;;) {
        const typename TreeX::Hdr h = X.hdr(d.node);
        d.bits = h.bits();
        const uint32_t k = X.nch(h);
        if (k == 0) break;
        const uint32_t fcn = X.fc(h);
        const float nv = d.node < nu ? vvis[d.node] : X.T.visits[X.base + d.node];
        const float sq = EXACT ? sqrtf(nv) : __builtin_amdgcn_sqrtf(nv);
        Best b{0.0f, -1};
        for (uint32_t j = lane; j < k; j += 64) {
            const uint32_t ci = fcn + j;
            const float vis = ci < nu ? vvis[ci] : X.T.visits[X.base + ci], val = ci < nu ? vval[ci] : X.T.value[X.base + ci];
            const float sc_ = EXACT ? puct_score(vis, val, X.pri(ci), sq, c) : puct_score_approx(vis, val, X.pri(ci), sq, c);
            if (sc_ == sc_ && (b.j < 0 || !(b.s > sc_))) { b.s = sc_; b.j = (int)j; }
        }
        b = wave_best(b);
        d.node = fcn + (uint32_t)(b.j >= 0 ? b.j : (int)k - 1);
        ++d.depth;
        if ((uint32_t)lane == d.depth) d.mine = d.node;
        if (d.depth >= 63) break;
    }
    return d;
}
// the virtual visit of the descent's path with value x (the scratch copy alone)
__device__ __forceinline__ void virtual_visit(const VirtualDescent& d, float* vvis, float* vval, uint32_t nu, float x, int lane) {
    if ((uint32_t)lane <= d.depth && d.mine < nu) { vvis[d.mine] += 1.0f; vval[d.mine] += x; }
}

}  // namespace diee
