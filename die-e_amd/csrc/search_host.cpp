// search_host.cpp -- host driver of the batched search: the buffers of a ctx, one move-step's search and its dispatch, mcts_batch.
// Reference call structure: alpha_mcts_parallel (src/mcts/alpha_mcts.rs:91-202).  The host only enqueues kernels: per move-step
// there is ONE device->host read (the live-game count, selfplay_host.cpp); the reference crosses the host<->device boundary twice
// per MCTS iteration.
#include "search_host.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "bg_device.h"

namespace diee {

void free_search(SearchBufs* s) { delete s; }

// ---- the buffers (what grows, when, and to max(old, new)) ---------------------------------------------------------------------------
void SearchBufs::Tree::reserve(uint32_t slot_cap, uint32_t nodes) {
    const uint32_t nc = std::max(nodes, node_cap);
    const size_t N = (size_t)slot_cap * nc;
    visits.ensure(N); value.ensure(N); prior.ensure(N);
    parent.ensure(N); first_child.ensure(N); meta.ensure(N); nstate.ensure(N);
    used.ensure(slot_cap);
    node_cap = nc;
}
void SearchBufs::Slots::reserve(uint32_t slots, uint32_t iterations) {
    if (slots > cap) {
        const uint32_t sc = slots;
        roots.ensure(sc); eval_states.ensure(sc); game_id.ensure(sc); round.ensure(sc); seg.ensure(sc);
        leaf.ensure(sc); sel.ensure(sc); sel_value.ensure(sc); leaf_term.ensure(sc);
        path.ensure((size_t)sc * kPathCap); path_len.ensure(sc); leaf_meta.ensure(sc);
        grow_k.ensure(sc); grow_code.ensure((size_t)sc * kMaxPlays);
        row_slot.ensure(sc); slot_row.ensure(sc); n_rows.ensure(4);
        slot_cnt.ensure((size_t)sc * SC_COUNT);
        cap = sc;
    }
    if (!noise.p) {
        noise.ensure((size_t)kMaxSegments * 1352); root_value0.ensure(kMaxSegments);
        counters.ensure((size_t)kMaxSegments * CNT_COUNT); counters_bak.ensure((size_t)kMaxSegments * CNT_COUNT);
    }
    if (!step_log.p) step_log.ensure(2 * (size_t)kStepLog);
    if (iterations + 1 > iter_cap) { iter_flags.ensure((size_t)kMaxSegments * 2 * ((size_t)iterations + 1)); iter_cap = iterations + 1; }
}
diee::Slots SearchBufs::Slots::view(Engine& e) const {
    const NetHeads H = nn_heads(e, (int)cap);      // the network's output buffers, sized for every slot
    return diee::Slots{roots.p, eval_states.p, game_id.p, round.p, seg.p, leaf.p, sel.p, sel_value.p, leaf_term.p,
                       nullptr, H.logits, H.hv, H.wv, noise.p, root_value0.p, iter_flags.p, counters.p, slot_cnt.p, e.flags_dev.p,
                       leaf_meta.p, path.p, path_len.p, grow_k.p, grow_code.p, std::min<uint32_t>(e.opt.path_cap, kPathCap), 0u};
}
void SearchBufs::Segs::reserve() {
    if (noise_host) return;
    seed.ensure(kMaxSegments); first_id.ensure(kMaxSegments); game0.ensure(kMaxSegments);
    span.ensure(2 * kMaxSegments); live_dev.ensure(kLiveWords);
    HIPCHK(hipHostMalloc((void**)&noise_host, sizeof(float) * 2 * kMaxSegments * 1352));
    HIPCHK(hipHostMalloc((void**)&live_host, sizeof(uint32_t) * (kLiveWords + 1)));
}
void reserve_search(Engine& e, uint32_t slots, uint32_t iterations) {
    if (!e.search) e.search = new SearchBufs();
    SearchBufs& B = *e.search;
    const uint32_t per_exp = std::max<uint32_t>(e.opt.nodes_per_expansion, 1);
    B.slots.reserve(slots, iterations);
    B.tree.reserve(B.slots.cap, (iterations + 1) * per_exp + 64);
    B.segs.reserve();
}
int device_cus(Engine& e) {
    int& cus = e.search->cus;
    if (!cus) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, e.device) == hipSuccess) cus = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256; }
    return cus;
}

// ---- the state of a call --------------------------------------------------------------------------------------------------------------
SearchCall::SearchCall(Engine& eng, uint32_t refill_noise_rows) : e(eng), B(*eng.search), noise_rows(refill_noise_rows) {
    HIPCHK(hipMemsetAsync(B.slots.step_log.p, 0, sizeof(unsigned long long) * 2 * kStepLog, e.stream));
}
void SearchCall::stage_noise(diee::Slots& S, uint32_t n_segs, int buf) const {
    // slot refill: no game is past round noise_rows - 1, so later move-steps add nothing to the table
    const bool by_round = noise_rows != 0;
    if (by_round) { S.noise = B.refill.noise_tab.p; S.noise_segs = n_segs; }
    if (!by_round || cur_step < noise_rows)
        HIPCHK(hipMemcpyAsync(by_round ? B.refill.noise_tab.p + (size_t)cur_step * n_segs * 1352 : B.slots.noise.p, B.segs.noise_host + (size_t)buf * kMaxSegments * 1352,
                              sizeof(float) * 1352 * n_segs, hipMemcpyHostToDevice, e.stream));
}

void upload_segments(Engine& e, const std::vector<diee_batch>& bt) {
    SearchBufs& B = *e.search;
    std::vector<unsigned long long> seeds(bt.size());
    std::vector<uint32_t> first(bt.size()), game0(bt.size());
    uint32_t g = 0;
    for (size_t k = 0; k < bt.size(); ++k) { seeds[k] = bt[k].seed; first[k] = bt[k].first_game_id; game0[k] = g; g += bt[k].n_games; }
    e.h2d(B.segs.seed.p, seeds.data(), seeds.size());
    e.h2d(B.segs.first_id.p, first.data(), first.size());
    e.h2d(B.segs.game0.p, game0.data(), game0.size());
    HIPCHK(hipMemsetAsync(B.slots.counters.p, 0, sizeof(unsigned long long) * kMaxSegments * CNT_COUNT, e.stream));
    e.sync();                                                          // the vectors are stack-scoped
}

void draw_noise(SearchBufs& B, int buf, const std::vector<diee_batch>& bt, uint32_t step, float alpha) {
    for (size_t k = 0; k < bt.size(); ++k)
        dirichlet_host(bt[k].seed, step, alpha, 1352, B.segs.noise_host + ((size_t)buf * kMaxSegments + k) * 1352);
}

namespace {

// The rounds of one move-step's speculative search behind its first launch: search(0), then pairs { tower(q) over the rows search(q)
// planned, search(q + 1) } for q < bound.  Launches sent ahead of a search that is complete return at once (~2 us each), so the pairs
// go out in chunks -- `chunk` of them first, then 4 at a time --, the host looking at the pinned done word in between.
struct Rounds { uint32_t sent; bool done; };
template <class Tower, class Search>
Rounds send_rounds(Engine& e, uint32_t bound, uint32_t chunk, const uint32_t* done_word, uint64_t& syncs, Tower&& tower, Search&& search) {
    search(0u);
    uint32_t q = 0;
    bool done = false;
    while (!done && q < bound) {
        const uint32_t end = std::min<uint32_t>(bound, q + std::max<uint32_t>(chunk, 1u));
        for (; q < end; ++q) { tower(q); search(q + 1); }
        HIPCHK(hipGetLastError());
        e.sync();
        ++syncs;
        done = *done_word != 0;
        chunk = 4;
    }
    return Rounds{q, done};
}

// ---- the tail of a batch (search_types.h, Tail) -------------------------------------------------------------------------------
// rows of a tail launch by live games: a launch of 32 / 64 / 128 boards costs ~95 / 125 / 172 us, and a search needs about
// 91 / (1 + s) launches when every game gets s speculative rows per launch (s saturates near 8: the rows come from nodes that exist)
uint32_t tail_rows_for(const Engine& e, uint32_t n) {
    if (n >= e.opt.spec_fused_from || n > kTailRowsMax) return (uint32_t)kTailFusedRows;          // the fused family
    return n >= e.opt.spec_rows128_from ? 128u : n >= e.opt.spec_rows64_from ? 64u : 32u;
}
bool tail_possible(Engine& e, uint32_t n, const diee_mcts_cfg& cfg) {
    if (e.opt.spec_eval == 0 || n < 1 || cfg.iterations < 1) return false;
    const uint32_t rows = tail_rows_for(e, n);
    // k_tail's workgroups (one per game, > 100 KB of LDS each: one per compute unit) meet inside the launch: all of them must be resident together.
    // A device (or a partition of one) with fewer compute units than live games searches launch by launch instead of timing out at every meeting.
    const int cus = device_cus(e);
    if (cus && n > (uint32_t)cus) return false;
    if (rows < n) return false;      // (options spec_rows64_from / spec_rows128_from can ask for fewer rows than games: every live game needs its demanded row)
    // the ring of evaluated rows grows with the iterations ((iterations + 1) launches x rows x (1352 + 72) floats; crow / cval: 256 x node_cap words):
    // beyond option spec_ring_mb the search runs one launch per iteration instead of failing an allocation in mid-batch
    const uint32_t ring_rows = rows > kTailRowsMax ? (uint32_t)kTailFusedRows : kTailRowsMax;
    const double ring_mb = ((double)(cfg.iterations + 1) * ring_rows * (1352 + 72 + 8 + 1) * 4.0 + (double)kTailMaxSlots * ((double)(cfg.iterations + 1) * std::max<uint32_t>(e.opt.nodes_per_expansion, 1) + 64) * 8.0) / 1048576.0;
    if (ring_mb > (double)e.opt.spec_ring_mb) return false;
    const bool in_reach = rows == (uint32_t)kTailFusedRows ? n <= std::min<uint32_t>(e.opt.spec_fused_games, kTailMaxSlots)
                                                           : n <= std::min<uint32_t>(e.opt.spec_max_games, kTailRowsMax);
    return in_reach && nn_tail_available(e, (int)rows, (int)n);
}

}  // namespace

void SearchBufs::Tail::reserve(uint32_t launches_now, uint32_t nodes, uint32_t rows_now) {
    if (launches_now > launches || nodes > node_cap || rows_now > rows_cap) {
        const uint32_t L = std::max(launches_now, launches), nc = std::max(nodes, node_cap), R = std::max(rows_now, rows_cap);
        crow.ensure((size_t)kTailMaxSlots * nc); cval.ensure((size_t)kTailMaxSlots * nc);
        rows_state.ensure((size_t)L * R); rows_node.ensure((size_t)L * R);
        logits.ensure((size_t)L * R * 1352); hv.ensure((size_t)L * R * 72);
        words.ensure((size_t)L + 4 + 2 * (size_t)L + 8 + (size_t)L + (size_t)L);
        launches = L; node_cap = nc; rows_cap = R;
    }
    if (!host) { HIPCHK(hipHostMalloc((void**)&host, sizeof(uint32_t) * 4)); memset(host, 0, sizeof(uint32_t) * 4); }
}
diee::Tail SearchBufs::Tail::view(Engine& e, const diee_mcts_cfg& cfg, uint32_t n) const {
    uint32_t* w = words.p;
    return diee::Tail{crow.p, cval.p, rows_state.p, rows_node.p, logits.p, hv.p, w, w + 4 * (size_t)launches + 12, w + launches, w + launches + 4,
                      w + launches + 4 + 2 * (size_t)launches + 8, host, cfg.iterations + 1, cfg.iterations, e.opt.spec_rollout_steps, tail_rows_for(e, n),
                      e.opt.spec_child_rows, e.opt.spec_extra_rows, (uint32_t)e.opt.test_tail_skip};
}

namespace {

// The iterations of one move-step's search for n <= kTailMaxSlots (option spec_max_games) live games, behind the root expansion (k_expand has selected every
// game's leaf for iteration 0): k_tail(0), then pairs of { tower launch q over the rows k_tail(q) planned, k_tail(q + 1) }.  Every pair
// completes at least one iteration, `iterations` pairs complete the search -- and far fewer do when the free rows of the launches
// carried the right nodes: the first chunk is as many pairs as the previous move-step needed (send_rounds).
void tail_run(SearchCall& call, uint32_t n, const Tree& T, const Slots& S, const Segs& G, const diee_mcts_cfg& cfg, const SearchParams& P) {
    Engine& e = call.e;
    SearchBufs::Tail& TB = call.B.tail;
    TB.reserve(cfg.iterations + 1, T.node_cap, tail_rows_for(e, n) > kTailRowsMax ? (uint32_t)kTailFusedRows : kTailRowsMax);
    const Tail L = TB.view(e, cfg, n);
    hipStream_t st = e.stream;
    // crow of the slots in use (the trees are rebuilt every move-step), the row counts, state words and meeting words
    HIPCHK(hipMemsetAsync(L.crow, 0, sizeof(uint32_t) * (size_t)n * T.node_cap, st));
    HIPCHK(hipMemsetAsync(TB.words.p, 0, sizeof(uint32_t) * (5 * (size_t)TB.launches + 12), st));
    TB.host[1] = 0; TB.host[2] = 0xFFFFFFFFu;
    uint32_t& hint = call.hint[call.side].tail;
    const Rounds r = send_rounds(e, cfg.iterations, hint ? hint + 2 : std::max<uint32_t>(8u, cfg.iterations / 6), &TB.host[1], call.host_syncs,
        [&](uint32_t q) {
            if (!nn_forward_tail(e, L.rows_state + (size_t)q * L.rows, (int)L.rows, L.n_rows + q, L.hv + (size_t)q * L.rows * 72,
                                 L.logits + (size_t)q * L.rows * 1352, (int)n, L.n_dem + q))
                throw EngineError(DIEE_ERR_HIP, "tail search: the cluster tower could not be launched");
        },
        [&](uint32_t q) { launch_tail(st, T, S, G, n, P, cfg.c, L, q); });
    uint32_t words[4] = {0, 0, 0, 0}, flag_word = 0;
    e.d2h(words, L.state, 4);
    e.d2h(&flag_word, e.flags_dev.p, 1);
    e.sync();
    // a meeting that timed out raised the starved bit (and left 2 in the state word): this search is void, cluster_starved() repeats it
    // launch by launch -- whatever the done word says (a workgroup that gave up left its game's record unsaved)
    const bool starved = (flag_word & 4u) != 0u || words[1] == 2u;
    if (L.test_skip) e.opt.test_tail_skip = 0;                       // (tests: one forced time-out per request)
    if (!r.done && !starved) throw EngineError(DIEE_ERR_HIP, "tail search: the iterations did not complete");
    if (starved) { hint = 0; return; }
    if (e.opt.trace_steps)
        fprintf(stderr, "[diee] tail: %u games, %u iterations on %u launches with rows (%u pairs sent), %u speculative rows\n", n, cfg.iterations, words[2], r.sent, words[3]);
    hint = words[2];
    call.iterations += cfg.iterations; call.launches_sent += r.sent; call.launches_with_rows += words[2]; call.spec_rows += words[3];
}

// ---- the free-running search (search_types.h, Free) -----------------------------------------------------------------------------
// rows of a launch: up to 512 live games the 4-board pair tower's 512 rows (~300 us), beyond one pass of the chip (1024 rows, ~577 us); a
// game needs 0.91 rows per iteration and the virtual descents see about one iteration ahead, so more than ~2 rows per game and launch are not used
// (at most 128 live games: the plain evaluations are of the split-K cluster family, and so are the launches: 32 / 64 / 128 dense rows like the tail's)
// the launches of a search are of the arithmetic family of the plain evaluations of its n live games (what the oracle's evaluator runs):
// the fused 16x16x32 family where tower_table sends so many boards (from 41 by default; every size under DIEE_FLAG_INVARIANT_NN), else the split-K cluster family
bool free_fused(Engine& e, uint32_t n) { return nn_free_available(e, (int)n); }
uint32_t free_rows_for(Engine& e, uint32_t n) {
    if (!free_fused(e, n)) { const uint32_t r = tail_rows_for(e, n); return r > kTailRowsMax ? kTailRowsMax : r; }
    return n >= e.opt.free_rows1024_from ? 1024u : 512u;
}
bool free_possible(Engine& e, uint32_t n, const diee_mcts_cfg& cfg) {
    if (e.opt.free_eval == 0 || cfg.iterations < 1 || cfg.iterations >= (1u << 22)) return false;
    if (n < e.opt.free_min_games || n > std::min<uint32_t>(e.opt.free_max_games, kFreeMaxSlots)) return false;
    const uint32_t rows = free_rows_for(e, n);
    if (rows < n) return false;                                   // every live game's demanded leaf must fit the launch
    if ((uint64_t)(cfg.iterations + 1) * std::max<uint32_t>(e.opt.nodes_per_expansion, 1) + 64 > (1u << 20)) return false;      // (k_free's header word holds 20 bits of node index)
    return free_fused(e, n) || (n <= kTailRowsMax && nn_tail_available(e, (int)rows, (int)n));
}
// rounds a search may take before the host gives up: about 0.91 * iterations * n / rows are needed; a game that advances one iteration per
// round needs iterations + 1; a round is lost where an evaluation aged out of the ring before its game's turn came (small rings, an
// iteration cap of 1) or where a game had to wait for another's flag words -- 4 x (iterations + games) covers what the option mixes of
// tests/tools/free_fuzz.py ever needed many times over (the words per round are 8 bytes)
uint32_t free_launches_for(const diee_mcts_cfg& cfg, uint32_t n) { return 4 * (cfg.iterations + n) + 66; }
// the ring holds the rows of the last `ring` launches: a whole search at iterations = 100, option free_ring launches beyond
uint32_t free_ring_for(const Engine& e, const diee_mcts_cfg& cfg) { return std::min<uint32_t>(cfg.iterations + 2, std::max<uint32_t>(e.opt.free_ring, 4u)); }

}  // namespace

void SearchBufs::Free::reserve(uint32_t launches_now, uint32_t ring_now, uint32_t rows_now, uint32_t slots, uint32_t nodes) {
    if (slots > slot_cap || nodes > node_cap) {
        const uint32_t sc = std::max(slots, slot_cap), nc = std::max(nodes, node_cap);
        crow.ensure((size_t)sc * nc); cval.ensure((size_t)sc * nc);
        per_slot.ensure((size_t)5 * sc); wish.ensure((size_t)sc * kFreeWish);
        slot_cap = sc; node_cap = nc;
    }
    if (ring_now > ring || rows_now > rows) {
        const uint32_t W = std::max(ring_now, ring), R = std::max(rows_now, rows);
        rows_idx.ensure((size_t)W * R); logits.ensure((size_t)W * R * 1352); hv.ensure((size_t)W * R * 72);
        rows_state.ensure((size_t)W * std::min<uint32_t>(R, kTailRowsMax));
        ring = W; rows = R;
    }
    if (launches_now > launches) { words.ensure(2 * (size_t)launches_now + 8); launches = launches_now; }
    if (!host) { HIPCHK(hipHostMalloc((void**)&host, sizeof(uint32_t) * 2)); memset(host, 0, sizeof(uint32_t) * 2); }
}
diee::Free SearchBufs::Free::view(Engine& e, const diee_mcts_cfg& cfg, uint32_t n) const {
    const uint32_t rows_now = free_rows_for(e, n), known_cus = (uint32_t)device_cus(e), cus = known_cus ? known_cus : 256u;
    uint32_t* sl = per_slot.p;
    const uint32_t sc = slot_cap;
    return diee::Free{crow.p, cval.p, rows_idx.p, free_fused(e, n) ? nullptr : rows_state.p, logits.p, hv.p, words.p, words.p + launches, sl, sl + sc, wish.p, sl + 2 * (size_t)sc, sl + 3 * (size_t)sc,
                      sl + 4 * (size_t)sc, words.p + 2 * (size_t)launches, host, free_launches_for(cfg, n), cfg.iterations, rows_now, free_ring_for(e, cfg),
                      std::min<uint32_t>(free_lds_nodes_for(n, cus), std::max<uint32_t>(e.opt.free_lds_nodes, 64u)), e.opt.free_rollout_steps,
                      // candidates per game and round: about twice the spare rows a game can hope for (what is not granted is found again next round), at most the option's
                      std::min<uint32_t>(e.opt.free_cand_max, 1u + (e.opt.free_cand_x4 * (rows_now - std::min(rows_now, n)) + 4u * n - 1u) / (4u * n)),
                      e.opt.free_lag_boost, e.opt.free_lag_step,
                      // iterations per game and launch: with few games and many spare rows a game often runs 6 ... 8 iterations on one launch's rows (profiles/r06h_*)
                      std::max<uint32_t>(n <= kTailRowsMax ? 2u * e.opt.free_iter_cap : e.opt.free_iter_cap, 1u)};
}

namespace {

// The iterations of one move-step's search for free_min_games ... free_max_games (17 ... 800) live games, behind the root expansion (k_expand has selected every game's leaf
// for iteration 0): round 0 = { k_free, k_free_pack }, then rounds { tower launch q over the rows granted, k_free, k_free_pack }.  The game
// furthest behind completes an iteration in nearly every round (not where its evaluation aged out of the ring or a flag word of another game is
// still missing), so about `iterations` + 1 rounds suffice at worst -- and about 0.91 * n / rows of that do; the bound is F.launches (free_launches_for).
void free_run(SearchCall& call, uint32_t n, const Tree& T, const Slots& S, const Segs& G, const diee_mcts_cfg& cfg, const SearchParams& P) {
    Engine& e = call.e;
    SearchBufs::Free& FB = call.B.free;
    FB.reserve(free_launches_for(cfg, n), free_ring_for(e, cfg), free_rows_for(e, n), n, T.node_cap);
    const Free F = FB.view(e, cfg, n);
    hipStream_t st = e.stream;
    // crow of the slots in use (the trees are rebuilt every move-step), the row counts and state words, the per-slot progress (first_sel is
    // written by round 0)
    HIPCHK(hipMemsetAsync(F.crow, 0, sizeof(uint32_t) * (size_t)n * T.node_cap, st));
    HIPCHK(hipMemsetAsync(FB.words.p, 0, sizeof(uint32_t) * (2 * (size_t)FB.launches + 8), st));
    HIPCHK(hipMemsetAsync(FB.per_slot.p, 0, sizeof(uint32_t) * (size_t)5 * FB.slot_cap, st));
    FB.host[0] = 0; FB.host[1] = 0xFFFFFFFFu;
    uint32_t& hint = call.hint[call.side].free;
    const Rounds r = send_rounds(e, F.launches - 1, hint ? hint + 2 : std::max<uint32_t>(8u, (uint32_t)((double)cfg.iterations * n / F.rows) + 4u), &FB.host[0],
        call.host_syncs,
        [&](uint32_t q) {
            const size_t rb = (size_t)(q % F.ring) * F.rows;
            if (F.rows_state) {
                if (!nn_forward_tail(e, F.rows_state + rb, (int)F.rows, F.n_rows + q, F.hv + rb * 72, F.logits + rb * 1352, (int)n, F.n_dem + q))
                    throw EngineError(DIEE_ERR_HIP, "free-running search: the cluster tower could not be launched");
            } else
                nn_forward_free(e, T.state, F.rows_idx + rb, F.n_rows + q, (int)F.rows, F.hv + rb * 72, F.logits + rb * 1352, (int)n, F.n_dem + q);
        },
        [&](uint32_t q) { launch_free(st, T, S, G, n, P, cfg.c, F, q); });
    uint32_t words[4] = {0, 0, 0, 0};
    e.d2h(words, F.state, 4);
    e.sync();
    if (!r.done) throw EngineError(DIEE_ERR_HIP, "free-running search: the iterations did not complete");
    if (e.opt.trace_steps)
        fprintf(stderr, "[diee] free-running: %u games, %u iterations on %u launches with rows of <= %u (%u rounds sent), %u speculative rows, %u nodes in LDS\n",
                n, cfg.iterations, words[1], F.rows, r.sent, words[2], F.lds_nodes);
    if (e.opt.trace_steps >= 2) {                                      // development: the rows of every round (where the stragglers' rounds begin)
        std::vector<uint32_t> nr((size_t)r.sent + 1), nd((size_t)r.sent + 1);
        e.d2h(nr.data(), F.n_rows, nr.size()); e.d2h(nd.data(), F.n_dem, nd.size()); e.sync();
        fprintf(stderr, "[diee] free-running rounds (rows/demanded):");
        for (size_t i = 0; i < nr.size(); ++i) fprintf(stderr, " %u/%u", nr[i], nd[i]);
        fprintf(stderr, "\n");
    }
    hint = words[1];
    call.iterations += cfg.iterations; call.launches_sent += r.sent; call.launches_with_rows += words[1]; call.spec_rows += words[2];
}

}  // namespace

// Above the speculative searches' reach it enqueues only; a tail or free-running search looks at its done word between chunks of
// launches, i.e. synchronises a few times per move-step.
void mcts_run(SearchCall& call, uint32_t n, uint32_t n_segs, const diee_mcts_cfg& cfg, int buf, uint32_t flags) {
    Engine& e = call.e;
    SearchBufs& B = call.B;
    const Tree T = B.tree.view();
    Slots S = B.slots.view(e);
    const Segs G = B.segs.view(n_segs, B.slots.iter_cap);
    hipStream_t st = e.stream;
    const uint32_t quirks = (flags & DIEE_FLAG_REF_QUIRKS) ? 1u : 0u;
    // slots whose selected leaf was terminal need no network row: above 256 live games only the others are evaluated
    const NnRows rows{B.slots.leaf_term.p, B.slots.row_slot.p, B.slots.slot_row.p, B.slots.n_rows.p};
    HIPCHK(hipMemsetAsync(B.slots.iter_flags.p, 0, sizeof(uint32_t) * 2 * (size_t)B.slots.iter_cap * n_segs, st));
    call.stage_noise(S, n_segs, buf);
    launch_init_roots(st, T, S, n);
    // option cl_grow (default on): below 129 boards the evaluation is ONE cluster-tower launch, latency-bound, with CUs to spare while
    // fewer than ~28 games live (the tail of a batch: 130 of its 364 move-steps): the launch takes the growth along on extra
    // workgroups (GrowReq) -- no second stream, no event --, and the k_expand behind it only has the priors, the backpropagation and
    // the next descent left (16.2 -> 9.4 us on the chain between two evaluations).
    const bool cl_grow = e.opt.cl_grow != 0;
    const ExpandVariant xv{e.opt.expand2 != 0, e.opt.expand2c != 0};      // handed down to every launch
    GrowReq greq{T, S, G, n, 0u};
    struct GrowScope { NetWeights* w; ~GrowScope() { w->grow_req = nullptr; w->grow_done = false; } } gscope{e.net};
    bool grown = false;                                              // the tower launch of this evaluation took the growth along
    auto forward = [&](uint32_t it, const NnRows* rws) {
        greq.S = S; greq.it = it;
        e.net->grow_req = cl_grow ? &greq : nullptr;
        e.net->grow_done = false;
        const bool compacted = nn_forward(e, B.slots.eval_states.p, (int)n, nullptr, nullptr, rws);
        e.net->grow_req = nullptr;
        grown = e.net->grow_done;
        return compacted;
    };
    forward(kRootIteration, nullptr);                                // forward_policy, alpha_mcts.rs:104 (softmax / tanh in k_expand)
    const SearchParams P{cfg.dir_eps, quirks};
    // one MCTS kernel per network evaluation: expand + backpropagate iteration it, then select for it+1
    launch_expand(st, T, S, G, n, kRootIteration, P, cfg.iterations ? 0u : kNoNextIteration, cfg.c, grown, xv);
    if (free_possible(e, n, cfg)) {                                  // 17 ... 800 live games: every game on its own iteration counter
        S.slot_row = nullptr;
        free_run(call, n, T, S, G, cfg, P);
    } else if (tail_possible(e, n, cfg)) {                           // <= 16 live games: the games in lockstep inside one launch
        S.slot_row = nullptr;
        tail_run(call, n, T, S, G, cfg, P);
    } else {
        for (uint32_t it = 0; it < cfg.iterations; ++it) {           // alpha_mcts.rs:149
            const bool compacted = forward(it, &rows);               // alpha_mcts.rs:186
            S.slot_row = compacted ? B.slots.slot_row.p : nullptr;
            launch_expand(st, T, S, G, n, it, P, it + 1 < cfg.iterations ? it + 1 : kNoNextIteration, cfg.c, grown, xv);
        }
    }
    launch_reduce_counters(st, S, G, B.slots.step_log.p, std::min(call.cur_step, kStepLog - 1));
    HIPCHK(hipGetLastError());
}

// a starved in-launch hand-over of the cluster tower (another process on the GPU took its CUs) raises bit 2 of the
// flag word: the tower then finished "dead" and this search is garbage.  Detected before the move is played: the
// cluster table is dropped for the rest of the process and the caller repeats the search on the per-layer kernels.
bool cluster_starved(Engine& e) {
    if (!e.net || !nn_cluster_used(e)) return false;
    uint32_t* flag_word = e.search->segs.live_host + kLiveWords;
    e.d2h(flag_word, e.flags_dev.p, 1);
    e.sync();
    // tests: option test_starve_at = k treats the k-th check of this ctx as a starved hand-over (the fallback path has
    // no other way to be exercised on a box with one process per GPU)
    const bool forced = e.opt.test_starve_at > 0 && ++e.starve_checks == e.opt.test_starve_at;
    if (!(*flag_word & 4u) && !forced) return false;
    nn_disable_cluster(e);                                            // clears the flag bit and re-arms the counters
    fprintf(stderr, "[diee] cluster tower: a workgroup hand-over starved (is another process using this GPU?); "
                    "falling back to the per-layer kernels for the rest of this process\n");
    return true;
}

void read_counters(Engine& e, uint32_t seg, diee_stats* stats) {
    if (!stats) return;
    unsigned long long c[CNT_COUNT];
    e.d2h(c, e.search->slots.counters.p + (size_t)seg * CNT_COUNT, (size_t)CNT_COUNT);
    e.sync();
    stats->nn_evals = c[CNT_NN_EVALS]; stats->expansions = c[CNT_EXPANSIONS]; stats->children = c[CNT_CHILDREN];
    stats->terminal_hits = c[CNT_TERMINAL]; stats->depth_sum = c[CNT_DEPTH_SUM]; stats->selections = c[CNT_SELECTIONS];
    stats->illegal_decodes = c[CNT_ILLEGAL]; stats->max_children = c[CNT_MAX_CHILDREN];
    stats->plies = c[CNT_PLIES]; stats->games = c[CNT_GAMES]; stats->nn_rows = c[CNT_NN_ROWS];
}

void Engine::mcts_batch(const diee_bg_state* roots, uint32_t n, const diee_mcts_cfg* cfg, uint64_t seed, uint32_t step,
                        const uint32_t* game_ids, const uint32_t* rounds, uint32_t flags, float* visit_probs,
                        uint32_t* n_children, float* root_visits, diee_stats* stats) {
    HIPCHK(hipSetDevice(device));
    if (!net || !net->loaded) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called");
    if (stats) memset(stats, 0, sizeof *stats);
    if (!n) return;
    for (uint32_t i = 0; i < n; ++i)
        if (roots[i].roll[0] == 0 && roots[i].roll[1] == 0) throw EngineError(DIEE_ERR_ARG, "die has not been rolled (backgammon_logic.rs:404)");
    reserve_search(*this, n, cfg->iterations);
    nn_reserve(*this, (int)n);
    SearchBufs& B = *search;
    SearchCall call(*this);
    const InvariantScope inv(*this, flags);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> ids(n), rds(n);
    for (uint32_t i = 0; i < n; ++i) { ids[i] = game_ids ? game_ids[i] : i; rds[i] = rounds ? rounds[i] : 0; }
    // the roots are ONE batch (one alpha_mcts_parallel call): a single segment spanning every slot
    const std::vector<diee_batch> one{{n, 0u, seed}};
    upload_segments(*this, one);
    const uint32_t span[2] = {0u, n};
    h2d(B.segs.span.p, &span[0], 1); h2d(B.segs.span.p + kMaxSegments, &span[1], 1);
    HIPCHK(hipMemsetAsync(B.slots.seg.p, 0, sizeof(uint32_t) * n, stream));
    h2d((uint8_t*)B.slots.roots.p, (const uint8_t*)roots, (size_t)n * 32);
    h2d(B.slots.game_id.p, ids.data(), (size_t)n); h2d(B.slots.round.p, rds.data(), (size_t)n);
    sync();
    const int se = net->sample_every; net->sample_every = 0;
    draw_noise(B, 0, one, step, cfg->dir_alpha);
    net->cur_step = 0;
    search_or_repeat(call, n, 1, *cfg, 0, flags, [&] {               // (a repeat starts from zeroed counters)
        HIPCHK(hipMemsetAsync(B.slots.counters.p, 0, sizeof(unsigned long long) * CNT_COUNT, stream));
    });
    net->sample_every = se;
    tmp_a.ensure((size_t)n * 1352 * 4); tmp_b.ensure((size_t)n * 4); tmp_c.ensure((size_t)n * 4);
    launch_root_probs(stream, B.tree.view(), n, (float*)tmp_a.p, (uint32_t*)tmp_b.p, (float*)tmp_c.p);
    HIPCHK(hipGetLastError());
    d2h((uint8_t*)visit_probs, tmp_a.p, (size_t)n * 1352 * 4);
    if (n_children) d2h((uint8_t*)n_children, tmp_b.p, (size_t)n * 4);
    if (root_visits) d2h((uint8_t*)root_visits, tmp_c.p, (size_t)n * 4);
    sync();
    if (stats) {
        read_counters(*this, 0, stats);
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        call.report(*stats);
    }
    check_overflow();
}

}  // namespace diee
