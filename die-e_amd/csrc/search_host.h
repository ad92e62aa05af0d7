// search_host.h -- what the host drivers of the search share: the buffers of a ctx (SearchBufs: allocations only), the state of the call
// in progress (SearchCall: on the entry point's stack), one move-step's search (mcts_run) and the entry points' common steps.
// search_host.cpp: buffers, the round drivers, the dispatch, Engine::mcts_batch; selfplay_host.cpp: Engine::self_play*;
// arena_host.cpp: Engine::arena; dirichlet_host.cpp; pinned_pool.cpp.
#pragma once
#include <vector>

#include "engine.h"
#include "launch.h"
#include "nn_host.h"
#include "pinned_pool.h"

namespace diee {

constexpr uint32_t kStepLog = 2048;                          // move-steps of a call with a log entry of their own (later ones share the last)
constexpr uint32_t kLiveWords = 1 + 4 * kMaxSegments;        // DeliverSummary at its largest; live_host[kLiveWords] = the flag word

// One group per parameter block of search_types.h: its device allocations, capacities (grown to max(old, new), never shrunk) and view.
// What lives as long as the ctx stays here too: the copy stream and its events, the pinned words, `cus`.
struct SearchBufs {
    struct Tree {
        DevBuf<float> visits, value, prior;
        DevBuf<uint32_t> parent, first_child, meta, used;
        DevBuf<BgState> nstate;
        uint32_t node_cap = 0;
        void reserve(uint32_t slot_cap, uint32_t nodes);
        diee::Tree view() const { return diee::Tree{visits.p, value.p, prior.p, parent.p, first_child.p, meta.p, nstate.p, used.p, node_cap}; }
    } tree;
    struct Slots {
        DevBuf<BgState> roots, eval_states;
        DevBuf<uint32_t> game_id, round, seg, leaf, sel, iter_flags, row_slot, slot_row, n_rows;
        DevBuf<float> sel_value, noise, root_value0;
        DevBuf<uint8_t> leaf_term, path_len;
        DevBuf<uint32_t> path, leaf_meta, grow_k;
        DevBuf<uint16_t> grow_code;
        DevBuf<unsigned long long> counters, counters_bak;
        DevBuf<uint32_t> slot_cnt;
        DevBuf<unsigned long long> step_log;                   // [2 * kStepLog] per move-step { expansions, rows evaluated } (k_reduce_counters)
        uint32_t cap = 0, iter_cap = 0;
        void reserve(uint32_t slots, uint32_t iterations);
        diee::Slots view(Engine& e) const;
    } slots;
    struct Segs {                                              // batches ("segments") in flight
        DevBuf<unsigned long long> seed;
        DevBuf<uint32_t> first_id, game0, span;                // span = first_slot[kMaxSegments] ++ end_slot[kMaxSegments]
        DevBuf<uint32_t> live_dev;                             // [kLiveWords] DeliverSummary of the move-step
        float* noise_host = nullptr;                           // pinned, [2][kMaxSegments][1352]: upload without a sync
        uint32_t* live_host = nullptr;                         // pinned, [kLiveWords + 1]: n_live, per-batch live, ..., flag word
        void reserve();
        diee::Segs view(uint32_t n_segs, uint32_t iter_cap) const { return diee::Segs{seed.p, first_id.p, game0.p, span.p, span.p + kMaxSegments, n_segs, iter_cap}; }
        ~Segs() { if (noise_host) (void)hipHostFree(noise_host); if (live_host) (void)hipHostFree(live_host); }
    } segs;
    struct Tail {                                              // the tail of a batch (search_types.h, Tail)
        DevBuf<uint32_t> crow, rows_node, words;               // words = n_rows[launches] ++ state[4] ++ bar[2 * launches + 8] ++ bar2[launches] ++ n_dem[launches]
        DevBuf<float> cval, logits, hv;
        DevBuf<BgState> rows_state;
        uint32_t* host = nullptr;                              // pinned, [4]
        uint32_t launches = 0, node_cap = 0, rows_cap = 0;
        void reserve(uint32_t launches_now, uint32_t nodes, uint32_t rows_now);
        diee::Tail view(Engine& e, const diee_mcts_cfg& cfg, uint32_t n) const;
        ~Tail() { if (host) (void)hipHostFree(host); }
    } tail;
    struct Free {                                              // the free-running search (search_types.h, Free)
        DevBuf<uint32_t> crow, rows_idx, words, per_slot, wish;      // words = n_rows[launches] ++ n_dem[launches] ++ state[8]; per_slot = grant_off ++ grant_cnt ++ wish_n ++ prog ++ first_sel, [slots] each
        DevBuf<float> cval, logits, hv;
        DevBuf<BgState> rows_state;                            // dense states of the launches of at most 128 rows (cluster family)
        uint32_t* host = nullptr;                              // pinned, [2]
        uint32_t launches = 0, ring = 0, rows = 0, slot_cap = 0, node_cap = 0;
        void reserve(uint32_t launches_now, uint32_t ring_now, uint32_t rows_now, uint32_t slots, uint32_t nodes);
        diee::Free view(Engine& e, const diee_mcts_cfg& cfg, uint32_t n) const;
        ~Free() { if (host) (void)hipHostFree(host); }
    } free;
    struct Games {                                             // the games of a self-play call and their record areas
        DevBuf<BgState> state;
        DevBuf<uint32_t> rounds, nfrags, ev_a_count, ev_a_step, ev_b_count, ev_b_step, live;
        DevBuf<uint8_t> alive, seg;
        DevBuf<int8_t> winner, frag_player;
        DevBuf<float> frag_ps, frag_planes;
        uint32_t game_cap = 0, area_cap = 0, frag_cap = 0;     // games (the small per-game words), record areas and fragments per area
        void reserve(uint32_t n_games, uint32_t areas, uint32_t frags);
        diee::Games view(unsigned long long* counters, uint32_t* area) const {
            return diee::Games{state.p, rounds.p, nfrags.p, alive.p, winner.p, ev_a_count.p, ev_a_step.p, ev_b_count.p, ev_b_step.p, live.p, seg.p,
                               frag_ps.p, frag_planes.p, frag_player.p, frag_cap, counters, area};
        }
    } games;
    // slot refill (self_play_refill): the record area of every game, the stack of free areas { count, stack[width] }, and the Dirichlet
    // samples of the call so far, [move-step][batch][1352] (Slots::noise_segs)
    struct Refill {
        DevBuf<uint32_t> area, free_areas;
        DevBuf<float> noise_tab;
        void reserve(uint32_t n_games, uint32_t width, size_t noise_floats) { area.ensure(n_games); free_areas.ensure((size_t)width + 1); noise_tab.ensure(noise_floats); }
    } refill;
    struct Arena {                                             // the arena (search_types.h, Arena)
        DevBuf<BgState> state, initial;
        DevBuf<uint8_t> alive;
        DevBuf<int8_t> winner, side;
        DevBuf<uint32_t> round, live, list, words;
        void reserve(uint32_t n_games);
        diee::Arena view(uint32_t n_games) const { return diee::Arena{state.p, initial.p, alive.p, winner.p, round.p, side.p, live.p, list.p, words.p, n_games}; }
    } arena;
    // output delivery: a step's flushes (double-buffered: the copy stream reads step s's list while step s + 1's is written),
    // one staging buffer (the copy stream runs gather -> copies out -> next gather in order), the stream and its guards
    struct Deliver {
        DevBuf<DeliverEvent> events[2];
        DevBuf<float> ps, planes;
        DevBuf<int8_t> outcome;
        DevBuf<uint32_t> game;
        uint32_t rows = 0;                                     // staging rows
        hipStream_t copy = nullptr;
        hipEvent_t ev_copy[2] = {nullptr, nullptr};            // the copy stream is done with events[i]
        void reserve_events(uint32_t slots) { for (auto& ev : events) ev.ensure((size_t)2 * slots); }
        void reserve_stage(uint32_t stage_rows);               // ... and the stream, on first use
        DeliverOut view() const { return DeliverOut{ps.p, planes.p, outcome.p, game.p}; }
        ~Deliver() {
            if (copy) (void)hipStreamDestroy(copy);
            for (hipEvent_t e : ev_copy) if (e) (void)hipEventDestroy(e);
        }
    } deliver;
    int cus = 0;                                               // compute units of the device (device_cus)
};

void free_search(SearchBufs* s);
void reserve_search(Engine& e, uint32_t slots, uint32_t iterations);      // tree, slots and segments (creates e.search)
int device_cus(Engine& e);                                     // compute units of e.device, asked once per ctx; 0: the query failed (asked again next time)

// The state of ONE call of an entry point (mcts_batch, self_play*, arena): constructed on its stack behind reserve_search, handed to every
// search of the call, gone with it.  The constructor is the call's prologue (it zeroes the step log on the engine's stream).
struct SearchCall {
    Engine& e;
    SearchBufs& B;
    uint32_t cur_step = 0;                                     // the move-step (arena: round) whose search is being enqueued
    const uint32_t noise_rows;                                 // slot refill: move-steps Refill::noise_tab holds in this call; 0: not a refill call
    struct Hint { uint32_t tail = 0, free = 0; } hint[2];      // tower launches the previous search needed (sizes the first chunk of the next); the arena keeps
    uint32_t side = 0;                                         // one pair per player and sets `side`, every other call uses hint[0]
    // the speculative searches (k_tail and the free-running one) of the call so far
    uint64_t iterations = 0, launches_sent = 0, launches_with_rows = 0, spec_rows = 0, host_syncs = 0;
    bool ev_copy_armed[2] = {false, false};                    // Deliver::ev_copy[i] has been recorded and not waited for
    explicit SearchCall(Engine& eng, uint32_t refill_noise_rows = 0);
    // this move-step's Dirichlet samples (pinned buffer `buf`) -> the device; slot refill: they join the table of the call's, and a root reads the row of its own round
    void stage_noise(diee::Slots& S, uint32_t n_segs, int buf) const;
    void report(diee_stats& st) const { st.tail_iterations = iterations; st.tail_launches = launches_with_rows; st.tail_spec_rows = spec_rows; }
};

struct InvariantScope {    // DIEE_FLAG_INVARIANT_NN for the duration of one call
    NetWeights* w; bool saved;
    InvariantScope(Engine& e, uint32_t flags) : w(e.net), saved(e.net->invariant) { if (flags & DIEE_FLAG_INVARIANT_NN) w->invariant = true; }
    ~InvariantScope() { w->invariant = saved; }
};

// the batches ("segments") of a call: seeds, RNG keys of their first games, positions of their first games; zeroes the counters
void upload_segments(Engine& e, const std::vector<diee_batch>& bt);
// one Dirichlet sample per batch and move-step (noise.rs:27-34), drawn on the host into pinned buffer `buf`
void draw_noise(SearchBufs& B, int buf, const std::vector<diee_batch>& bt, uint32_t step, float alpha);
void dirichlet_host(uint64_t seed, uint32_t step, float alpha, int n, float* out);      // dirichlet_host.cpp (also drawn by ttt_host.cpp)
// alpha_mcts_parallel on the n slots already loaded into Slots::roots / game_id / round / seg (segment table uploaded, the Dirichlet
// samples of this move-step in pinned buffer `buf`)
void mcts_run(SearchCall& call, uint32_t n, uint32_t n_segs, const diee_mcts_cfg& cfg, int buf, uint32_t flags);
bool cluster_starved(Engine& e);                               // the search just enqueued is void: repeat it (the cluster table has been dropped)
void read_counters(Engine& e, uint32_t seg, diee_stats* stats);

// One search and, where a hand-over starved during it, the same search again on the per-layer kernels: restore_counters() puts the
// counter rows back to what they held before the first attempt.  while_searching() is host work that overlaps the first attempt.
template <class Restore, class Overlap>
void search_or_repeat(SearchCall& call, uint32_t n, uint32_t n_segs, const diee_mcts_cfg& cfg, int buf, uint32_t flags, Restore&& restore_counters,
                      Overlap&& while_searching) {
    mcts_run(call, n, n_segs, cfg, buf, flags);
    while_searching();
    if (cluster_starved(call.e)) {
        restore_counters();
        mcts_run(call, n, n_segs, cfg, buf, flags);
    }
}
template <class Restore>
void search_or_repeat(SearchCall& call, uint32_t n, uint32_t n_segs, const diee_mcts_cfg& cfg, int buf, uint32_t flags, Restore&& restore_counters) {
    search_or_repeat(call, n, n_segs, cfg, buf, flags, restore_counters, [] {});
}

}  // namespace diee
