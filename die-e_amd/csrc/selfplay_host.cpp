// selfplay_host.cpp -- host driver of self-play: the move-step loop around the search and the delivery of the records.
// Reference call structure: self_play_parallel (src/alphazero/alpha_parallel.rs:101-231).  Per move-step there is ONE
// device->host read (the live-game count and the step's delivery summary).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "search_host.h"

namespace diee {

void SearchBufs::Games::reserve(uint32_t n_games, uint32_t areas, uint32_t frags) {
    if (n_games > game_cap) {
        const uint32_t gc = n_games;
        state.ensure(gc); rounds.ensure(gc); nfrags.ensure(gc); alive.ensure(gc); winner.ensure(gc);
        ev_a_count.ensure(gc); ev_a_step.ensure(gc); ev_b_count.ensure(gc); ev_b_step.ensure(gc);
        live.ensure(gc); seg.ensure(gc);
        game_cap = gc;
    }
    if (areas > area_cap || frags > frag_cap) {
        const uint32_t ac = std::max(areas, area_cap), fc = std::max(frags, frag_cap);
        frag_ps.ensure((size_t)ac * fc * 1352); frag_planes.ensure((size_t)ac * fc * 144);
        frag_player.ensure((size_t)ac * fc);
        area_cap = ac; frag_cap = fc;
    }
}
void SearchBufs::Deliver::reserve_stage(uint32_t stage_rows) {
    if (!copy) {
        HIPCHK(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        for (auto& e : ev_copy) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (stage_rows > rows) {
        ps.ensure((size_t)stage_rows * 1352); planes.ensure((size_t)stage_rows * 144);
        outcome.ensure(stage_rows); game.ensure(stage_rows); rows = stage_rows;
    }
}

void Engine::self_play(uint32_t n_games, uint32_t first_game_id, const diee_mcts_cfg* cfg, float temperature,
                       uint64_t seed, uint32_t flags, uint32_t max_steps, diee_fragments* out, diee_stats* stats) {
    const diee_batch one{n_games, first_game_id, seed};
    self_play_multi(&one, 1, cfg, temperature, flags, max_steps, out, stats);
}

// K calls of self_play_parallel (alpha_parallel.rs:101-231) played side by side: every batch starts at move-step 0,
// the slot space holds the live games of batch 0, then of batch 1, ..., and every network launch evaluates them all.
// Each batch keeps its own seed, Dirichlet stream, `node_selected` flags and slot-0 bookkeeping, so what a batch
// produces depends on the other batches only through the network kernel its rows are evaluated by.
void Engine::self_play_multi(const diee_batch* batches, uint32_t n_batches, const diee_mcts_cfg* cfg, float temperature,
                             uint32_t flags, uint32_t max_steps, diee_fragments* outs, diee_stats* stats) {
    self_play_run(batches, n_batches, 0u, cfg, temperature, flags, max_steps, outs, stats);
}

// Slot refill (opt-in; the reference's loop, alpha_parallel.rs:129, plays the games a call started with and nothing else): at most `width`
// games of the call are in flight, and the slot of a game retired in move-step s is taken in s + 1 by the next unstarted game (batch-major,
// ascending game id).  Without the quirks nothing couples the games of a batch but the Dirichlet sample of a move-step, and in a reference
// call every live game's round IS the move-step: a game admitted late reads the sample of its own round (Slots::noise_segs), its dice and
// sampling keys are (batch seed, game id, round) anyway, so its records are those of a plain call of its batch.  What the call holds in HBM
// goes by `width`: slots, trees, network rows and the record areas of the games in flight (Games::area).
void Engine::self_play_refill(const diee_batch* batches, uint32_t n_batches, uint32_t width, const diee_mcts_cfg* cfg, float temperature,
                              uint32_t flags, uint32_t max_steps, diee_fragments* outs, diee_stats* stats) {
    if (flags & DIEE_FLAG_REF_QUIRKS) throw EngineError(DIEE_ERR_ARG, "slot refill needs DIEE_FLAG_REF_QUIRKS off (Q14 couples the slots of a reference call)");
    if (width == 0) throw EngineError(DIEE_ERR_ARG, "width must be >= 1");
    self_play_run(batches, n_batches, width, cfg, temperature, flags, max_steps, outs, stats);
}

namespace {

// ---- output delivery (alpha_parallel.rs:215-230: the call returns all_memories) --------------------------------
// A game's records are final in the move-step that removes it, and the reference's order is (move-step, game, round-limit
// flush before win flush): the output of a batch grows by whole steps.  So each step's flushes are listed on the device
// (k_deliver_scan, 3 words per batch read back with the live counts), gathered + relabelled into a staging buffer and
// copied into pinned host arrays on a second stream while the next move-steps search; the long tail of a batch (147 of
// 364 move-steps with <= 32 live games) leaves nothing to wait for at the end.  outs == NULL: listed and counted only.
struct Delivery {
    SearchCall& call;
    const Games& Gm; const Segs& G;
    const uint32_t n_batches, stage_rows;
    const bool deliver;
    std::vector<FragBufs> fb;
    std::vector<uint64_t> frag_total;
    std::vector<uint32_t> pending;                                      // DeliverSummary of the step whose records still have to go out
    int pending_buf = 0;
    double secs = 0.0;
    uint64_t bytes = 0;
    Delivery(SearchCall& c, const Games& gm, const Segs& g, const std::vector<diee_batch>& bt, uint32_t n_slots, uint32_t frag_cap, bool on)
        : call(c), Gm(gm), G(g), n_batches((uint32_t)bt.size()), stage_rows(std::max<uint32_t>(c.e.opt.deliver_stage_rows, 1)), deliver(on),
          fb(on ? bt.size() : 0), frag_total(bt.size(), 0) {
        SearchBufs::Deliver& D = call.B.deliver;
        D.reserve_events(n_slots);
        if (!deliver) return;
        D.reserve_stage(stage_rows);
        // first guess: 128 records per game (a random-init game runs ~107 plies); grown when a batch outruns it
        for (size_t k = 0; k < bt.size(); ++k)
            fb[k].reserve(std::min<size_t>((size_t)bt[k].n_games * frag_cap, (size_t)bt[k].n_games * call.e.opt.deliver_rows_per_game + 1024));
    }
    ~Delivery() { if (deliver) (void)hipStreamSynchronize(call.B.deliver.copy); }      // (no copy may outlive its pinned target)
    void send_pending() {
        if (pending.empty()) return;
        SearchBufs::Deliver& D = call.B.deliver;
        const DeliverOut stage = D.view();
        const auto td = std::chrono::steady_clock::now();
        bool sent = false;
        for (uint32_t k = 0; k < n_batches; ++k) {
            const uint32_t rows = pending[DeliverSummary::rows(n_batches, k)], e0 = pending[DeliverSummary::ev0(n_batches, k)],
                           ne = pending[DeliverSummary::nev(n_batches, k)];
            frag_total[k] += rows;
            if (!deliver || !rows) continue;
            FragBufs& f = fb[k];
            if (f.n + rows > f.cap) { HIPCHK(hipStreamSynchronize(D.copy)); f.reserve(f.n + rows); }
            for (uint32_t o = 0; o < rows; o += stage_rows) {
                const uint32_t m = std::min(stage_rows, rows - o);
                launch_deliver_copy(D.copy, Gm, G, D.events[pending_buf].p + e0, ne, o, o + m, stage);
                HIPCHK(hipGetLastError());
                const size_t at = f.n + o;
                HIPCHK(hipMemcpyAsync(f.ps + at * 1352, stage.ps, (size_t)m * 1352 * sizeof(float), hipMemcpyDeviceToHost, D.copy));
                HIPCHK(hipMemcpyAsync(f.state + at * 144, stage.planes, (size_t)m * 144 * sizeof(float), hipMemcpyDeviceToHost, D.copy));
                HIPCHK(hipMemcpyAsync(f.outcome + at, stage.outcome, (size_t)m, hipMemcpyDeviceToHost, D.copy));
                HIPCHK(hipMemcpyAsync(f.game + at, stage.game, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, D.copy));
                bytes += (size_t)m * (1352 * 4 + 144 * 4 + 1 + 4);
            }
            f.n += rows;
            sent = true;
        }
        if (sent) { HIPCHK(hipEventRecord(D.ev_copy[pending_buf], D.copy)); call.ev_copy_armed[pending_buf] = true; }
        pending.clear();
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - td).count();
    }
    // the engine's stream waits until the copy stream is done with events[buf] (if it was handed any)
    void wait_copied(int buf) {
        if (!call.ev_copy_armed[buf]) return;
        HIPCHK(hipStreamWaitEvent(call.e.stream, call.B.deliver.ev_copy[buf], 0));
        call.ev_copy_armed[buf] = false;
    }
    void finish() {                                                     // the last copies (one game's records, typically)
        send_pending();
        if (!deliver) return;
        const auto td = std::chrono::steady_clock::now();
        HIPCHK(hipStreamSynchronize(call.B.deliver.copy));
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - td).count();
    }
};

}  // namespace

// width == 0: every game of the call starts at move-step 0 (self_play_multi); else slot refill
void Engine::self_play_run(const diee_batch* batches, uint32_t n_batches, uint32_t width, const diee_mcts_cfg* cfg, float temperature,
                           uint32_t flags, uint32_t max_steps, diee_fragments* outs, diee_stats* stats) {
    HIPCHK(hipSetDevice(device));
    if (!net || !net->loaded) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called");
    if (outs) memset(outs, 0, sizeof(diee_fragments) * n_batches);
    if (stats) memset(stats, 0, sizeof(diee_stats) * n_batches);
    if (cfg->iterations == 0) throw EngineError(DIEE_ERR_ARG, "iterations must be >= 1");
    if (n_batches == 0 || n_batches > kMaxSegments) throw EngineError(DIEE_ERR_ARG, "1 .. 64 batches per call");
    const std::vector<diee_batch> bt(batches, batches + n_batches);
    std::vector<uint32_t> game0(n_batches);
    uint64_t total_games = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
        if (bt[k].n_games == 0) throw EngineError(DIEE_ERR_ARG, "a batch needs at least one game");
        game0[k] = (uint32_t)total_games; total_games += bt[k].n_games;
    }
    if (total_games > (1u << 22)) throw EngineError(DIEE_ERR_ARG, "too many games in flight");
    const uint32_t n_games = (uint32_t)total_games;
    const bool refill = width != 0;
    const uint32_t n_slots = refill ? std::min(width, n_games) : n_games;      // games in flight at most: slots, trees, network rows, record areas
    // slot refill: the Dirichlet samples of move-steps 0 ... round_limit (no game is searched in a later round), fewer under max_steps
    const uint64_t noise_rows = refill ? std::min<uint64_t>(cfg->round_limit, max_steps ? max_steps - 1 : 0xFFFFFFFFu) + 1 : 0;
    if (noise_rows * n_batches * 1352 * sizeof(float) > ((uint64_t)8 << 30))
        throw EngineError(DIEE_ERR_ARG, "slot refill keeps one Dirichlet sample per batch and round: round_limit x batches is too large");
    reserve_search(*this, n_slots, cfg->iterations);
    nn_reserve(*this, (int)n_slots);
    SearchBufs& B = *search;
    const InvariantScope inv(*this, flags);
    const uint32_t frag_cap = cfg->round_limit + 2;
    B.games.reserve(n_games, n_slots, frag_cap);
    if (refill) {
        B.refill.reserve(n_games, n_slots, (size_t)noise_rows * n_batches * 1352);
        refill_areas = n_slots;
    }
    SearchCall call(*this, (uint32_t)noise_rows);
    const Games Gm = B.games.view(B.slots.counters.p, refill ? B.refill.area.p : nullptr);
    const Tree T = B.tree.view();
    const Slots S = B.slots.view(*this);
    const Segs G = B.segs.view(n_batches, B.slots.iter_cap);
    const uint32_t quirks = (flags & DIEE_FLAG_REF_QUIRKS) ? 1u : 0u;
    const PlayParams PP{cfg->round_limit, (float)(1.0 / (double)temperature), quirks};
    Delivery dl(call, Gm, G, bt, n_slots, frag_cap, outs != nullptr);

    upload_segments(*this, bt);
    nn_reset_timing(*this);
    launch_init_games(stream, Gm, G, n_games);
    std::vector<uint32_t> area0;                                        // slot refill: the first n_slots games are in flight, game g on area g; no area is free
    if (refill) {
        area0.resize(n_slots);
        for (uint32_t g = 0; g < n_slots; ++g) area0[g] = g;
        h2d(B.refill.area.p, area0.data(), area0.size());
        HIPCHK(hipMemsetAsync(B.refill.free_areas.p, 0, sizeof(uint32_t), stream));
    }
    draw_noise(B, 0, bt, 0, cfg->dir_alpha);
    sync();
    // ---- timed region: every input is resident in HBM ----
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t n_live = n_slots, step = 0;
    uint32_t next_game = n_slots;                                       // slot refill: the next unstarted game
    std::vector<uint32_t> steps_of(n_batches, 0);                       // move-steps each batch took part in
    std::vector<uint32_t> live_of(n_batches);
    auto started_of = [&](uint32_t k, uint32_t lo, uint32_t hi) {       // games of batch k among games [lo, hi)
        const uint32_t a = std::max(lo, game0[k]), b = std::min(hi, game0[k] + bt[k].n_games);
        return b > a ? b - a : 0u;
    };
    for (uint32_t k = 0; k < n_batches; ++k) live_of[k] = started_of(k, 0, n_slots);
    const bool trace_steps = opt.trace_steps != 0;                        // development: batch size of every move-step
    uint32_t* const live_host = B.segs.live_host;
    while (n_live > 0 && (max_steps == 0 || step < max_steps)) {       // alpha_parallel.rs:129
        if (trace_steps) fprintf(stderr, "[diee] move-step %u: %u games alive\n", step, n_live);
        for (uint32_t k = 0; k < n_batches; ++k) if (live_of[k]) steps_of[k] = step + 1;
        const int buf = (int)(step & 1u);
        HIPCHK(hipMemsetAsync(B.segs.span.p, 0, sizeof(uint32_t) * 2 * kMaxSegments, stream));
        launch_gather_roots(stream, Gm, S, G, n_live);
        HIPCHK(hipMemcpyAsync(B.slots.counters_bak.p, B.slots.counters.p, sizeof(unsigned long long) * CNT_COUNT * n_batches, hipMemcpyDeviceToDevice, stream));
        call.cur_step = step; net->cur_step = (int)std::min(step, kStepLog - 1);
        search_or_repeat(call, n_live, n_batches, *cfg, buf, flags,    // :146; rare: this move-step's search again, per-layer kernels
            [&] { HIPCHK(hipMemcpyAsync(B.slots.counters.p, B.slots.counters_bak.p, sizeof(unsigned long long) * CNT_COUNT * n_batches, hipMemcpyDeviceToDevice, stream)); },
            [&] {
                // while the GPU searches: the next move-step's Dirichlet samples (the only host arithmetic of a move-step) and the
                // previous move-step's records (enqueued behind this step's search so that the search never waits for the host)
                if (!refill || step + 1 < call.noise_rows) draw_noise(B, buf ^ 1, bt, step + 1, cfg->dir_alpha);
                dl.send_pending();
            });
        // slot refill: the areas of the games retired in step - 1 went to the games admitted behind them, whose first records are written now --
        // behind the gather of the retired games' records (send_pending above, on the copy stream).  The search has just covered that wait.
        if (refill) dl.wait_copied(buf ^ 1);
        launch_play_move(stream, T, Gm, G, n_live, step, PP);           // :164-224
        dl.wait_copied(buf);                                            // (step - 2's list has been read)
        launch_deliver_scan(stream, Gm, G, n_live, step, B.deliver.events[buf].p, B.segs.live_dev.p);
        if (refill) launch_refill_release(stream, Gm, n_live, B.refill.free_areas.p, n_slots);
        launch_compact_live(stream, Gm, n_live, n_batches, B.segs.live_dev.p);   // :226-228
        if (refill) launch_refill_admit(stream, Gm, B.segs.live_dev.p, n_slots, next_game, n_games, B.refill.free_areas.p);
        HIPCHK(hipGetLastError());
        d2h(live_host, B.segs.live_dev.p, (size_t)1 + 4 * n_batches);
        sync();
        n_live = live_host[0];
        for (uint32_t k = 0; k < n_batches; ++k) live_of[k] = live_host[1 + k];
        if (refill) {                                                   // what k_refill_admit appended to the live list
            const uint32_t add = std::min(n_slots - n_live, n_games - next_game);
            for (uint32_t k = 0; k < n_batches; ++k) live_of[k] += started_of(k, next_game, next_game + add);
            n_live += add; next_game += add;
        }
        dl.pending.assign(live_host, live_host + 1 + 4 * n_batches);
        dl.pending_buf = buf;
        ++step;
    }
    dl.finish();
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    check_overflow();
    std::vector<unsigned long long> step_log(2 * (size_t)kStepLog);
    d2h(step_log.data(), B.slots.step_log.p, step_log.size());
    sync();
    net->cur_step = -1;
    if (stats) {
        nn_harvest(*this, &stats[0], &step_log);                        // sampled tower timings: whole call, reported with batch 0
        for (uint32_t k = 0; k < n_batches; ++k) {
            read_counters(*this, k, &stats[k]);
            stats[k].move_steps = steps_of[k]; stats[k].seconds = secs; stats[k].fragments = dl.frag_total[k];
        }
        stats[0].deliver_seconds = dl.secs; stats[0].deliver_bytes = dl.bytes;
        call.report(stats[0]);
    } else {
        nn_harvest(*this, nullptr, &step_log);
    }
    if (dl.deliver)
        for (uint32_t k = 0; k < n_batches; ++k) dl.fb[k].release(&outs[k]);
}

}  // namespace diee
