// arena_host.cpp -- host driver of the arena: model-vs-model games of one call, both agents' turns on the device.
// Reference call structure: play() (src/versus.rs:160-318).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "search_host.h"
#include "vanilla_host.h"

namespace diee {

static_assert(sizeof(diee_turn) == sizeof(ArenaTurn), "the device's turn record is the ABI's");

void SearchBufs::Arena::reserve(uint32_t n_games) {
    state.ensure(n_games); initial.ensure(n_games); alive.ensure(n_games); winner.ensure(n_games); side.ensure(n_games);
    round.ensure(n_games); live.ensure(n_games); list.ensure(2 * (size_t)n_games); words.ensure(AW_COUNT);
}

// play() of versus.rs:160-268 with both agents' turns on the device.  Per round: ONE device->host read (the two sides' counts and
// the games alive, k_arena_split), then for each side with games to move { gather its list into the slots, search it with that
// player's network (mcts_run, unchanged: e.net points at it for the duration), play its moves }.  Both sides' trees share the slot
// space, so a side's moves are played before the other side searches; a game is in one list only, which makes that the same as the
// reference's "collect the actions of both, then apply".
void Engine::arena(NetWeights* net1, int agent1, NetWeights* net2, int agent2, uint32_t n_games, const diee_mcts_cfg* cfg, float temperature,
                   uint64_t seed, uint32_t round_limit, uint32_t max_rounds, const uint32_t flags[2], diee_arena_log* log, diee_arena_result* res,
                   int8_t* winner, uint32_t* retired_round, int8_t* retired_side, diee_bg_state* initial_states, diee_bg_state* final_states,
                   diee_stats* stats) {
    HIPCHK(hipSetDevice(device));
    if (log) memset(log, 0, sizeof *log);
    if (res) memset(res, 0, sizeof *res);
    if (stats) memset(stats, 0, sizeof(diee_stats) * 2);
    if (n_games == 0 || round_limit == 0) throw EngineError(DIEE_ERR_ARG, "the arena needs n_games >= 1 and round_limit >= 1");
    if (n_games > (1u << 22)) throw EngineError(DIEE_ERR_ARG, "too many games in flight");
    NetWeights* const nets[2] = {net1, net2};
    const int agents[2] = {agent1, agent2};
    for (int s = 0; s < 2; ++s) {
        if (agents[s] != DIEE_AGENT_RANDOM && agents[s] != DIEE_AGENT_MODEL && agents[s] != DIEE_AGENT_MCTS)
            throw EngineError(DIEE_ERR_ARG, "agent: DIEE_AGENT_RANDOM, DIEE_AGENT_MODEL or DIEE_AGENT_MCTS");
        if (agents[s] == DIEE_AGENT_MODEL && (!nets[s] || !nets[s]->loaded)) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called for a Model agent's ctx");
    }
    const bool any_model = agent1 == DIEE_AGENT_MODEL || agent2 == DIEE_AGENT_MODEL, any_mcts = agent1 == DIEE_AGENT_MCTS || agent2 == DIEE_AGENT_MCTS;
    if (any_mcts) vanilla_check_cfg(*cfg);
    reserve_search(*this, n_games, any_mcts && !any_model ? 0u : cfg->iterations);      // (the Model searches' tree arena: a vanilla search has its own slabs)
    SearchBufs& B = *search;
    const bool base_inv[2] = {net1 && net1->invariant, net2 && net2->invariant};     // (as the ctxs were set before this call)
    // the two networks for the duration of the call: no sampled timing (as in mcts_batch), DIEE_FLAG_INVARIANT_NN, activations for n_games rows
    struct NetScope {
        Engine& e; NetWeights* own; NetWeights* w[2] = {nullptr, nullptr}; bool inv[2]; int se[2];
        ~NetScope() { for (int s = 0; s < 2; ++s) if (w[s]) { w[s]->invariant = inv[s]; w[s]->sample_every = se[s]; } e.net = own; }
    } scope{*this, net};
    for (int s = 0; s < 2; ++s) {
        if (agents[s] != DIEE_AGENT_MODEL || (s == 1 && scope.w[0] == nets[1])) continue;
        NetWeights* w = nets[s];
        scope.w[s] = w; scope.inv[s] = w->invariant; scope.se[s] = w->sample_every;
        if (flags[s] & DIEE_FLAG_INVARIANT_NN) w->invariant = true;
        w->sample_every = 0; w->cur_step = 0;
        net = w;
        nn_reserve(*this, (int)n_games);
    }
    B.arena.reserve(n_games);
    const Arena A = B.arena.view(n_games);
    const Segs G = B.segs.view(1, B.slots.iter_cap);
    // every search is ONE batch (one alpha_mcts_parallel call) of the call's seed; its counters collect in row 0 of the counter table, the
    // two players' running totals are kept in rows 1 and 2
    const std::vector<diee_batch> one{{n_games, 0u, seed}};
    upload_segments(*this, one);
    unsigned long long* const cnt0 = B.slots.counters.p;
    auto acc = [&](int s) { return B.slots.counters.p + (size_t)(1 + s) * CNT_COUNT; };
    SearchCall call(*this);                                             // (its launch-count hints: one pair per player, SearchCall::side)
    if (any_mcts) {                                                     // the slabs for the call's widest search; one counter block per player
        (void)vanilla_reserve(*this, n_games, *cfg, seed, flags[0]);
        vanilla_zero_counters(*this);
    }
    launch_arena_init(stream, A, seed);
    HIPCHK(hipGetLastError());
    sync();
    const auto t0 = std::chrono::steady_clock::now();
    const float inv_t = (float)(1.0 / (double)temperature);
    uint32_t n_live = n_games, round = 0;
    uint64_t searches[2] = {0, 0}, bands[2][DIEE_BANDS] = {};
    static const uint32_t kBandBounds[DIEE_BANDS - 1] = {16, 32, 64, 128, 256, 512, 928, 1024};
    uint32_t* const live_host = B.segs.live_host;
    // the turn log (search_types.h, ArenaTurn): round-major rows of n_games records in chunks of opt.arena_log_rounds rounds, allocated as the
    // rounds go by -- nothing is moved, and how many rounds a call plays need not be known (round_limit does not bound them)
    struct LogChunk { DevBuf<ArenaTurn> rows; uint32_t first_round = 0, rounds = 0; };
    std::vector<std::unique_ptr<LogChunk>> chunks;
    const size_t row_bytes = (size_t)n_games * sizeof(ArenaTurn), log_cap = (size_t)opt.arena_log_mb << 20;
    size_t log_bytes = 0;
    auto log_row = [&](uint32_t r) -> ArenaTurn* {
        if (!log) return nullptr;
        if (chunks.empty() || r >= chunks.back()->first_round + chunks.back()->rounds) {
            const size_t fit = (log_cap - std::min(log_cap, log_bytes)) / row_bytes;
            const uint32_t rounds = (uint32_t)std::min<size_t>(opt.arena_log_rounds ? opt.arena_log_rounds : 1u, fit);
            if (!rounds)
                throw EngineError(DIEE_ERR_CAPACITY, "the turn log of round " + std::to_string(r) + " does not fit option arena_log_mb = " +
                                                         std::to_string(opt.arena_log_mb) + " (the round was not played)");
            chunks.emplace_back(new LogChunk());
            chunks.back()->rows.ensure((size_t)rounds * n_games);
            chunks.back()->first_round = r; chunks.back()->rounds = rounds;
            log_bytes += (size_t)rounds * row_bytes;
        }
        return chunks.back()->rows.p + (size_t)(r - chunks.back()->first_round) * n_games;
    };
    for (;;) {                                                          // versus.rs:191
        launch_arena_split(stream, A, n_live);                         // :195-196
        HIPCHK(hipGetLastError());
        d2h(live_host, A.words + AW_COUNT0, 3);
        sync();
        const uint32_t cnt[2] = {live_host[0], live_host[1]};
        n_live = live_host[2];
        if (n_live == 0 || (max_rounds != 0 && round >= max_rounds)) break;
        if (opt.trace_steps) fprintf(stderr, "[diee] arena round %u: %u + %u games to move\n", round, cnt[0], cnt[1]);
        ArenaTurn* const row = log_row(round);                          // (before anything of the round is enqueued)
        for (uint32_t s = 0; s < 2; ++s) {
            if (!cnt[s]) continue;
            uint32_t b = 0;
            while (b < DIEE_BANDS - 1 && cnt[s] > kBandBounds[b]) ++b;
            ++bands[s][b];
            if (agents[s] == DIEE_AGENT_MODEL) {                        // :279-283
                net = nets[s];
                net->invariant = base_inv[s] || (flags[s] & DIEE_FLAG_INVARIANT_NN);     // (the two players may share one network)
                draw_noise(B, (int)s, one, 2 * round + s, cfg->dir_alpha);      // (buffer s was last read by round - 1's search: complete, the split's sync is behind it)
                launch_arena_gather(stream, A, B.slots.view(*this), G, s, cnt[s], round);
                auto load_totals = [&] { HIPCHK(hipMemcpyAsync(cnt0, acc((int)s), sizeof(unsigned long long) * CNT_COUNT, hipMemcpyDeviceToDevice, stream)); };
                load_totals();
                call.cur_step = round; call.side = s;
                // (a starved hand-over drops the cluster / pair tower of THIS player's network for the rest of the process, by the hosting ctx's options;
                // rare: this search again on the per-layer kernels, before the moves are played)
                search_or_repeat(call, cnt[s], 1, *cfg, (int)s, flags[s], load_totals);
                HIPCHK(hipMemcpyAsync(acc((int)s), cnt0, sizeof(unsigned long long) * CNT_COUNT, hipMemcpyDeviceToDevice, stream));
                ++searches[s];
            }
            const uint32_t* mcts_play = nullptr;
            if (agents[s] == DIEE_AGENT_MCTS) {                         // :303-306
                const Vanilla V = vanilla_reserve(*this, cnt[s], *cfg, seed, flags[s], s);
                launch_vanilla_gather(stream, A, s, cnt[s], round, V.roots, V.game_id, V.round);
                vanilla_search(*this, V, cnt[s]);
                mcts_play = V.out_play;
                ++searches[s];
            }
            const ArenaParams P{seed, round, round_limit, inv_t, s, (uint32_t)agents[s], row};
            launch_arena_move(stream, B.tree.view(), A, cnt[s], P, flags_dev.p, mcts_play);      // :220-266
        }
        HIPCHK(hipGetLastError());
        ++round;                                                        // :219
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    check_overflow();
    uint32_t words[AW_COUNT];
    d2h(words, A.words, (size_t)AW_COUNT);
    std::vector<uint32_t> rr_log;                                       // the log needs the retired rounds whether the caller asked for them or not
    std::vector<ArenaTurn> rows_host;
    if (log) {
        rr_log.resize(n_games);
        if (!retired_round) retired_round = rr_log.data();
        rows_host.resize((size_t)round * n_games);
        for (const auto& c : chunks) {
            if (c->first_round >= round) break;
            d2h(rows_host.data() + (size_t)c->first_round * n_games, c->rows.p, (size_t)std::min(c->rounds, round - c->first_round) * n_games);
        }
    }
    if (winner) d2h(winner, A.winner, (size_t)n_games);
    if (retired_round) d2h(retired_round, A.retired_round, (size_t)n_games);
    if (retired_side) d2h(retired_side, A.retired_side, (size_t)n_games);
    if (initial_states) d2h((uint8_t*)initial_states, (const uint8_t*)A.initial, (size_t)n_games * 32);
    if (final_states) d2h((uint8_t*)final_states, (const uint8_t*)A.state, (size_t)n_games * 32);
    sync();
    diee_stats st[2];
    memset(st, 0, sizeof st);
    for (int s = 0; s < 2; ++s) {
        read_counters(*this, (uint32_t)(1 + s), &st[s]);
        st[s].seconds = secs; st[s].move_steps = searches[s];
        st[s].plies = words[AW_TURNS0 + s]; st[s].fragments = words[AW_MOVES0 + s]; st[s].games = words[AW_RETIRED0 + s];
        for (uint32_t b = 0; b < DIEE_BANDS; ++b) st[s].band_launches[b] = bands[s][b];
        if (agents[s] == DIEE_AGENT_MCTS) {                             // the fields that have a meaning for a vanilla search
            diee_vanilla_stats vs;
            vanilla_read_counters(*this, (uint32_t)s, &vs);
            st[s].selections = vs.iterations; st[s].expansions = vs.expansions; st[s].terminal_hits = vs.terminal_hits; st[s].depth_sum = vs.depth_sum;
        }
    }
    call.report(st[0]);
    if (log) {
        // rows -> game-major: game g's turns are rounds 0 ... retired_round[g], or every round played for a game still alive; the records
        // of the rounds after a game retired were never written and are not read.  One block: first[n_games + 1], then the turns
        std::vector<uint64_t> first((size_t)n_games + 1, 0);
        for (uint32_t g = 0; g < n_games; ++g) first[g + 1] = first[g] + (retired_round[g] == 0xFFFFFFFFu ? round : retired_round[g] + 1u);
        const size_t head = sizeof(uint64_t) * ((size_t)n_games + 1);                     // (a multiple of 8: the turns are aligned)
        char* const block = (char*)malloc(head + sizeof(diee_turn) * std::max<uint64_t>(first[n_games], 1));
        if (!block) throw std::bad_alloc();
        memcpy(block, first.data(), head);
        diee_turn* const turns = (diee_turn*)(block + head);
        for (uint32_t g = 0; g < n_games; ++g)
            for (uint64_t t = 0; t < first[g + 1] - first[g]; ++t) memcpy(&turns[first[g] + t], &rows_host[(size_t)t * n_games + g], sizeof(diee_turn));
        log->turns = turns; log->first = (uint64_t*)block; log->n_games = n_games; log->owner = block;
    }
    if (stats) memcpy(stats, st, sizeof st);
    if (res) {
        res->wins_p1 = words[AW_WINS1]; res->wins_p2 = words[AW_WINS2]; res->draws = words[AW_DRAWS];
        res->rounds = round; res->illegal_decodes = st[0].illegal_decodes + st[1].illegal_decodes; res->seconds = secs;
    }
}

}  // namespace diee
