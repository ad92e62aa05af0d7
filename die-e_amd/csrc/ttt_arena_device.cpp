// ttt_arena_device.cpp -- host side of the tic-tac-toe device arena (ttt_arena_device.h): buffers, the round loop or the one launch of
// k_ttt_arena_run, the one copy-out.
#include "ttt_arena_device.h"

#include <chrono>
#include <cstring>

#include "engine.h"
#include "search_host.h"

namespace diee {
namespace ttt {

namespace {
void drop(void*& p, bool host) {
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    p = nullptr;
}
size_t out_bytes(uint32_t n) { return kTaWords * sizeof(unsigned long long) + (size_t)n * (4 + 4 + 1 + 1); }
}  // namespace

DeviceArena::~DeviceArena() {
    if (hipSetDevice(net_.device()) != hipSuccess) return;
    (void)hipStreamSynchronize(net_.stream());
    release();
}

void DeviceArena::release() {
    drop(d_out_, false); drop(h_out_, true); drop(d_work_, false); drop(h_counts_, true);
    drop(d_run_, false); drop(h_run_, true); drop(d_nodes_, false);
    cap_ = 0; cap_run_ = 0; cap_nodes_ = 0;
}

// k_ttt_arena_run has k_ttt_search_run's registers: one workgroup per CU.  A call of more workgroups than CUs would run in passes, each
// pass as long as its longest game; it goes to the round loop, whose searches shrink as games retire.
bool DeviceArena::serves(const ArenaArgs& a) {
    if (search_.fused_level() != 2 || a.cfg.iterations > kRunMaxIters) return false;
    for (int s = 0; s < 2; ++s) {
        if (a.agents[s] != DIEE_AGENT_MODEL && a.agents[s] != DIEE_AGENT_RANDOM) return false;      // k_ttt_vanilla is no device function of the family
        if (a.agents[s] == DIEE_AGENT_MODEL && (a.flags[s] & DIEE_FLAG_REF_QUIRKS) != 0) return false;      // Q14 couples the slots of a search
    }
    int cus = 0, lds = 0;
    search_.limits(cus, lds);
    return arena_run_groups(a.n_games) <= (uint32_t)cus;
}

// As reserve(): a buffer that has to grow is freed first and its capacity cleared.
void DeviceArena::reserve_run(size_t bytes, size_t nodes) {
    if (bytes <= cap_run_ && nodes <= cap_nodes_) return;
    HIPCHK(hipStreamSynchronize(net_.stream()));
    if (bytes > cap_run_) {
        size_t cap = 64 * 1024;
        while (cap < bytes) cap *= 2;
        drop(d_run_, false); drop(h_run_, true);
        cap_run_ = 0;
        HIPCHK(hipMalloc(&d_run_, cap));
        HIPCHK(hipHostMalloc(&h_run_, cap));
        cap_run_ = cap;
    }
    if (nodes > cap_nodes_) {
        size_t cap = 64 * 1024;
        while (cap < nodes) cap *= 2;
        drop(d_nodes_, false);
        cap_nodes_ = 0;
        HIPCHK(hipMalloc(&d_nodes_, cap * sizeof(RunNode)));
        cap_nodes_ = cap;
    }
}

bool DeviceArena::run_one_launch(const ArenaArgs& a, diee_arena_result* res, int8_t* winner, uint32_t* retired_round, int8_t* retired_side,
                                 diee_ttt_state* final_states, diee_stats* stats) {
    const uint32_t n = a.n_games, iters = a.cfg.iterations;
    bool any_model = false;
    for (int s = 0; s < 2; ++s) any_model = any_model || a.agents[s] == DIEE_AGENT_MODEL;
    HIPCHK(hipSetDevice(net_.device()));
    int cus = 0, lds = 0;
    search_.limits(cus, lds);
    const bool lds_tree = iters <= kRunLdsIters && lds >= 160 * 1024;
    const size_t head = sizeof(ArHead) + (size_t)2 * kArRounds * iters * 4, bytes = head + (size_t)n * (4 + 4 + 1 + 1);
    try { reserve_run(bytes, any_model && !lds_tree ? (size_t)n * run_node_bound(iters) : 0); } catch (...) { (void)hipGetLastError(); throw; }
    hipStream_t stream = net_.stream();

    ArParams P{};
    P.sp.nodes = (RunNode*)d_nodes_;
    P.sp.n = n; P.sp.iterations = iters; P.sp.slab = run_node_bound(iters); P.sp.quirks = 0u;
    P.sp.c = a.cfg.c; P.sp.eps = a.cfg.dir_eps; P.sp.one_minus_eps = 1.0f - a.cfg.dir_eps;
    unsigned char* o = (unsigned char*)d_run_;
    P.head = (ArHead*)o;
    P.any_selected = (uint32_t*)(o + sizeof(ArHead));
    P.state = (uint32_t*)(o + head);
    P.retired_round = P.state + n;
    P.winner = (int8_t*)(P.retired_round + n);
    P.retired_side = P.winner + n;
    P.seed = a.seed; P.round_limit = a.round_limit; P.inv_t = (float)(1.0 / (double)a.temperature);
    P.rounds = a.max_rounds != 0 && a.max_rounds < kArRounds ? a.max_rounds : kArRounds;
    for (uint32_t s = 0; s < 2; ++s) {
        P.agents[s] = a.agents[s];
        if (a.agents[s] != DIEE_AGENT_MODEL) continue;
        P.nets[s] = *a.nets[s];
        for (uint32_t r = 0; r < P.rounds; ++r) dirichlet_host(a.seed, 2 * r + s, a.cfg.dir_alpha, A, P.noise[2 * r + s]);      // as DeviceSearch::enqueue for (seed, step)
    }

    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemsetAsync(d_run_, 0, head, stream));
    HIPCHK(launch_ttt_arena_run(stream, P, lds_tree, lds_tree && !lds_asked_));
    lds_asked_ = lds_asked_ || lds_tree;
    HIPCHK(hipMemcpyAsync(h_run_, d_run_, bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    const unsigned char* h = (const unsigned char*)h_run_;
    const ArHead* H = (const ArHead*)h;
    if (H->alive != 0u && (a.max_rounds == 0 || a.max_rounds > kArRounds)) return false;       // skipped turns: the round loop plays the call
    const uint32_t* flag = (const uint32_t*)(h + sizeof(ArHead));
    unsigned long long tot[kTaWords];
    memcpy(tot, H->totals, sizeof tot);
    uint64_t move_steps[2] = {0, 0};
    uint32_t rounds = P.rounds;
    for (uint32_t r = P.rounds; r-- > 0;) {
        if (H->live[2 * r] + H->live[2 * r + 1] == 0u) rounds = r;                            // the first round with nobody alive
        for (uint32_t s = 0; s < 2; ++s) {
            const uint32_t step = 2 * r + s;
            if (a.agents[s] != DIEE_AGENT_MODEL || H->live[step] == 0u) continue;
            uint64_t evals = 1;                                                                // the roots, then one per iteration somebody selected in
            for (uint32_t k = 0; k < iters; ++k) evals += flag[(size_t)step * iters + k] != 0u;
            tot[(size_t)s * kTaPlayerWords + kTaNnEvals] += evals * H->live[step];
            move_steps[s] += 1;
        }
    }
    last_launches_ = 1;
    decode(a, tot, (const uint32_t*)(h + head), move_steps, rounds, secs, res, winner, retired_round, retired_side, final_states, stats);
    return true;
}

// As the searches' buffers: freed before they grow, so a failed allocation leaves the ctx consistent and nothing has been launched.
void DeviceArena::reserve(uint32_t n) {
    if (n <= cap_) return;
    HIPCHK(hipStreamSynchronize(net_.stream()));
    release();
    size_t cap = 1024;
    while (cap < n) cap *= 2;                                             // (n <= 2^22)
    HIPCHK(hipMalloc(&d_out_, out_bytes((uint32_t)cap)));
    HIPCHK(hipHostMalloc(&h_out_, out_bytes((uint32_t)cap)));
    HIPCHK(hipMalloc(&d_work_, cap * (2 * sizeof(diee_ttt_state) + 4 * 4 + 4) + 16));
    HIPCHK(hipHostMalloc(&h_counts_, 16));
    cap_ = (uint32_t)cap;
}

void DeviceArena::run(const ArenaArgs& a, diee_arena_result* res, int8_t* winner, uint32_t* retired_round, int8_t* retired_side,
                      diee_ttt_state* final_states, diee_stats* stats) {
    const uint32_t n = a.n_games;
    bool any_model = false, any_mcts = false;
    for (int s = 0; s < 2; ++s) { any_model = any_model || a.agents[s] == DIEE_AGENT_MODEL; any_mcts = any_mcts || a.agents[s] == DIEE_AGENT_MCTS; }
    HIPCHK(hipSetDevice(net_.device()));
    try { reserve(n); } catch (...) { (void)hipGetLastError(); release(); throw; }
    const bool any_quirks = ((a.flags[0] | a.flags[1]) & DIEE_FLAG_REF_QUIRKS) != 0;
    if (any_model) { try { search_.reserve(n, a.cfg.iterations, any_quirks); } catch (...) { (void)hipGetLastError(); throw; } }
    if (any_mcts) vanilla_.reserve_for(n, a.cfg);
    hipStream_t stream = net_.stream();

    ArenaGames G{};
    unsigned char* o = (unsigned char*)d_out_;
    G.totals = (unsigned long long*)o;
    G.state = (uint32_t*)(o + kTaWords * sizeof(unsigned long long));
    G.retired_round = G.state + n;
    G.winner = (int8_t*)(G.retired_round + n);
    G.retired_side = G.winner + n;
    G.roots = (diee_ttt_state*)d_work_;                                   // 32-byte records first: they are stored 16 bytes at a time
    G.keys = (uint32_t*)(G.roots + 2 * (size_t)n);
    G.live = G.keys + 4 * (size_t)n;
    G.counts = G.live + n;
    G.n_games = n;

    const float inv_t = (float)(1.0 / (double)a.temperature);
    uint32_t* const counts = (uint32_t*)h_counts_;
    launch_ttt_arena_init(stream, G);
    HIPCHK(hipGetLastError());
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t n_live = n, round = 0;
    uint64_t searches[2] = {0, 0};
    uint32_t launches = 0;                                                // search-kernel launches: option arena_last_launches
    for (;;) {                                                            // versus.rs:191
        launch_ttt_arena_split(stream, G, n_live, round);                 // :195-196
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(counts, G.counts, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        const uint32_t cnt[2] = {counts[0], counts[1]};
        n_live = counts[2];
        if (n_live == 0 || (a.max_rounds != 0 && round >= a.max_rounds)) break;
        for (uint32_t s = 0; s < 2; ++s) {
            if (!cnt[s]) continue;
            const diee_ttt_state* roots = G.roots + (size_t)s * n;
            const uint32_t* keys = G.keys + 2 * (size_t)s * n;
            const bool quirks = (a.flags[s] & DIEE_FLAG_REF_QUIRKS) != 0;
            ArenaMove M{};
            M.seed = a.seed; M.n = cnt[s]; M.side = s; M.round = round; M.round_limit = a.round_limit; M.iterations = a.cfg.iterations; M.inv_t = inv_t;
            if (a.agents[s] == DIEE_AGENT_MODEL) {                        // :279-283
                const DeviceSearch::Enqueued E = search_.enqueue(roots, cnt[s], *a.nets[s], a.cfg, a.seed, 2 * round + s, quirks);
                M.probs = E.probs; M.n_children = E.n_children; M.counters = E.counters; M.any_selected = E.any_selected;
                ++searches[s]; launches += search_.last_launches();
            } else if (a.agents[s] == DIEE_AGENT_MCTS) {                  // :303-306
                M.vout = vanilla_.enqueue(roots, keys, cnt[s], a.cfg, a.seed, quirks);
                ++searches[s]; launches += 1;
            }
            launch_ttt_arena_move(stream, G, M, a.agents[s]);             // :220-266
            HIPCHK(hipGetLastError());
        }
        ++round;                                                          // :219
    }
    HIPCHK(hipMemcpyAsync(h_out_, d_out_, out_bytes(n), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    const unsigned char* h = (const unsigned char*)h_out_;
    const unsigned long long* tot = (const unsigned long long*)h;
    if (tot[kTaOverflow]) throw EngineError(DIEE_ERR_CAPACITY, "k_ttt_vanilla: a game's slab is full");
    last_launches_ = launches;
    decode(a, tot, (const uint32_t*)(h + kTaWords * sizeof(unsigned long long)), searches, round, secs, res, winner, retired_round, retired_side,
           final_states, stats);
}

// the outputs of diee_ttt_arena from the call's totals and its per-game block: state | retired_round | winner | retired_side
void DeviceArena::decode(const ArenaArgs& a, const unsigned long long* tot, const uint32_t* state, const uint64_t move_steps[2], uint32_t rounds, double secs,
                         diee_arena_result* res, int8_t* winner, uint32_t* retired_round, int8_t* retired_side, diee_ttt_state* final_states,
                         diee_stats* stats) {
    const uint32_t n = a.n_games;
    const uint32_t* rr = state + n;
    const int8_t* win = (const int8_t*)(rr + n);
    if (winner) memcpy(winner, win, n);
    if (retired_round) memcpy(retired_round, rr, (size_t)n * sizeof(uint32_t));
    if (retired_side) memcpy(retired_side, win + n, n);
    if (final_states) {
        memset(final_states, 0, (size_t)n * sizeof(diee_ttt_state));
        for (uint32_t g = 0; g < n; ++g) {
            for (int c = 0; c < 9; ++c) { const uint32_t v = (state[g] >> (2 * c)) & 3u; final_states[g].board[c] = v == 3u ? -1 : (int8_t)v; }
            final_states[g].player = (state[g] >> 18) & 1u ? 1 : -1;
        }
    }
    if (stats) {
        memset(stats, 0, 2 * sizeof(diee_stats));
        for (int s = 0; s < 2; ++s) {
            const unsigned long long* t = tot + (size_t)s * kTaPlayerWords;
            diee_stats& st = stats[s];
            st.plies = t[kTaPlies]; st.fragments = t[kTaMoves]; st.games = t[kTaRetired]; st.move_steps = move_steps[s]; st.seconds = secs;
            st.nn_evals = t[kTaNnEvals]; st.nn_rows = t[kTaNnEvals]; st.expansions = t[kTaExpansions]; st.children = t[kTaChildren];
            st.max_children = t[kTaMaxChildren]; st.selections = t[kTaSelections]; st.depth_sum = t[kTaDepthSum]; st.terminal_hits = t[kTaTerminal];
        }
    }
    if (res) {
        memset(res, 0, sizeof *res);
        res->wins_p1 = (uint32_t)tot[kTaWins1]; res->wins_p2 = (uint32_t)tot[kTaWins2]; res->draws = (uint32_t)tot[kTaDraws];
        res->rounds = rounds; res->seconds = secs;
    }
}

}  // namespace ttt
}  // namespace diee
