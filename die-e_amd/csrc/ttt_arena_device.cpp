// ttt_arena_device.cpp -- host side of the tic-tac-toe device arena (ttt_arena_device.h): buffers, the round loop, the one copy-out.
#include "ttt_arena_device.h"

#include <chrono>
#include <cstring>

#include "engine.h"

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
    cap_ = 0;
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
                ++searches[s];
            } else if (a.agents[s] == DIEE_AGENT_MCTS) {                  // :303-306
                M.vout = vanilla_.enqueue(roots, keys, cnt[s], a.cfg, a.seed, quirks);
                ++searches[s];
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
    const uint32_t* state = (const uint32_t*)(h + kTaWords * sizeof(unsigned long long));
    const uint32_t* rr = state + n;
    const int8_t* win = (const int8_t*)(rr + n);
    if (tot[kTaOverflow]) throw EngineError(DIEE_ERR_CAPACITY, "k_ttt_vanilla: a game's slab is full");
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
            st.plies = t[kTaPlies]; st.fragments = t[kTaMoves]; st.games = t[kTaRetired]; st.move_steps = searches[s]; st.seconds = secs;
            st.nn_evals = t[kTaNnEvals]; st.nn_rows = t[kTaNnEvals]; st.expansions = t[kTaExpansions]; st.children = t[kTaChildren];
            st.max_children = t[kTaMaxChildren]; st.selections = t[kTaSelections]; st.depth_sum = t[kTaDepthSum]; st.terminal_hits = t[kTaTerminal];
        }
    }
    if (res) {
        memset(res, 0, sizeof *res);
        res->wins_p1 = (uint32_t)tot[kTaWins1]; res->wins_p2 = (uint32_t)tot[kTaWins2]; res->draws = (uint32_t)tot[kTaDraws];
        res->rounds = round; res->seconds = secs;
    }
}

}  // namespace ttt
}  // namespace diee
