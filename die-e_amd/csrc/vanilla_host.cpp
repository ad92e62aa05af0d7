// vanilla_host.cpp -- host side of Agent::Mcts: buffers, the launch loop and diee_mcts_vanilla_batch (kernels: vanilla_kernels.hip).
#include "vanilla_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "launch.h"

namespace diee {

struct VanillaBufs {
    DevBuf<BgState> state, roots;
    DevBuf<uint32_t> parent, nplays, ncreated, visits, play, head, next, done, used, game_id, round, out_play, n_children;
    DevBuf<float> value, ln, child_visits, child_values;
    DevBuf<unsigned long long> counters;                       // [2][slot_cap][VC_COUNT]
    uint32_t slot_cap = 0, node_cap = 0, ln_n = 0;
};
void free_vanilla(VanillaBufs* v) { delete v; }

void vanilla_check_cfg(const diee_mcts_cfg& cfg) {
    if (cfg.iterations >= (1u << 20)) throw EngineError(DIEE_ERR_ARG, "Agent::Mcts: iterations must be below 2^20 (the RNG counter is iteration << 12 | ply)");
    if (cfg.round_limit > 4094) throw EngineError(DIEE_ERR_ARG, "Agent::Mcts: round_limit (simulate_round_limit) must be at most 4094 (the RNG counter is iteration << 12 | ply)");
}

Vanilla vanilla_reserve(Engine& e, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t flags, uint32_t side) {
    vanilla_check_cfg(cfg);
    if (!e.vanilla) e.vanilla = new VanillaBufs();
    VanillaBufs& B = *e.vanilla;
    const uint32_t want_cap = cfg.iterations + 1;
    if (n > B.slot_cap || want_cap > B.node_cap) {
        const uint32_t sc = std::max(n, B.slot_cap), nc = std::max(want_cap, B.node_cap);
        const size_t N = (size_t)sc * nc;
        B.state.ensure(N); B.parent.ensure(N); B.nplays.ensure(N); B.ncreated.ensure(N); B.visits.ensure(N); B.value.ensure(N);
        B.play.ensure(N); B.head.ensure(N); B.next.ensure(N);
        B.roots.ensure(sc); B.done.ensure(sc); B.used.ensure(sc); B.game_id.ensure(sc); B.round.ensure(sc); B.out_play.ensure(sc);
        B.n_children.ensure(sc);
        B.counters.ensure(2 * (size_t)sc * VC_COUNT);
        B.slot_cap = sc; B.node_cap = nc;
        vanilla_zero_counters(e);
    }
    if (cfg.iterations + 2 > B.ln_n) {                         // ln is not reproducible between libm and the device: one table, built here
        std::vector<float> ln(cfg.iterations + 2, 0.0f);
        for (uint32_t k = 1; k < ln.size(); ++k) ln[k] = (float)std::log((double)k);
        B.ln.ensure(ln.size());
        e.h2d(B.ln.p, ln.data(), ln.size());
        e.sync();                                               // (the vector is stack-scoped)
        B.ln_n = (uint32_t)ln.size();
    }
    const uint32_t quirks = (flags & DIEE_FLAG_REF_QUIRKS) ? 1u : 0u;
    // a launch stays far below a second: a rollout ply is one legal-play enumeration (microseconds), an iteration plays at most
    // round_limit of them -- or none under the quirks, where it is one enumeration
    uint32_t budget = e.opt.vanilla_iters_per_launch;
    if (budget == 0) budget = quirks ? 4096u : std::max(1u, 16384u / (cfg.round_limit + 1u));
    return Vanilla{B.state.p, B.parent.p, B.nplays.p, B.ncreated.p, B.visits.p, B.value.p, B.play.p, B.head.p, B.next.p, B.done.p, B.used.p,
                   B.roots.p, B.game_id.p, B.round.p, B.ln.p, B.counters.p + (size_t)side * B.slot_cap * VC_COUNT, B.out_play.p, e.flags_dev.p,
                   (unsigned long long)seed, B.node_cap, cfg.iterations, cfg.round_limit, budget, quirks, cfg.c};
}

void vanilla_search(Engine& e, const Vanilla& V, uint32_t n, uint32_t* n_children, float* child_visits, float* child_values, uint32_t cap) {
    launch_vanilla_init(e.stream, V, n);
    // every game runs exactly V.iterations iterations (or none): the number of launches is known, nothing is read back in between
    for (uint32_t done = 0; done < V.iterations; done += std::min(V.budget, V.iterations - done)) launch_vanilla(e.stream, V, n);
    launch_vanilla_result(e.stream, V, n, n_children, child_visits, child_values, cap);
    HIPCHK(hipGetLastError());
}

void vanilla_zero_counters(Engine& e) {
    VanillaBufs& B = *e.vanilla;
    HIPCHK(hipMemsetAsync(B.counters.p, 0, sizeof(unsigned long long) * 2 * (size_t)B.slot_cap * VC_COUNT, e.stream));
}

void vanilla_read_counters(Engine& e, uint32_t side, diee_vanilla_stats* out) {
    VanillaBufs& B = *e.vanilla;
    std::vector<unsigned long long> c((size_t)B.slot_cap * VC_COUNT);
    e.d2h(c.data(), B.counters.p + (size_t)side * B.slot_cap * VC_COUNT, c.size());
    e.sync();
    unsigned long long t[VC_COUNT] = {};
    for (size_t i = 0; i < c.size(); ++i) t[i % VC_COUNT] += c[i];
    out->iterations = t[VC_ITERATIONS]; out->expansions = t[VC_EXPANSIONS]; out->terminal_hits = t[VC_TERMINAL];
    out->dead_end_hits = t[VC_DEAD_END]; out->rollouts = t[VC_ROLLOUTS]; out->rollout_plies = t[VC_PLIES];
    out->rollout_decided = t[VC_DECIDED]; out->depth_sum = t[VC_DEPTH_SUM];
}

// mct_search (simple_mcts.rs:10-39) for n roots, as get_actions_for_player calls it per game (versus.rs:303-306)
void Engine::mcts_vanilla_batch(const diee_bg_state* roots, uint32_t n, const diee_mcts_cfg* cfg, uint64_t seed, const uint32_t* game_ids,
                                const uint32_t* rounds, uint32_t flags, int8_t* plays, uint32_t* n_children, float* child_visits,
                                float* child_values, uint32_t cap, diee_vanilla_stats* stats) {
    HIPCHK(hipSetDevice(device));
    if (stats) memset(stats, 0, sizeof *stats);
    vanilla_check_cfg(*cfg);
    if (!n) return;
    for (uint32_t i = 0; i < n; ++i)
        if (roots[i].roll[0] == 0 && roots[i].roll[1] == 0) throw EngineError(DIEE_ERR_ARG, "die has not been rolled (backgammon_logic.rs:404)");
    if ((child_visits || child_values) && cap == 0) throw EngineError(DIEE_ERR_ARG, "child_visits / child_values need cap >= 1");
    const Vanilla V = vanilla_reserve(*this, n, *cfg, seed, flags);
    VanillaBufs& B = *vanilla;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> ids(n), rds(n);
    for (uint32_t i = 0; i < n; ++i) { ids[i] = game_ids ? game_ids[i] : i; rds[i] = rounds ? rounds[i] : 0; }
    h2d((uint8_t*)B.roots.p, (const uint8_t*)roots, (size_t)n * 32);
    h2d(B.game_id.p, ids.data(), (size_t)n); h2d(B.round.p, rds.data(), (size_t)n);
    vanilla_zero_counters(*this);
    const size_t rows = (size_t)n * cap;
    if (child_visits) { B.child_visits.ensure(rows); HIPCHK(hipMemsetAsync(B.child_visits.p, 0, rows * sizeof(float), stream)); }
    if (child_values) { B.child_values.ensure(rows); HIPCHK(hipMemsetAsync(B.child_values.p, 0, rows * sizeof(float), stream)); }
    vanilla_search(*this, V, n, B.n_children.p, child_visits ? B.child_visits.p : nullptr, child_values ? B.child_values.p : nullptr, cap);
    d2h((uint8_t*)plays, (const uint8_t*)B.out_play.p, (size_t)n * 4);
    if (n_children) d2h(n_children, B.n_children.p, (size_t)n);
    if (child_visits) d2h(child_visits, B.child_visits.p, rows);
    if (child_values) d2h(child_values, B.child_values.p, rows);
    sync();
    if (stats) {
        vanilla_read_counters(*this, 0, stats);
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    check_overflow();
}

}  // namespace diee
