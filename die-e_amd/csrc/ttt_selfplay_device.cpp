// ttt_selfplay_device.cpp -- host side of the one-launch tic-tac-toe self-play (ttt_selfplay_device.h): buffers, the three launches, the
// copy-out, the statistics.
#include "ttt_selfplay_device.h"

#include <cstdlib>
#include <cstring>
#include <new>

#include "engine.h"
#include "search_host.h"

namespace diee {
namespace ttt {

namespace {
// the capacity that holds `need`: doubling from `from`
size_t grown(size_t cap, size_t need, size_t from) {
    if (cap == 0) cap = from;
    while (cap < need) cap = cap > (~(size_t)0) / 2 ? need : cap * 2;
    return cap;
}
void drop(void*& p, bool host) {
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    p = nullptr;
}
}  // namespace

DeviceSelfPlay::~DeviceSelfPlay() {
    if (hipSetDevice(net_.device()) != hipSuccess) return;
    (void)hipStreamSynchronize(net_.stream());
    release();
}

void DeviceSelfPlay::release() {
    drop(d_frags_, false); drop(d_games_, false); drop(d_first_, false); drop(d_rec_, false); drop(h_rec_, true);
    drop(d_head_, false); drop(h_head_, true); drop(d_nodes_, false);
    cap_n_ = 0; cap_head_ = 0; cap_nodes_ = 0;
}

// k_ttt_selfplay_run has k_ttt_search_run's registers: one workgroup per CU.  A call of more workgroups than CUs would run in passes, each
// pass as long as its longest game; it goes to the host loop, whose searches shrink as games retire.
bool DeviceSelfPlay::serves(uint32_t n_games, uint32_t iterations) {
    if (n_games == 0 || iterations > kRunMaxIters) return false;
    int cus = 0, lds = 0;
    search_.limits(cus, lds);
    return n_games / kBoardsPerGroup + (n_games % kBoardsPerGroup != 0) <= (uint32_t)cus;
}

// As DeviceSearch::reserve: a buffer that has to grow is freed first and its capacity cleared, so a failed allocation leaves the ctx consistent.
void DeviceSelfPlay::reserve(uint32_t n, uint32_t iterations, bool lds_tree) {
    const size_t head = sizeof(SpHead) + (size_t)kSpMaxSteps * iterations * 4;
    const size_t nodes = lds_tree ? 0 : (size_t)n * run_node_bound(iterations);
    if (n <= cap_n_ && head <= cap_head_ && nodes <= cap_nodes_) return;
    HIPCHK(hipStreamSynchronize(net_.stream()));
    if (n > cap_n_) {
        const size_t cap = grown(cap_n_, n, 1024);
        drop(d_frags_, false); drop(d_games_, false); drop(d_first_, false); drop(d_rec_, false); drop(h_rec_, true);
        cap_n_ = 0;
        HIPCHK(hipMalloc(&d_frags_, cap * kSpMaxSteps * sizeof(SpFrag)));
        HIPCHK(hipMalloc(&d_games_, cap * sizeof(SpGame)));
        HIPCHK(hipMalloc(&d_first_, cap * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&d_rec_, cap * kSpMaxSteps * kSpRowBytes));
        HIPCHK(hipHostMalloc(&h_rec_, cap * kSpMaxSteps * kSpRowBytes));
        cap_n_ = (uint32_t)cap;
    }
    if (head > cap_head_) {
        const size_t cap = grown(cap_head_, head, 4096);
        drop(d_head_, false); drop(h_head_, true);
        cap_head_ = 0;
        HIPCHK(hipMalloc(&d_head_, cap));
        HIPCHK(hipHostMalloc(&h_head_, cap));
        cap_head_ = cap;
    }
    if (nodes > cap_nodes_) {
        const size_t cap = grown(cap_nodes_, nodes, 1024 * 64);
        drop(d_nodes_, false);
        cap_nodes_ = 0;
        HIPCHK(hipMalloc(&d_nodes_, cap * sizeof(RunNode)));
        cap_nodes_ = cap;
    }
}

void DeviceSelfPlay::run(uint32_t n_games, uint32_t first_game_id, const diee_mcts_cfg& cfg, float temperature, uint64_t seed, uint32_t max_steps,
                         diee_fragments* out, diee_stats* stats) {
    if (!net_.ready()) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called");
    HIPCHK(hipSetDevice(net_.device()));
    int cus = 0, lds = 0;
    search_.limits(cus, lds);
    const bool lds_tree = cfg.iterations <= kRunLdsIters && lds >= 160 * 1024;
    try { reserve(n_games, cfg.iterations, lds_tree); } catch (...) { (void)hipGetLastError(); throw; }      // (a failed allocation is not the next launch's error)
    hipStream_t stream = net_.stream();

    SpParams P{};
    P.sp.net = net_.params();
    P.sp.nodes = (RunNode*)d_nodes_;
    P.sp.n = n_games; P.sp.iterations = cfg.iterations; P.sp.slab = run_node_bound(cfg.iterations); P.sp.quirks = 0u;
    P.sp.c = cfg.c; P.sp.eps = cfg.dir_eps; P.sp.one_minus_eps = 1.0f - cfg.dir_eps;
    P.head = (SpHead*)d_head_;
    P.any_selected = (uint32_t*)((unsigned char*)d_head_ + sizeof(SpHead));
    P.frags = (SpFrag*)d_frags_; P.games = (SpGame*)d_games_; P.first_row = (uint32_t*)d_first_; P.rec = (unsigned char*)d_rec_;
    P.seed = seed; P.first_game_id = first_game_id; P.round_limit = cfg.round_limit;
    P.steps = max_steps != 0 && max_steps < kSpMaxSteps ? max_steps : kSpMaxSteps;
    P.inv_t = (float)(1.0 / (double)temperature);                                              // :165 pow_(1.0 / temperature)
    for (uint32_t s = 0; s < P.steps; ++s) dirichlet_host(seed, s, cfg.dir_alpha, A, P.noise[s]);   // ONE sample per move-step for all its games

    const size_t head = sizeof(SpHead) + (size_t)P.steps * cfg.iterations * 4;
    HIPCHK(hipMemsetAsync(d_head_, 0, head, stream));
    HIPCHK(launch_ttt_selfplay(stream, P, lds_tree, lds_tree && !lds_asked_));
    lds_asked_ = lds_asked_ || lds_tree;
    HIPCHK(hipMemcpyAsync(h_head_, d_head_, head, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    search_.report_launches(1, 1);

    const SpHead* H = (const SpHead*)h_head_;
    const size_t nf = H->nf;
    if (nf > (size_t)n_games * kSpMaxSteps) throw EngineError(DIEE_ERR_CAPACITY,"search_fused = 2: more rows than games x 9");
    if (stats) {
        const uint32_t* flag = (const uint32_t*)((const unsigned char*)h_head_ + sizeof(SpHead));
        for (uint32_t s = 0; s < P.steps; ++s) {
            if (H->live[s] == 0u) continue;
            uint64_t evals = 1;                                                                // the roots, then one per iteration somebody selected in
            for (uint32_t k = 0; k < cfg.iterations; ++k) evals += flag[(size_t)s * cfg.iterations + k] != 0u;
            stats->nn_evals += evals * H->live[s];
            stats->move_steps += 1;
        }
        stats->nn_rows = stats->nn_evals;
        stats->expansions = H->counters[kCntExpansions]; stats->children = H->counters[kCntChildren]; stats->max_children = H->counters[kCntMaxChildren];
        stats->selections = H->counters[kCntSelections]; stats->depth_sum = H->counters[kCntDepthSum]; stats->terminal_hits = H->counters[kCntTerminalHits];
        stats->plies = H->counters[kSpPlies]; stats->games = H->counters[kSpGames]; stats->illegal_decodes = H->counters[kSpIllegal];
        stats->fragments = nf;
    }
    if (!out || nf == 0) return;
    HIPCHK(hipMemcpyAsync(h_rec_, d_rec_, nf * kSpRowBytes, hipMemcpyDeviceToHost, stream));       // exactly the rows delivered
    HIPCHK(hipStreamSynchronize(stream));
    out->outcome = (int8_t*)malloc(nf); out->ps = (float*)malloc(nf * A * sizeof(float));
    out->state = (float*)malloc(nf * PLANES * sizeof(float)); out->game = (uint32_t*)malloc(nf * sizeof(uint32_t));
    if (!out->outcome || !out->ps || !out->state || !out->game) { diee_free_fragments(out); throw std::bad_alloc(); }
    const unsigned char* h = (const unsigned char*)h_rec_;
    memcpy(out->state, h, nf * PLANES * 4); h += nf * PLANES * 4;
    memcpy(out->ps, h, nf * A * 4); h += nf * A * 4;
    memcpy(out->game, h, nf * 4); h += nf * 4;
    memcpy(out->outcome, h, nf);
    out->n = (uint32_t)nf;
}

}  // namespace ttt
}  // namespace diee
