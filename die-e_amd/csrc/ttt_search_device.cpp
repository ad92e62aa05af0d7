// ttt_search_device.cpp -- host side of the tic-tac-toe device search (ttt_search_device.h): buffers, the launch loop, the copy-out.
#include "ttt_search_device.h"

#include <cstring>
#include <string>

#include "engine.h"
#include "search_host.h"

namespace diee {
namespace ttt {

namespace {
// the capacity that holds `need`: doubling from `from`, `need` itself where doubling would overflow
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

DeviceSearch::~DeviceSearch() {
    if (hipSetDevice(net_.device()) != hipSuccess) return;
    (void)hipStreamSynchronize(net_.stream());
    release();
}

void DeviceSearch::release() {
    drop(d_roots_, false); drop(d_nodes_, false); drop(d_games_, false); drop(d_out_, false); drop(h_roots_, true); drop(h_out_, true);
    cap_n_ = 0; cap_nodes_ = 0; cap_out_ = 0;
}

// Which kernel a call goes to.  k_ttt_search_run serves a call whose games are independent or share one workgroup (quirks off, or n <= 16)
// up to kRunMaxIters iterations, while every workgroup has a CU of its own: the kernel's registers hold it to one workgroup per CU in
// either placement, k_ttt_search runs two, and measured (profiles/HISTORY.md, r18a) the one launch wins up to 4096 roots on 256 CUs and
// loses from 8192, where its workgroups take two passes.  Its tree is in LDS while a game's bound fits (faster than HBM at every size).
DeviceSearch::Path DeviceSearch::path(uint32_t n, uint32_t iterations, bool quirks) {
    if (!fused_ || (quirks && n > (uint32_t)kBoardsPerGroup) || iterations > kRunMaxIters) return Path::PerIteration;
    int cus, lds;
    limits(cus, lds);
    if (n / kBoardsPerGroup + (n % kBoardsPerGroup != 0) > (uint32_t)cus) return Path::PerIteration;
    return iterations <= kRunLdsIters && lds >= 160 * 1024 ? Path::RunLds : Path::RunHbm;
}

void DeviceSearch::limits(int& cus, int& lds_per_group) {
    if (cus_ == 0) {
        HIPCHK(hipDeviceGetAttribute(&lds_per_group_, hipDeviceAttributeMaxSharedMemoryPerBlock, net_.device()));
        HIPCHK(hipDeviceGetAttribute(&cus_, hipDeviceAttributeMultiprocessorCount, net_.device()));
    }
    cus = cus_; lds_per_group = lds_per_group_;
}

// A buffer that has to grow is freed first and its capacity cleared, so a failed allocation leaves the ctx consistent (the next call
// allocates again) and the error goes to the caller before anything has been launched.  d_nodes_ is reserved for the placement that needs
// it: k_ttt_search_run with its tree in LDS needs none.
void DeviceSearch::reserve(uint32_t n, uint32_t iterations, bool quirks) {
    if (iterations > (0x7FFFFFFFu - 10u) / 8u) throw EngineError(DIEE_ERR_CAPACITY, "option search = device: a game's nodes are indexed with 31 bits");
    const Path p = path(n, iterations, quirks);
    const size_t nodes = p == Path::RunLds ? 0 : (size_t)n * run_node_bound(iterations);
    const size_t out = kCntCount * sizeof(unsigned long long) + (2 * (size_t)iterations + (size_t)n * (A + 2)) * 4;
    if (n <= cap_n_ && nodes <= cap_nodes_ && out <= cap_out_) return;
    HIPCHK(hipStreamSynchronize(net_.stream()));
    if (n > cap_n_) {
        const size_t cap = grown(cap_n_, n, 1024);
        drop(d_roots_, false); drop(d_games_, false); drop(h_roots_, true);
        cap_n_ = 0;
        HIPCHK(hipMalloc(&d_roots_, cap * sizeof(diee_ttt_state)));
        HIPCHK(hipMalloc(&d_games_, cap * sizeof(SearchGame)));
        HIPCHK(hipHostMalloc(&h_roots_, cap * sizeof(diee_ttt_state)));
        cap_n_ = (uint32_t)(cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : cap);
    }
    if (nodes > cap_nodes_) {
        const size_t cap = grown(cap_nodes_, nodes, 1024 * 64);
        drop(d_nodes_, false);
        cap_nodes_ = 0;
        HIPCHK(hipMalloc(&d_nodes_, cap * sizeof(RunNode)));
        cap_nodes_ = cap;
    }
    if (out > cap_out_) {
        const size_t cap = grown(cap_out_, out, 64 * 1024);
        drop(d_out_, false); drop(h_out_, true);
        cap_out_ = 0;
        HIPCHK(hipMalloc(&d_out_, cap));
        HIPCHK(hipHostMalloc(&h_out_, cap));
        cap_out_ = cap;
    }
}

void DeviceSearch::run(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step, bool quirks, diee_stats* st,
                       RootResult& R) {
    R.probs.clear(); R.n_children.clear(); R.root_visits.clear();
    if (n == 0) return;
    if (!net_.ready()) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called");
    // a node keeps its board at 2 bits per cell and its player in one: what the rules produce from any legal position
    for (uint32_t i = 0; i < n; ++i) {
        bool ok = roots[i].player == 1 || roots[i].player == -1;
        for (int cidx = 0; cidx < 9; ++cidx) ok = ok && roots[i].board[cidx] >= -1 && roots[i].board[cidx] <= 1;
        if (!ok) throw EngineError(DIEE_ERR_ARG, "option search = device: root " + std::to_string(i) + " has a cell or a player outside -1 / 0 / +1");
    }
    HIPCHK(hipSetDevice(net_.device()));
    try { reserve(n, cfg.iterations, quirks); } catch (...) { (void)hipGetLastError(); throw; }      // (a failed allocation is not the next launch's error)
    hipStream_t stream = net_.stream();

    memcpy(h_roots_, roots, (size_t)n * sizeof(diee_ttt_state));
    HIPCHK(hipMemcpyAsync(d_roots_, h_roots_, (size_t)n * sizeof(diee_ttt_state), hipMemcpyHostToDevice, stream));
    const Enqueued E = enqueue((const diee_ttt_state*)d_roots_, n, net_.params(), cfg, seed, step, quirks);
    HIPCHK(hipMemcpyAsync(h_out_, d_out_, E.bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));

    const unsigned char* h = (const unsigned char*)h_out_;
    const float* probs = (const float*)(h + E.head);
    const uint32_t* nch = (const uint32_t*)(probs + (size_t)n * A);
    const float* rv = (const float*)(nch + n);
    R.probs.assign(probs, probs + (size_t)n * A);
    R.n_children.assign(nch, nch + n);
    R.root_visits.assign(rv, rv + n);
    if (st) {
        const unsigned long long* cnt = (const unsigned long long*)h;
        const uint32_t* flag = (const uint32_t*)(h + kCntCount * sizeof(unsigned long long));
        uint64_t evals = 1;                                                                      // the roots, then one per iteration somebody selected in
        for (uint32_t k = 0; k < cfg.iterations; ++k) evals += flag[k] != 0u;
        st->nn_evals += evals * n;
        st->expansions += cnt[kCntExpansions]; st->children += cnt[kCntChildren];
        if (cnt[kCntMaxChildren] > st->max_children) st->max_children = cnt[kCntMaxChildren];
        st->selections += cnt[kCntSelections]; st->depth_sum += cnt[kCntDepthSum]; st->terminal_hits += cnt[kCntTerminalHits];
    }
}

DeviceSearch::Enqueued DeviceSearch::enqueue(const diee_ttt_state* d_roots, uint32_t n, const NetParams& net, const diee_mcts_cfg& cfg, uint64_t seed,
                                             uint32_t step, bool quirks) {
    hipStream_t stream = net_.stream();

    SearchParams P{};
    P.net = net;
    P.roots = d_roots;
    P.nodes = (RunNode*)d_nodes_;
    P.games = (SearchGame*)d_games_;
    unsigned char* o = (unsigned char*)d_out_;
    const size_t head = kCntCount * sizeof(unsigned long long) + 2 * (size_t)cfg.iterations * 4;     // counters and per-iteration words: cleared in-stream
    P.counters = (unsigned long long*)o;
    P.any_selected = (uint32_t*)(o + kCntCount * sizeof(unsigned long long));
    P.never_selected = P.any_selected + cfg.iterations;
    P.probs = (float*)(o + head);
    P.n_children = (uint32_t*)(P.probs + (size_t)n * A);
    P.root_visits = (float*)(P.n_children + n);
    P.n = n; P.iterations = cfg.iterations; P.slab = run_node_bound(cfg.iterations); P.quirks = quirks ? 1u : 0u;
    P.c = cfg.c; P.eps = cfg.dir_eps; P.one_minus_eps = 1.0f - cfg.dir_eps;
    dirichlet_host(seed, step, cfg.dir_alpha, A, P.noise);                                       // apply_dirichlet, noise.rs:27-34: ONE sample for all rows

    const Path p = path(n, cfg.iterations, quirks);
    if ((p == Path::RunLds ? 0 : (size_t)n * P.slab) > cap_nodes_) throw EngineError(DIEE_ERR_CAPACITY, "option search = device: the search was not reserved for");
    HIPCHK(hipMemsetAsync(d_out_, 0, head, stream));
    if (p == Path::PerIteration) {
        for (uint32_t k = 0; k <= cfg.iterations; ++k) {
            P.k = k;
            launch_ttt_search(stream, P);
            HIPCHK(hipGetLastError());
        }
        last_launches_ = cfg.iterations + 1;
    } else {
        HIPCHK(launch_ttt_search_run(stream, P, p == Path::RunLds, p == Path::RunLds && !lds_asked_));
        lds_asked_ = lds_asked_ || p == Path::RunLds;
        last_launches_ = 1;
    }
    return Enqueued{P.counters, P.any_selected, P.probs, P.n_children, head, head + (size_t)n * (A + 2) * 4};
}

}  // namespace ttt
}  // namespace diee
