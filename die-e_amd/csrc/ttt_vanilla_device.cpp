// ttt_vanilla_device.cpp -- host side of the tic-tac-toe device vanilla search (ttt_vanilla_device.h): buffers, the ln table, the launch
// loop, the copy-out.
#include "ttt_vanilla_device.h"

#include <cmath>
#include <cstring>
#include <vector>

#include "engine.h"

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

DeviceVanilla::~DeviceVanilla() {
    if (hipSetDevice(net_.device()) != hipSuccess) return;
    (void)hipStreamSynchronize(net_.stream());
    release();
}

void DeviceVanilla::release() {
    drop(d_in_, false); drop(h_in_, true); drop(d_games_, false); drop(d_out_, false); drop(h_out_, true); drop(d_nodes_, false); drop(d_ln_, false);
    cap_n_ = 0; cap_ln_ = 0; ln_n_ = 0; cap_words_ = 0;
}

// A buffer that has to grow is freed first and its capacity cleared, so a failed allocation leaves the ctx consistent (the next call
// allocates again) and the error goes to the caller before anything has been launched.
void DeviceVanilla::reserve(uint32_t n, size_t node_words, uint32_t ln_n) {
    if (n <= cap_n_ && node_words <= cap_words_ && ln_n <= ln_n_) return;
    HIPCHK(hipStreamSynchronize(net_.stream()));
    if (n > cap_n_) {
        const size_t cap = grown(cap_n_, n, 1024);
        drop(d_in_, false); drop(h_in_, true); drop(d_games_, false); drop(d_out_, false); drop(h_out_, true);
        cap_n_ = 0;
        const size_t in = cap * (sizeof(diee_ttt_state) + 2 * sizeof(uint32_t));
        HIPCHK(hipMalloc(&d_in_, in));
        HIPCHK(hipHostMalloc(&h_in_, in));
        HIPCHK(hipMalloc(&d_games_, cap * sizeof(VanillaGame)));
        HIPCHK(hipMalloc(&d_out_, cap * sizeof(VanillaOut)));
        HIPCHK(hipHostMalloc(&h_out_, cap * sizeof(VanillaOut)));
        cap_n_ = (uint32_t)(cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : cap);
    }
    if (node_words > cap_words_) {
        const size_t cap = grown(cap_words_, node_words, (size_t)1 << 20);
        drop(d_nodes_, false);
        cap_words_ = 0;
        HIPCHK(hipMalloc(&d_nodes_, cap * sizeof(uint32_t)));
        cap_words_ = cap;
    }
    if (ln_n > ln_n_) {                                          // ln is not reproducible between libm and the device: one table, built here
        if (ln_n > cap_ln_) {
            const size_t cap = grown(cap_ln_, ln_n, 4096);
            drop(d_ln_, false);
            cap_ln_ = 0; ln_n_ = 0;
            HIPCHK(hipMalloc(&d_ln_, cap * sizeof(float)));
            cap_ln_ = (uint32_t)cap;
        }
        std::vector<float> ln(ln_n, 0.0f);
        for (uint32_t k = 1; k < ln_n; ++k) ln[k] = (float)std::log((double)k);
        HIPCHK(hipMemcpy(d_ln_, ln.data(), ln.size() * sizeof(float), hipMemcpyHostToDevice));      // synchronous: the vector is stack-scoped
        ln_n_ = ln_n;
    }
}

const VanillaOut* DeviceVanilla::run(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, const uint32_t* game_ids,
                                     const uint32_t* rounds, bool quirks) {
    if (n == 0) return nullptr;
    HIPCHK(hipSetDevice(net_.device()));
    reserve_for(n, cfg);
    hipStream_t stream = net_.stream();

    diee_ttt_state* h_roots = (diee_ttt_state*)h_in_;
    uint32_t* h_keys = (uint32_t*)(h_roots + n);
    memcpy(h_roots, roots, (size_t)n * sizeof(diee_ttt_state));
    for (uint32_t i = 0; i < n; ++i) { h_keys[2 * i] = game_ids ? game_ids[i] : i; h_keys[2 * i + 1] = rounds ? rounds[i] : 0u; }
    const size_t in = (size_t)n * (sizeof(diee_ttt_state) + 2 * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(d_in_, h_in_, in, hipMemcpyHostToDevice, stream));
    const diee_ttt_state* d_roots = (const diee_ttt_state*)d_in_;
    (void)enqueue(d_roots, (const uint32_t*)(d_roots + n), n, cfg, seed, quirks);
    HIPCHK(hipMemcpyAsync(h_out_, d_out_, (size_t)n * sizeof(VanillaOut), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const VanillaOut* out = (const VanillaOut*)h_out_;
    for (uint32_t i = 0; i < n; ++i)
        if (out[i].overflow) throw EngineError(DIEE_ERR_CAPACITY, "k_ttt_vanilla: a game's slab is full");
    return out;
}

namespace {
uint32_t slab_of(const diee_mcts_cfg& cfg) { return cfg.iterations + 1 < kVanillaMaxNodes ? cfg.iterations + 1 : kVanillaMaxNodes; }
}  // namespace

void DeviceVanilla::reserve_for(uint32_t n, const diee_mcts_cfg& cfg) {
    const uint32_t slab = slab_of(cfg);
    try { reserve(n, slab <= kVanillaLdsNodes ? 0 : (size_t)n * slab * kVNodeWords, cfg.iterations + 2); } catch (...) { (void)hipGetLastError(); throw; }
}

const VanillaOut* DeviceVanilla::enqueue(const diee_ttt_state* d_roots, const uint32_t* d_keys, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed,
                                         bool quirks) {
    const uint32_t slab = slab_of(cfg);
    const bool lds = slab <= kVanillaLdsNodes;
    hipStream_t stream = net_.stream();

    VanillaParams P{};
    P.roots = d_roots;
    P.keys = d_keys;
    P.ln = (const float*)d_ln_;
    P.nodes = lds ? nullptr : (uint32_t*)d_nodes_;
    P.games = (VanillaGame*)d_games_;
    P.out = (VanillaOut*)d_out_;
    P.seed = seed;
    P.n = n; P.iterations = cfg.iterations; P.slab = slab; P.round_limit = cfg.round_limit; P.quirks = quirks ? 1u : 0u;
    P.c = cfg.c;
    // every game runs exactly cfg.iterations iterations (or none): the number of launches is known, nothing is read back in between.
    // iterations == 0 is one launch too: it builds the roots and answers.
    uint32_t it = 0;
    do {
        P.it0 = it;
        P.it1 = cfg.iterations - it > kVanillaItersPerLaunch ? it + kVanillaItersPerLaunch : cfg.iterations;
        launch_ttt_vanilla(stream, P);
        HIPCHK(hipGetLastError());
        it = P.it1;
    } while (it < cfg.iterations);
    return (const VanillaOut*)d_out_;
}

}  // namespace ttt
}  // namespace diee
