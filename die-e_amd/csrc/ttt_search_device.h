// ttt_search_device.h -- the tic-tac-toe search on the device (option "search" = "device" of a tic-tac-toe ctx whose "nn" is "device"):
// alpha_mcts_parallel (ttt_host.cpp: search) as iterations + 1 launches of k_ttt_search (ttt_search_kernels.hip) enqueued back to back on
// the ctx's stream, one synchronise and one copy-out at the end.  The host reads nothing in between.  Option "search_fused" = "1" (opt-in)
// sends an eligible call to ONE launch of k_ttt_search_run (ttt_search_run_kernels.hip) instead: same output block, same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/diee.h"
#include "ttt_device.h"
#include "ttt_host.h"

namespace diee {
namespace ttt {

// A node of a game's tree, 16 bytes.  The children of a node are contiguous, first_child + j in ascending cell order like the host Store: a
// child's action and state follow from the parent's state (child j is the j-th empty cell) and the path of a descent is written down, so
// neither is stored.
struct RunNode {
    float visits, value, prior;
    uint32_t link;             // first_child | n_children << 20 | drained << 24
};
static_assert(sizeof(RunNode) == 16, "one 16-byte load per child");
constexpr uint32_t kRunDrained = 1u << 24;
// The most nodes a game's tree can hold after `iterations` iterations: a game's slab.  Level d of a tic-tac-toe tree has at most
// 9 * 8 * .. * (10 - d) nodes, each with at most 9 - d children; the root is expanded before the first iteration and an iteration expands at
// most one node.  The sum is largest when the expansions go to the shallowest levels first: 9 nodes of 8 children, 72 of 7, 504 of 6, ...
// (369 at 50.)  It stops at the whole game tree, so first_child fits the 20 bits of the link word whatever the iterations.
constexpr uint32_t run_node_bound(uint32_t iterations) {
    uint32_t nodes = 10, level = 9;
    for (uint32_t d = 1; d < 9 && iterations != 0; ++d) {
        const uint32_t e = iterations < level ? iterations : level;
        nodes += e * (9 - d); iterations -= e; level *= 9 - d;
    }
    return nodes;
}
static_assert(run_node_bound(0) == 10 && run_node_bound(9) == 82 && run_node_bound(50) == 369 && run_node_bound(0xFFFFFFFFu) == 986410, "");
static_assert(run_node_bound(0xFFFFFFFFu) < (1u << 20), "RunNode::link keeps first_child in 20 bits");
constexpr int kPathCap = 10;   // root + 9 plies

// What a game carries from launch to launch.
struct SearchGame {
    float policy[9], value;    // its last evaluation: the state of `sel` (launch 0: the root, Dirichlet noise mixed in)
    int32_t sel;               // alpha_mcts.rs:142 vec![0; n]: the last leaf this slot selected (stale while fresh == 0)
    uint32_t fresh;
    uint32_t n_nodes;
    uint32_t depth;            // of `sel`; path[0 .. depth] = root .. sel
    uint32_t sel_state;
    uint32_t expansions, children, max_children, selections, depth_sum, terminal_hits;     // diee_stats, this game's share
    uint32_t ever;             // 0 until this slot selects for the first time: till then `sel` names node 0 of the ONE NodeStore, game 0's root
    float root_value;          // the evaluation of the root's state (what a slot that never selected backpropagates under the quirks)
    uint32_t root_state;       // the packed word of ttt_rules_device.h
    int32_t path[kPathCap];
    uint32_t pad2[2];
};
static_assert(sizeof(SearchGame) == 144, "16-byte multiples");

enum { kCntExpansions, kCntChildren, kCntMaxChildren, kCntSelections, kCntDepthSum, kCntTerminalHits, kCntCount };

struct SearchParams {
    NetParams net;
    const diee_ttt_state* roots;
    RunNode* nodes;                    // [n][slab], slab = run_node_bound(iterations); unused by k_ttt_search_run with its tree in LDS
    SearchGame* games;                 // [n]
    uint32_t* any_selected;            // [iterations]: word k is set by launch k if any game selected a leaf that needs the network
    uint32_t* never_selected;          // [iterations]: word k counts the games other than game 0 that have not selected once up to launch k
    unsigned long long* counters;      // [kCntCount], written by the last launch
    float* probs;                      // [n][9]                "
    uint32_t* n_children;              // [n]                   "
    float* root_visits;                // [n]                   "
    uint32_t n, iterations, k, slab, quirks;
    float c, eps, one_minus_eps;
    float noise[9];                    // ONE Dirichlet sample for all roots (noise.rs:27-34)
};

// ttt_search_kernels.hip: launch k of 0 .. iterations; ceil(n / 16) workgroups, no workgroup waits for another
void launch_ttt_search(hipStream_t st, const SearchParams& P);

// ---- k_ttt_search_run: the whole search of a workgroup's 16 games in one launch ------------------------------------------------------------------
// The tree stays in LDS while the 16 games' bounds fit into what the network's 62400 bytes (NetLds) and the kernel's own 1280 leave of a
// CU's 160 KB; above that it lies in the HBM slab.  kRunLdsIters is the largest `iterations` of the LDS placement.
constexpr uint32_t kRunLdsBytes = 160 * 1024 - 62400 - 1280;
constexpr uint32_t run_lds_iters() {
    uint32_t it = 0;
    while (run_node_bound(it + 1) * 16 * sizeof(RunNode) <= kRunLdsBytes) ++it;
    return it;
}
constexpr uint32_t kRunLdsIters = run_lds_iters();
constexpr uint32_t kRunMaxIters = 4096;            // k_ttt_vanilla's bound: a launch stays far below a second
// ttt_search_run_kernels.hip: ceil(n / 16) workgroups; P.k is unused, P.nodes only if !lds_tree.  `first`: no launch with the tree in LDS
// has been made on this device yet (the dynamic LDS has to be asked for once).
hipError_t launch_ttt_search_run(hipStream_t st, const SearchParams& P, bool lds_tree, bool first);

// The buffers of the device search, owned by the ctx, grown by doubling; results of one call in page-locked memory.
class DeviceSearch {
public:
    explicit DeviceSearch(DeviceNet& net) : net_(net) {}
    ~DeviceSearch();
    DeviceSearch(const DeviceSearch&) = delete;
    DeviceSearch& operator=(const DeviceSearch&) = delete;
    // the whole search; throws EngineError and writes nothing to R or st if a buffer cannot be had or a HIP call fails
    void run(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step, bool quirks, diee_stats* st, RootResult& R);
    // What a search leaves on the device: pointers into d_out_, good until the next search is enqueued.
    struct Enqueued {
        const unsigned long long* counters;    // [kCntCount]
        const uint32_t* any_selected;          // [iterations]
        const float* probs;                    // [n][9]
        const uint32_t* n_children;            // [n]
        size_t head, bytes;                    // of d_out_: counters and flag words | all of it
    };
    // run() without its two ends: n >= 1 roots already on the device (cells of -1 / 0 / +1), launches 0 .. iterations enqueued on the ctx's
    // stream over `net` (this ctx's network, or another ctx's on the same device: read-only), nothing copied and nothing waited for.
    // The caller has reserved (n or more games, cfg.iterations) and set the device.
    Enqueued enqueue(const diee_ttt_state* d_roots, uint32_t n, const NetParams& net, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step, bool quirks);
    // `quirks`: whether any search to come runs under DIEE_FLAG_REF_QUIRKS (it decides which kernel a call goes to, and so what it needs)
    void reserve(uint32_t n, uint32_t iterations, bool quirks);
    // option "search_fused" (0, 1, or 2: as 1, and an eligible self-play call is one launch, ttt_selfplay_device.h) and what the read-only options report
    void set_fused(uint32_t level) { fused_ = level != 0; fused_level_ = level; }
    uint32_t fused_level() const { return fused_level_; }
    uint32_t last_launches() const { return last_launches_; }
    uint32_t self_play_launches() const { return self_play_launches_; }
    // what a self-play call has launched: its last search | all its searches
    void report_launches(uint32_t last, uint32_t self_play) { last_launches_ = last; self_play_launches_ = self_play; }
    // the device's CUs and the LDS a workgroup can have, asked once
    void limits(int& cus, int& lds_per_group);

private:
    enum class Path { PerIteration, RunLds, RunHbm };
    Path path(uint32_t n, uint32_t iterations, bool quirks);
    void release();
    bool fused_ = false;
    uint32_t fused_level_ = 0;
    uint32_t last_launches_ = 0;               // search-kernel launches of the last enqueue()
    uint32_t self_play_launches_ = 0;          // search-kernel launches of the last self-play call
    int cus_ = 0, lds_per_group_ = 0;          // of the device, asked once
    bool lds_asked_ = false;                   // k_ttt_search_run's dynamic LDS has been asked for
    DeviceNet& net_;
    void *d_roots_ = nullptr, *d_nodes_ = nullptr, *d_games_ = nullptr, *d_out_ = nullptr, *h_roots_ = nullptr, *h_out_ = nullptr;
    // d_out_ / h_out_: counters [kCntCount] u64 | any_selected [iterations] | never_selected [iterations] | probs [n][9] | n_children [n] | root_visits [n], copied out as one
    uint32_t cap_n_ = 0;                       // games of d_roots_, h_roots_, d_games_
    size_t cap_nodes_ = 0, cap_out_ = 0;       // nodes of d_nodes_, bytes of d_out_ and h_out_
};

}  // namespace ttt
}  // namespace diee
