// ttt_search_device.h -- the tic-tac-toe search on the device (option "search" = "device" of a tic-tac-toe ctx whose "nn" is "device"):
// alpha_mcts_parallel (ttt_host.cpp: search) as iterations + 1 launches of k_ttt_search (ttt_search_kernels.hip) enqueued back to back on
// the ctx's stream, one synchronise and one copy-out at the end.  The host reads nothing in between.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/diee.h"
#include "ttt_device.h"
#include "ttt_host.h"

namespace diee {
namespace ttt {

// One node, 32 bytes.  A game's nodes are a slab of 10 + 8 * iterations of them (the root, at most 9 root children, at most one expansion
// of at most 8 children per iteration); the children of a node are contiguous, first_child + j in ascending cell order, like the host Store.
struct SearchNode {
    float visits, value, prior;
    uint32_t state;            // 2 bits per cell (0 empty, 1 = +1, 3 = -1) in bits 0 .. 17, bit 18 = the player to move is +1
    int32_t parent, first_child;
    uint32_t meta;             // n_children | action << 8 | drained << 16
    uint32_t pad;
};
static_assert(sizeof(SearchNode) == 32, "two 16-byte loads per child");
constexpr uint32_t kMetaDrained = 1u << 16;
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
    uint32_t pad;
    int32_t path[kPathCap];
    uint32_t pad2[2];
};
static_assert(sizeof(SearchGame) == 144, "16-byte multiples");

enum { kCntExpansions, kCntChildren, kCntMaxChildren, kCntSelections, kCntDepthSum, kCntTerminalHits, kCntCount };

struct SearchParams {
    NetParams net;
    const diee_ttt_state* roots;
    SearchNode* nodes;                 // [n][slab]
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
    void reserve(uint32_t n, uint32_t iterations);

private:
    void release();
    DeviceNet& net_;
    void *d_roots_ = nullptr, *d_nodes_ = nullptr, *d_games_ = nullptr, *d_out_ = nullptr, *h_roots_ = nullptr, *h_out_ = nullptr;
    // d_out_ / h_out_: counters [kCntCount] u64 | any_selected [iterations] | never_selected [iterations] | probs [n][9] | n_children [n] | root_visits [n], copied out as one
    uint32_t cap_n_ = 0;                       // games of d_roots_, h_roots_, d_games_
    size_t cap_nodes_ = 0, cap_out_ = 0;       // nodes of d_nodes_, bytes of d_out_ and h_out_
};

}  // namespace ttt
}  // namespace diee
