// ttt_vanilla_device.h -- Agent::Mcts for tic-tac-toe on the device (diee_ttt_mcts_vanilla_batch while option "search" of the ctx is "device"):
// mct_search (ttt_host.cpp: vanilla_search_host) as launches of k_ttt_vanilla (ttt_vanilla_kernels.hip), each running up to
// kVanillaItersPerLaunch whole iterations per game, enqueued back to back on the ctx's stream; one synchronise and one copy-out per call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/diee.h"
#include "ttt_device.h"

namespace diee {
namespace ttt {

// One node, 12 words: visits | value (f32 bits) | meta | the indices of its children in creation order.  meta = the packed board of
// ttt_search_device.h (2 bits per cell: 0 empty, 1 = +1, 3 = -1; bit 18 = the player to move is +1) | children created << 20.  A node keeps
// no parent: the path root .. leaf is held in the row's lanes during a descent.  child[j] is written when child j is created and read for
// j < children created only, so a slab is never cleared.
constexpr int kVNodeWords = 12;
constexpr uint32_t kVStateMask = 0x7FFFFu;
constexpr int kVCreatedShift = 20;
// sum over k of 9! / (9 - k)!: every sequence of distinct cells.  No tree from one root has more nodes, whatever `iterations` says.
constexpr uint32_t kVanillaMaxNodes = 986410u;
// The tree lives in LDS when the whole search is one launch and a game needs at most this many nodes (16 games x 64 nodes x 48 bytes = 48 KB
// of the workgroup); otherwise in HBM, [n][slab] nodes, where it also carries over from launch to launch.
constexpr uint32_t kVanillaLdsNodes = 64;
// Iterations a game runs in one launch at most.  One launch at this bound over 1024 empty-board roots with round_limit 400 and the
// rollouts played takes tens of milliseconds (profiles/HISTORY.md), far below a second; the results do not depend on it.
constexpr uint32_t kVanillaItersPerLaunch = 4096;
static_assert(kVanillaLdsNodes - 1 <= kVanillaItersPerLaunch, "a search whose tree is in LDS is one launch: LDS does not outlive it");

enum { kVcIterations, kVcExpansions, kVcTerminal, kVcRollouts, kVcPlies, kVcDecided, kVcDepthSum, kVcCount };

// What a game carries from launch to launch (HBM placement only).
struct VanillaGame {
    uint32_t used;                     // nodes of its slab in use
    uint32_t cnt[kVcCount];            // diee_vanilla_stats, this game's share
};
static_assert(sizeof(VanillaGame) == 32, "two 16-byte words");

// What the last launch leaves per game, copied out as one block.
struct VanillaOut {
    uint32_t move;                     // 0 .. 8, or 10 = EMPTY_MOVE
    uint32_t n_children;
    uint32_t overflow;                 // never set by a slab of min(iterations + 1, kVanillaMaxNodes) nodes: DIEE_ERR_CAPACITY if it is
    uint32_t pad;
    float child_visits[9], child_values[9];
    uint32_t cnt[kVcCount];
    uint32_t pad2[3];
};
static_assert(sizeof(VanillaOut) == 128, "16-byte multiples");

struct VanillaParams {
    const diee_ttt_state* roots;       // [n]
    const uint32_t* keys;              // [n][2]: game id, round
    const float* ln;                   // [iterations + 2]: ln[k] = (float)log((double)k), built on the host
    uint32_t* nodes;                   // [n][slab][kVNodeWords]; null: the LDS placement
    VanillaGame* games;                // [n]
    VanillaOut* out;                   // [n], written by the launch whose it1 == iterations
    unsigned long long seed;
    uint32_t n, iterations, it0, it1;  // this launch runs iterations it0 .. it1 - 1 of every game; it0 == 0 builds the roots
    uint32_t slab, round_limit, quirks;
    float c;
};

// ttt_vanilla_kernels.hip: ceil(n / 16) workgroups of 256, a game per row of 16 lanes, no workgroup waits for another
void launch_ttt_vanilla(hipStream_t st, const VanillaParams& P);

// The buffers of the device vanilla search, owned by the ctx, grown by doubling; roots, keys and results in page-locked memory.
class DeviceVanilla {
public:
    explicit DeviceVanilla(DeviceNet& net) : net_(net) {}
    ~DeviceVanilla();
    DeviceVanilla(const DeviceVanilla&) = delete;
    DeviceVanilla& operator=(const DeviceVanilla&) = delete;
    // the whole search of validated roots; out[n] points into page-locked memory that the next call reuses.  Throws EngineError before
    // anything is written if a buffer cannot be had or a HIP call fails.
    const VanillaOut* run(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, const uint32_t* game_ids,
                          const uint32_t* rounds, bool quirks);
    // run() without its two ends: n >= 1 roots and their keys [n][2] already on the device, the launches enqueued on the ctx's stream, nothing
    // copied and nothing waited for.  -> the answers [n] on the device, good until the next search is enqueued (`overflow` is the reader's to
    // check).  The caller has called reserve_for (n or more games, the same cfg) and set the device.
    const VanillaOut* enqueue(const diee_ttt_state* d_roots, const uint32_t* d_keys, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, bool quirks);
    void reserve_for(uint32_t n, const diee_mcts_cfg& cfg);

private:
    void reserve(uint32_t n, size_t node_words, uint32_t ln_n);
    void release();
    DeviceNet& net_;                   // the ctx's device and its one stream; the network itself is not used
    void *d_in_ = nullptr, *h_in_ = nullptr, *d_games_ = nullptr, *d_out_ = nullptr, *h_out_ = nullptr, *d_nodes_ = nullptr, *d_ln_ = nullptr;
    // d_in_ / h_in_: roots [cap_n_] | keys [cap_n_][2], copied in as one
    uint32_t cap_n_ = 0, cap_ln_ = 0, ln_n_ = 0;       // ln_n_: entries of d_ln_ that are filled
    size_t cap_words_ = 0;
};

}  // namespace ttt
}  // namespace diee
