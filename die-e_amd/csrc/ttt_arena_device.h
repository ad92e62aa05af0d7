// ttt_arena_device.h -- the tic-tac-toe arena on the device (diee_ttt_arena while option "search" of the hosting ctx is "device"): play::<TicTacToe>
// (versus.rs:160-268; ttt_host.cpp: Engine::arena is the host statement of the same rules) with every round on the hosting ctx's stream.
// A round is k_ttt_arena_split, then per side with games to move { its search, enqueued on roots the split left on the device;
// k_ttt_arena_move<agent> }.  The host reads three page-locked words per round and one block when the call ends.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/diee.h"
#include "ttt_search_device.h"
#include "ttt_vanilla_device.h"

namespace diee {
namespace ttt {

constexpr uint32_t kArenaNone = 0xFFFFFFFFu;       // retired_round of a game still alive

// the call's totals, 64-bit words: one block per player, then the call's own
enum { kTaPlies, kTaMoves, kTaRetired, kTaNnEvals, kTaExpansions, kTaChildren, kTaMaxChildren, kTaSelections, kTaDepthSum, kTaTerminal,
       kTaPlayerWords };
enum { kTaWins1 = 2 * kTaPlayerWords, kTaWins2, kTaDraws, kTaOverflow, kTaWords };

// The games of one call in HBM.  `out` is one block, copied out once: totals | state | retired_round | winner | retired_side.
struct ArenaGames {
    unsigned long long* totals;        // [kTaWords]
    uint32_t* state;                   // [n_games]: the packed word of ttt_rules_device.h
    uint32_t* retired_round;           // [n_games]: kArenaNone while the game is alive
    int8_t* winner;                    // [n_games]
    int8_t* retired_side;              // [n_games]
    uint32_t* counts;                  // [3]: side 0's list, side 1's list, the games alive (k_ttt_arena_move keeps that one)
    uint32_t* live;                    // [n_games]: the live games in ascending index, compacted by every split
    uint32_t* keys;                    // [2][n_games][2]: a side's list as (game id, round) pairs, the keys k_ttt_vanilla reads
    diee_ttt_state* roots;             // [2][n_games]: the states of a side's list
    uint32_t n_games;
};

// what k_ttt_arena_move needs of the turn it finishes
struct ArenaMove {
    unsigned long long seed;
    uint32_t n, side, round, round_limit, iterations;
    float inv_t;
    const float* probs;                // Model: the search's rows [n][9] ...
    const uint32_t* n_children;        // ... [n] ...
    const unsigned long long* counters;    // ... its counters [kCntCount] ...
    const uint32_t* any_selected;      // ... and its [iterations] flag words, all still on the device
    const VanillaOut* vout;            // Mcts: the search's answers [n]
};

// ttt_arena_kernels.hip; no workgroup waits for another
void launch_ttt_arena_init(hipStream_t st, const ArenaGames& G);
void launch_ttt_arena_split(hipStream_t st, const ArenaGames& G, uint32_t n_live, uint32_t round);
void launch_ttt_arena_move(hipStream_t st, const ArenaGames& G, const ArenaMove& M, int agent);

struct ArenaArgs {
    int agents[2];
    const NetParams* nets[2];          // a Model player's network (player 2's may be another ctx's: read-only)
    uint32_t n_games;
    diee_mcts_cfg cfg;
    float temperature;
    uint64_t seed;
    uint32_t round_limit, max_rounds, flags[2];
};

// The buffers of the device arena, owned by the hosting ctx next to its two device searches, whose streams and buffers the call uses.
class DeviceArena {
public:
    DeviceArena(DeviceNet& net, DeviceSearch& search, DeviceVanilla& vanilla) : net_(net), search_(search), vanilla_(vanilla) {}
    ~DeviceArena();
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    // the whole call; outputs as diee_ttt_arena's (each may be null).  Throws EngineError before any output is written.
    void run(const ArenaArgs& a, diee_arena_result* res, int8_t* winner, uint32_t* retired_round, int8_t* retired_side, diee_ttt_state* final_states,
             diee_stats* stats);

private:
    void reserve(uint32_t n);
    void release();
    DeviceNet& net_;
    DeviceSearch& search_;
    DeviceVanilla& vanilla_;
    void *d_out_ = nullptr, *h_out_ = nullptr, *d_work_ = nullptr, *h_counts_ = nullptr;      // d_out_: ArenaGames' one block; d_work_: roots | keys | live | counts
    uint32_t cap_ = 0;
};

}  // namespace ttt
}  // namespace diee
