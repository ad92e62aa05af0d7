// ttt_arena_device.h -- the tic-tac-toe arena on the device (diee_ttt_arena while option "search" of the hosting ctx is "device"): play::<TicTacToe>
// (versus.rs:160-268; ttt_host.cpp: Engine::arena is the host statement of the same rules) with every round on the hosting ctx's stream.
// A round is k_ttt_arena_split, then per side with games to move { its search, enqueued on roots the split left on the device;
// k_ttt_arena_move<agent> }.  The host reads three page-locked words per round and one block when the call ends.
// With option "search_fused" = "2" on the hosting ctx a call of Model and Random players without DIEE_FLAG_REF_QUIRKS is ONE launch of
// k_ttt_arena_run (ttt_arena_run_kernels.hip) instead: same outputs, same bits; the round loop stays the path of every other call.
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

// ---- k_ttt_arena_run: a whole call in one launch (ttt_arena_run_kernels.hip; option "search_fused" = "2" of the hosting ctx) ------------------
constexpr uint32_t kArRounds = 9;                  // a game without skipped turns ends within nine rounds: the rounds one launch plays
// The small block: cleared in-stream before the launch, followed by any_selected [2 * rounds][iterations], then the per-game block of
// ArenaGames (state | retired_round | winner | retired_side); all of it is copied out as one.
struct ArHead {
    unsigned long long totals[kTaWords];
    uint32_t live[2 * kArRounds];                  // games of side s live in step 2 * round + s
    uint32_t alive;                                // games still alive after the last round played
    uint32_t pad;
};
static_assert(sizeof(ArHead) % 8 == 0, "");

struct ArParams {
    SearchParams sp;                               // n = n_games, iterations, slab, c, eps, one_minus_eps; nodes (RunNode [n][slab]) only if the tree is in HBM; quirks = 0; net: unused
    NetParams nets[2];                             // a Model side's network
    int agents[2];                                 // DIEE_AGENT_MODEL or DIEE_AGENT_RANDOM
    ArHead* head;
    uint32_t* any_selected;                        // [2 * rounds][iterations]: word (step, k) is set by a workgroup that selected in iteration k of that step
    uint32_t* state;                               // [n] ...
    uint32_t* retired_round;                       // ... [n] ...
    int8_t* winner;                                // ... [n] ...
    int8_t* retired_side;                          // ... [n]: as ArenaGames'
    unsigned long long seed;
    uint32_t rounds, round_limit;
    float inv_t;
    float noise[2 * kArRounds][A];                 // row 2 * round + side: the ONE Dirichlet sample of that search
};
// The two halves of a call (the first n / 2 games start with side 0 to move, the others with side 1) are mapped separately, so a
// workgroup's games are all on one side in any round.
constexpr uint32_t arena_run_groups(uint32_t n_games) {
    const uint32_t h = n_games / 2, b = (uint32_t)kBoardsPerGroup;
    return (h + b - 1) / b + (n_games - h + b - 1) / b;
}
// `first`: no launch with the tree in LDS has been made on this device yet (as launch_ttt_search_run)
hipError_t launch_ttt_arena_run(hipStream_t st, const ArParams& P, bool lds_tree, bool first);

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
    // Whether the call is one launch of k_ttt_arena_run: "search_fused" = "2", Model and Random players only, no quirks on a Model side
    // (without them the games read nothing of one another), every workgroup with a CU of its own, a launch far below a second.
    bool serves(const ArenaArgs& a);
    // run() for a call that serves() accepts.  Returns false, with no output written, if a game was still alive after kArRounds rounds
    // (skipped turns) and the caller allowed more: the call is a function of its arguments, so run() then plays the whole of it.
    bool run_one_launch(const ArenaArgs& a, diee_arena_result* res, int8_t* winner, uint32_t* retired_round, int8_t* retired_side,
                        diee_ttt_state* final_states, diee_stats* stats);
    // option "arena_last_launches": the search-kernel launches of the last call
    uint32_t last_launches() const { return last_launches_; }

private:
    void reserve(uint32_t n);
    void reserve_run(size_t bytes, size_t nodes);
    void release();
    void decode(const ArenaArgs& a, const unsigned long long* tot, const uint32_t* state, const uint64_t move_steps[2], uint32_t rounds, double secs,
                diee_arena_result* res, int8_t* winner, uint32_t* retired_round, int8_t* retired_side, diee_ttt_state* final_states, diee_stats* stats);
    uint32_t last_launches_ = 0;
    bool lds_asked_ = false;                       // k_ttt_arena_run's dynamic LDS has been asked for
    void *d_run_ = nullptr, *h_run_ = nullptr, *d_nodes_ = nullptr;       // k_ttt_arena_run's one block (ArHead | any_selected | the games) and its HBM trees
    size_t cap_run_ = 0, cap_nodes_ = 0;           // bytes of d_run_ and h_run_, RunNodes of d_nodes_
    DeviceNet& net_;
    DeviceSearch& search_;
    DeviceVanilla& vanilla_;
    void *d_out_ = nullptr, *h_out_ = nullptr, *d_work_ = nullptr, *h_counts_ = nullptr;      // d_out_: ArenaGames' one block; d_work_: roots | keys | live | counts
    uint32_t cap_ = 0;
};

}  // namespace ttt
}  // namespace diee
