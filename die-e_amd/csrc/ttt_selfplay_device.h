// ttt_selfplay_device.h -- tic-tac-toe self-play as ONE search-and-play launch (option "search_fused" = "2" of a tic-tac-toe ctx whose
// "search" is "device"): k_ttt_selfplay_run (ttt_selfplay_kernels.hip) carries a workgroup's 16 games from the empty board to their last
// move, k_ttt_sp_offsets and k_ttt_sp_gather deliver the records in the order of Engine::self_play's host loop (ttt_host.cpp), which stays
// the path of every call this one does not serve.  Without DIEE_FLAG_REF_QUIRKS the games of a call read nothing of one another.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/diee.h"
#include "ttt_device.h"
#include "ttt_host.h"
#include "ttt_search_device.h"

namespace diee {
namespace ttt {

constexpr uint32_t kSpMaxSteps = 9;                // a game ends within nine move-steps: check_winner reports the full board
constexpr uint32_t kSpNone = 0xFFFFFFFFu;          // SpGame::flush_step of a game that delivers nothing (alive when max_steps ended the call)
enum { kSpZero, kSpWinner };                       // SpGame::kind: the round-limit flush (outcomes 0) | the flush of a finished game

// What a game records at a move-step (alpha_parallel.rs:195-199): 160 bytes, words 0 .. 35 are the rows the gather copies.
struct SpFrag {
    float ps[A], planes[PLANES];
    int32_t player;
    uint32_t pad[3];
};
static_assert(sizeof(SpFrag) == 160, "16-byte multiples");
// What a game leaves for the delivery: its fragments 0 .. n_flushed - 1 go out at move-step flush_step.
struct SpGame {
    uint32_t flush_step, n_flushed, kind;
    int32_t winner;
};

// the search's counters (ttt_search_device.h), then the driver's
enum { kSpPlies = kCntCount, kSpGames, kSpIllegal, kSpCntCount };
// The small block: cleared in-stream before the launch, copied out as one, followed by any_selected [steps][iterations].
struct SpHead {
    unsigned long long counters[kSpCntCount];
    uint32_t nf;                                   // rows delivered (k_ttt_sp_offsets)
    uint32_t live[kSpMaxSteps];                    // games that were live in move-step s
};
static_assert(sizeof(SpHead) % 8 == 0, "");

struct SpParams {
    SearchParams sp;                               // net, n = n_games, iterations, slab, c, eps, one_minus_eps; nodes (RunNode [n][slab]) only if the tree is in HBM; quirks = 0
    SpHead* head;
    uint32_t* any_selected;                        // [steps][iterations]: word (s, k) is set by a workgroup that selected in iteration k of move-step s
    SpFrag* frags;                                 // [n][kSpMaxSteps]
    SpGame* games;                                 // [n]
    uint32_t* first_row;                           // [n]: a flushed game's first row of the output (k_ttt_sp_offsets)
    unsigned char* rec;                            // the output, nf rows: state f32 [nf][27] | ps f32 [nf][9] | game u32 [nf] | outcome i8 [nf]
    uint64_t seed;
    uint32_t first_game_id, steps, round_limit;
    float inv_t;
    float noise[kSpMaxSteps][A];                   // row s: the ONE Dirichlet sample of move-step s
};
constexpr size_t kSpRowBytes = (PLANES + A + 1) * 4 + 1;

// ttt_selfplay_kernels.hip.  `first`: no launch with the tree in LDS has been made on this device yet (as launch_ttt_search_run)
hipError_t launch_ttt_selfplay(hipStream_t st, const SpParams& P, bool lds_tree, bool first);

class DeviceSelfPlay {
public:
    DeviceSelfPlay(DeviceNet& net, DeviceSearch& search) : net_(net), search_(search) {}
    ~DeviceSelfPlay();
    DeviceSelfPlay(const DeviceSelfPlay&) = delete;
    DeviceSelfPlay& operator=(const DeviceSelfPlay&) = delete;
    // whether a call without the quirks is served: every workgroup has a CU of its own, a launch stays far below a second
    bool serves(uint32_t n_games, uint32_t iterations);
    // Engine::self_play for a call that serves() accepts; throws EngineError and leaves *out empty if a buffer cannot be had or a HIP call fails
    void run(uint32_t n_games, uint32_t first_game_id, const diee_mcts_cfg& cfg, float temperature, uint64_t seed, uint32_t max_steps, diee_fragments* out,
             diee_stats* stats);

private:
    void reserve(uint32_t n, uint32_t iterations, bool lds_tree);
    void release();
    DeviceNet& net_;
    DeviceSearch& search_;
    bool lds_asked_ = false;                       // k_ttt_selfplay_run's dynamic LDS has been asked for
    void *d_frags_ = nullptr, *d_games_ = nullptr, *d_first_ = nullptr, *d_rec_ = nullptr, *h_rec_ = nullptr;      // cap_n_ games
    void *d_head_ = nullptr, *h_head_ = nullptr;   // SpHead | any_selected: cap_head_ bytes
    void* d_nodes_ = nullptr;                      // cap_nodes_ RunNodes
    uint32_t cap_n_ = 0;
    size_t cap_head_ = 0, cap_nodes_ = 0;
};

}  // namespace ttt
}  // namespace diee
