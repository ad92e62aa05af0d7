// ttt_host.h -- tic-tac-toe behind the same C ABI (BASELINE.json configs[0]: "Tic-Tac-Toe, 1 self-play game,
// iterations=50, random-init net, CPU reference path (plumbing, no GPU)").
//
// The reference drives tic-tac-toe through the very functions it drives backgammon through (learn_parallel /
// self_play_parallel / alpha_mcts_parallel are generic over LearnableGame, src/main.rs:119-124), on the CPU: a 3x3
// board, 9 actions, a 64-filter 4-block ResNet of 2.85 M MAC per evaluation.  That is host work by definition of the
// config -- there is nothing for 256 CUs to do -- so this path is plain C++ on the host: rules (src/tictactoe/mod.rs:
// 28-100), the fp32 ResNet (src/alphazero/nnet.rs:24-34,57-133 with N_FILTERS = 64, N_RES_BLOCKS = 4, mod.rs:20-24),
// the batched search (src/mcts/alpha_mcts.rs:91-202) and the self-play driver (src/alphazero/alpha_parallel.rs:101-231).
// It is reached only through diee_create(.., DIEE_GAME_TTT, ..); the backgammon path has no host fallback.
// At the reference's batch sizes (1024 games per search) the network IS work for the chip: option "nn" = "device" (opt-in) sends
// forward() to one launch of k_ttt_net (ttt_device.h); rules, search and driver stay here.  Over that, option "search" = "device" (opt-in
// too) runs the batched search as one launch of k_ttt_search per iteration (ttt_search_device.h); the driver stays here.
// Agent::Mcts (mcts_vanilla_batch, no network) follows option "search" too: here by default, k_ttt_vanilla (ttt_vanilla_device.h) on "device".
// So does the arena that plays those searches against each other (arena): a round loop here, every round on the device (ttt_arena_device.h) on "device".
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/diee.h"

namespace diee {
namespace ttt {

constexpr int A = 9, PLANES = 27, F = 64, BLOCKS = 4, CIN = 3, HW = 9, PH = 32, VH = 3;

// LearnableGame for TicTacToe, src/tictactoe/mod.rs
int valid_moves(const diee_ttt_state& s, uint8_t out[9]);        // :36-44
void apply_move(diee_ttt_state& s, uint8_t a);                    // :46-49
void skip_turn(diee_ttt_state& s);                                // :51-53
bool check_winner(const diee_ttt_state& s, int& winner);          // :60-81 (winner 0 = draw)
void planes(const diee_ttt_state& s, float out[27]);              // :83-94

size_t weights_count();
void random_weights(uint64_t seed, float* blob);

struct Conv { std::vector<float> w, b; int cout = 0, cin = 0; };          // OIHW, BatchNorm folded (eval mode, eps 1e-5)
class DeviceNet;                                                          // ttt_device.h
class DeviceSearch;                                                       // ttt_search_device.h
class DeviceVanilla;                                                      // ttt_vanilla_device.h
class DeviceArena;                                                        // ttt_arena_device.h
class DeviceSelfPlay;                                                     // ttt_selfplay_device.h

// what a search leaves for its callers: get_prob_tensor_parallel's rows (utils.rs:42-58) and the roots' counts
struct RootResult {
    std::vector<float> probs;                                             // [n][9]; a childless root: NaN
    std::vector<uint32_t> n_children;                                     // [n]
    std::vector<float> root_visits;                                       // [n]
};

class Engine {
public:
    explicit Engine(int device = 0);                                      // `device`: the GPU option "nn" = "device" would use; not touched before
    ~Engine();
    // option "nn" (include/diee.h): "host" (default) = the fp32 loops below, "device" = k_ttt_net (ttt_device.h) behind forward().
    // A failed switch to "device" (no usable GPU: DIEE_ERR_HIP) leaves the ctx on the host path.
    // option "search": "host" (default) = both searches below on the host, "device" = k_ttt_search (ttt_search_device.h) behind mcts_batch
    // and every move-step of self_play, and k_ttt_vanilla (ttt_vanilla_device.h) behind mcts_vanilla_batch.  "device" needs "nn" = "device" (else DIEE_ERR_ARG), and "nn" cannot go back to "host" before "search" has.
    // option "search_fused": "0" (default) | "1" = an eligible device search is ONE launch of k_ttt_search_run (ttt_search_device.h); "1" needs
    // "search" = "device" (else DIEE_ERR_ARG) and "search" = "host" resets it.  "2" = "1", and a self_play call without the quirks whose
    // workgroups have a CU each is ONE launch of k_ttt_selfplay_run plus the delivery (ttt_selfplay_device.h), and an arena call of
    // Model and Random players without the quirks is ONE launch of k_ttt_arena_run (ttt_arena_device.h).  Read-only: "search_last_launches",
    // "self_play_last_launches" (the search launches of the last self_play), "arena_last_launches" (of the last arena), "search_fused_lds_iters".
    // Every other key: DIEE_ERR_UNSUPPORTED.
    void set_option(const std::string& key, const std::string& value);
    std::string get_option(const std::string& key) const;
    void load_weights(const float* blob, size_t n);
    bool loaded() const { return !w_.empty(); }
    // ResNet::forward_t (nnet.rs:120-133), eval mode: softmax policy [n][9], tanh value [n].  `const` as the searches below call it; on
    // the host path it is re-entrant, on the device path it is NOT: it goes through the ctx's one stream and staging buffers (one call
    // at a time per ctx, like every entry point of a backgammon ctx) and leaves the calling thread's current HIP device set to the ctx's.
    void forward(const diee_ttt_state* s, uint32_t n, float* policy, float* value) const;
    void mcts_batch(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step,
                    const uint32_t* game_ids, const uint32_t* rounds, uint32_t flags, float* visit_probs, uint32_t* n_children,
                    float* root_visits, diee_stats* stats) const;
    void self_play(uint32_t n_games, uint32_t first_game_id, const diee_mcts_cfg& cfg, float temperature, uint64_t seed,
                   uint32_t flags, uint32_t max_steps, diee_fragments* out, diee_stats* stats) const;
    // mct_search (simple_mcts.rs:10-39) per root, Agent::Mcts: diee_ttt_mcts_vanilla_batch of include/diee.h.  Needs no weights.
    void mcts_vanilla_batch(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, const uint32_t* game_ids,
                            const uint32_t* rounds, uint32_t flags, uint8_t* moves, uint32_t* n_children, float* child_visits,
                            float* child_values, diee_vanilla_stats* stats) const;
    // play::<TicTacToe> (versus.rs:160-318): diee_ttt_arena of include/diee.h, called on the hosting ctx (e1, or e2 when e1 is null).  Option
    // "search" of the hosting ctx names the path: "host" = the round loop of ttt_host.cpp over each player's own searches, "device" = every round
    // on this ctx's stream, or the whole call in one launch under "search_fused" = "2" (ttt_arena_device.h).
    void arena(const Engine* e1, int agent1, const Engine* e2, int agent2, uint32_t n_games, const diee_mcts_cfg& cfg, float temperature, uint64_t seed,
               uint32_t round_limit, uint32_t max_rounds, const uint32_t flags[2], diee_arena_result* res, int8_t* winner, uint32_t* retired_round,
               int8_t* retired_side, diee_ttt_state* final_states, diee_stats* stats) const;

private:
    void upload() const;                                                    // the folded weights -> dev_
    // alpha_mcts_parallel (alpha_mcts.rs:91-202) on the path option "search" names; statistics are added to *st
    void search(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step, bool quirks, diee_stats* st,
                RootResult& R) const;
    int device_;
    std::unique_ptr<DeviceNet> dev_;                                        // non-null = "nn" is "device"
    std::unique_ptr<DeviceSearch> dsearch_;                                 // non-null = "search" is "device" (dev_ is non-null then; declared after it: destroyed first)
    std::unique_ptr<DeviceVanilla> dvanilla_;                               // set and cleared with dsearch_
    std::unique_ptr<DeviceArena> darena_;                                   // set and cleared with dsearch_; it drives the two above (destroyed before them)
    std::unique_ptr<DeviceSelfPlay> dselfplay_;                             // set and cleared with dsearch_, whose device limits and launch counts it uses (destroyed before it)
    Conv init_, c1_[BLOCKS], c2_[BLOCKS], pconv_, vconv_;
    std::vector<float> pfc_w_, pfc_b_, vfc_w_, vfc_b_;
    std::vector<float> w_;                                                  // the blob as loaded (non-empty = loaded)
};

}  // namespace ttt
}  // namespace diee
