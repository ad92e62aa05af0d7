// vanilla_host.h -- host side of Agent::Mcts (vanilla_kernels.hip): what diee_mcts_vanilla_batch and the arena share.
#pragma once
#include <stdint.h>

#include "engine.h"
#include "search_types.h"

namespace diee {

// iterations >= 2^20 or round_limit > 4094 do not fit the RNG counter (iteration << 12 | k): DIEE_ERR_ARG
void vanilla_check_cfg(const diee_mcts_cfg& cfg);
// buffers for n roots and cfg.iterations + 1 nodes each, the ln table, the launch budget -> the kernels' view.  The roots and their RNG
// keys are the caller's to fill (V.roots / V.game_id / V.round, device memory); `side` picks the counter block (the arena keeps one per player)
Vanilla vanilla_reserve(Engine& e, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t flags, uint32_t side = 0);
// the search: roots -> V.out_play (and the root's children where asked for; device pointers or null).  Enqueues, does not wait.
void vanilla_search(Engine& e, const Vanilla& V, uint32_t n, uint32_t* n_children = nullptr, float* child_visits = nullptr,
                    float* child_values = nullptr, uint32_t cap = 0);
void vanilla_zero_counters(Engine& e);
void free_vanilla(VanillaBufs* v);
void vanilla_read_counters(Engine& e, uint32_t side, diee_vanilla_stats* out);      // waits for the stream

}  // namespace diee
