// search_types.h -- kernel parameter blocks (plain device pointers) shared by mcts_kernels.hip, selfplay_kernels.hip and
// the host drivers.  Layout in HBM:
//   Tree   : one fixed-stride arena per live-game slot (slot*node_cap + local index); node statistics
//            are SoA so that a wave reading the children of a node issues coalesced 4-byte loads;
//            children of a node are contiguous (first_child, n_children).
//   Slots  : per-slot search state of one move-step (slot = index into the live list).
//   Games  : per-game state of the self-play batches in flight (game = index over all batches, batch-major).
//   Segs   : the self-play batches ("segments") that share the slot space.  A batch is one call of the reference's
//            self_play_parallel: its games are coupled through the shared Dirichlet draw of a move-step, the
//            `node_selected` flag of an iteration and the stale-slot quirk (Q14), and through nothing else -- so K
//            batches can run side by side in ONE slot space (live games of batch 0, then of batch 1, ...) and share
//            every network launch, each with its own seed, flags and slot-0 bookkeeping.
#pragma once
#include <stdint.h>

#include "bg_device.h"

namespace diee {

enum Counter {
    CNT_NN_EVALS = 0, CNT_EXPANSIONS, CNT_CHILDREN, CNT_TERMINAL, CNT_DEPTH_SUM, CNT_SELECTIONS,
    CNT_ILLEGAL, CNT_MAX_CHILDREN, CNT_PLIES, CNT_GAMES, CNT_NN_ROWS, CNT_COUNT
};
constexpr uint32_t kMaxSegments = 64;

enum SlotCounter { SC_SELECTIONS = 0, SC_DEPTH_SUM, SC_TERMINAL, SC_EXPANSIONS, SC_CHILDREN, SC_MAX_CHILDREN, SC_ILLEGAL, SC_NN_ROWS, SC_COUNT };

struct Tree {
    float* visits;          // Node.visits  (f32 like the reference, node.rs:14)
    float* value;           // Node.value
    float* prior;           // Node.policy
    uint32_t* parent;       // local index, 0xFFFFFFFF = None
    uint32_t* first_child;  // local index of the first child
    uint32_t* meta;         // bit31 expanded ("expandable_moves drained"), bit30 / bit29 finished game / won by +1, bits28..16 n_children, bits15..0 action code
    BgState* state;         // Node.state (dice frozen at creation)
    uint32_t* used;         // [slots] bump allocator
    uint32_t node_cap;      // nodes per slot
};

struct Segs {
    const unsigned long long* seed;   // [segs] engine seed of the batch (keys dice, sampling, Dirichlet)
    const uint32_t* first_id;         // [segs] RNG key of the batch's game 0 (first_game_id)
    const uint32_t* game0;            // [segs] index of the batch's game 0 in the Games arrays
    uint32_t* first_slot;             // [segs] first live slot of the batch this move-step ...
    uint32_t* end_slot;               // [segs] ... and one past its last (both 0: no live game)
    uint32_t n;                       // batches in flight
    uint32_t iter_cap;                // iterations per batch in Slots::iter_flags
};

struct Slots {
    BgState* roots;         // [slots]
    BgState* eval_states;   // [slots] states evaluated by the ResNet this iteration (stale rows keep their content)
    uint32_t* game_id;      // [slots] RNG key
    uint32_t* round;        // [slots] RNG key
    uint32_t* seg;          // [slots] batch the slot's game belongs to
    uint32_t* leaf;         // [slots] selected leaf this iteration
    uint32_t* sel;          // [slots] selected_nodes_idxs (persists over iterations; 0xFFFFFFFF = initial)
    float* sel_value;       // [slots] NN value of sel
    uint8_t* leaf_term;     // [slots] leaf was terminal this iteration
    const uint32_t* slot_row;   // [slots] row of the slot's evaluation in the network outputs when the batch was compacted
                                // (k_row_map: slots with a terminal leaf get no row); null = row == slot
    const float* logits;    // [slots][1352] policy logits of this iteration's evaluation (nn_host's buffers)
    const float* hv;        // [slots][72] value features
    const float* wv;        // [73] value FC
    float* noise;           // [segs][1352] Dirichlet sample of this move-step, one per batch (noise.rs:27-34); slot refill (noise_segs != 0):
                            // [move-step][segs][1352], a root reads the row of its own game's round
    float* root_value0;     // [segs] NN value of the root in the batch's first slot
    uint32_t* iter_flags;   // [segs][iter_cap][2] any_selected, stale-initial count per iteration
    unsigned long long* counters;  // [segs][CNT_COUNT] totals (written by k_reduce_counters / single lanes only)
    uint32_t* slot_cnt;     // [slots][SC_COUNT] per-slot counters of this move-step: same-address atomics from a
                            // thousand waves serialise at ~11 ns each, per-slot words cost nothing
    uint32_t* overflow;     // capacity flag (bit0 sequence table, bit1 tree arena)
    uint32_t* leaf_meta;    // [slots] Tree::meta of leaf as the selection read it (nobody else writes this game's tree)
    uint32_t* path;         // [slots][kPathCap] nodes from the root to sel (entry d = depth d): backpropagation without the parent walk
    uint8_t* path_len;      // [slots] entries of path; 0 = deeper than path_cap (or no selection yet): walk the parents
    uint32_t* grow_k;       // [slots] children the growth workgroups of a tower launch created for the slot's leaf this iteration (0xFFFFFFFF: none to create / no room)
    uint16_t* grow_code;    // [slots][kMaxPlays] their action codes, child lane + 64 q at [lane * 4 + q]
    uint32_t path_cap;      // depths recorded (<= kPathCap = 64; option path_cap lowers it so that tests reach the parent walk)
    uint32_t noise_segs;    // 0: every live game of a batch is in the batch's current move-step (noise[seg]); n > 0: slot refill, n batches, the
                            // games of a batch are in different rounds and a game admitted late needs the sample of ITS round: noise[round * n + seg]
};
constexpr int kPathCap = 64;

struct Games {
    BgState* state;         // [games]
    uint32_t* rounds;       // n_rounds
    uint32_t* nfrags;
    uint8_t* alive;
    int8_t* winner;
    uint32_t* ev_a_count;   // round-limit flush: fragments flushed with outcome 0 (0xFFFFFFFF = none)
    uint32_t* ev_a_step;
    uint32_t* ev_b_count;   // win flush
    uint32_t* ev_b_step;
    uint32_t* live;         // [games] live list (ascending game index, hence batch-major)
    uint8_t* seg;           // [games] batch of the game
    float* frag_ps;         // [record areas][frag_cap][1352]
    float* frag_planes;     // [record areas][frag_cap][144]
    int8_t* frag_player;    // [record areas][frag_cap]
    uint32_t frag_cap;
    unsigned long long* counters;
    uint32_t* area;         // [games] record area of the game's fragments; null: the identity (one area per game of the call).  Slot refill
                            // keeps as many areas as games are in flight and hands a retired game's area to the game that takes its slot
};

// Output delivery of one move-step (alpha_parallel.rs:172-180, :215-223: a game's memory joins all_memories, relabelled, in
// the step the game is removed).  k_deliver_scan lists this step's flushes in the reference's order -- by game, round-limit
// flush before win flush, inside each batch -- with the row each starts at in its batch's output of the step; k_deliver_copy
// gathers a range of those rows (ps, planes, outcome, game id) into a staging buffer, which the host copies out on a second
// stream while the next move-step searches.
struct DeliverEvent { uint32_t g, kind_count, row0, seg; };   // kind_count = kind << 31 | rows; row0 = first row in the step's output of the batch
struct DeliverSummary {     // indices into the per-step summary the host reads with the live counts ([1 + 4 * segs] words)
    static constexpr uint32_t kLive = 0;                      // [0] games alive, [1 + b] alive in batch b   (k_compact_live)
    static __host__ __device__ uint32_t rows(uint32_t segs, uint32_t b) { return 1 + segs + b; }       // rows batch b delivers this step
    static __host__ __device__ uint32_t ev0(uint32_t segs, uint32_t b) { return 1 + 2 * segs + b; }    // its first event
    static __host__ __device__ uint32_t nev(uint32_t segs, uint32_t b) { return 1 + 3 * segs + b; }    // its events
};
struct DeliverOut { float* ps; float* planes; int8_t* outcome; uint32_t* game; };    // staging, row-major

// ---- the tail of a batch: speculative leaf evaluation (round 5) -----------------------------------------------------------------
// At <= 32 live games a network evaluation costs the same ~95 us whether its launch carries 1 or 32 boards (one cluster-tower
// launch, k_tower_cl<1, 8>; 125 us up to 64, 172 us up to 128 boards), and a search iteration is one such launch + the tree kernel:
// 147 of a batch's 364 move-steps are played with <= 32 live games, a serial chain of ~100 launches each.  But every leaf a search selects exists -- state, frozen dice -- from the moment its parent was
// expanded, and below 129 boards a row's network output is a pure function of its state (the split-K cluster family is one
// arithmetic, rows batch-independent: tests/test_nn_gpu.py).  So a launch's free rows carry unexpanded nodes the search is likely to
// select next (found by a virtual descent of the same PUCT rule on a scratch copy of the tree's statistics: "UCB selection staged in
// LDS"), every evaluated row stays in a ring of [launch][row] outputs, and an iteration whose selected leaves were all evaluated
// earlier needs NO launch: k_tail (mcts_kernels.hip) runs the iterations of all live games in lockstep, one after the other inside
// one launch, for as long as every selected leaf is in the ring, and plans the next launch's rows when one is not.  The search
// itself -- selection, expansion, backpropagation, the quirks' coupling of the games of a batch -- is the same code on the same
// numbers in the same order (expand_body): results are bit-identical to the launch-per-iteration path.  It ships for <= 16 live games: the free-running search below takes 17 ... 800.
// What rides in a launch beside the demanded leaves: every game's share of candidates (virtual descents), the candidates beyond the shares
// where rows are scarce (extra_rows: they take what other games leave free), and the children of a demanded leaf (child_rows: the one
// parent whose expanding iteration -- the key of its children's dice -- is known before it is expanded).
constexpr uint32_t kTailMaxSlots = 256;   // live games (all batches of the call) up to which a move-step's search may run this way: one workgroup per CU
                                          // (options spec_max_games <= 128 on the cluster family's launches, spec_fused_games for 129 ... 256 on the fused family's)
constexpr int kTailFusedRows = 512;      // rows of a tail launch at 129 ... 256 live games: the 4-board pair tower + k_policy_fc (the fused family, like those games' plain evaluations)
constexpr uint32_t kTailRowsMax = 128;    // rows of a tail launch at most: 32 (k_tower_cl<1, 8>, ~95 us), 64 (<2, 8>, ~125 us) or 128 (<4, 8>, ~172 us) -- one
                                          // arithmetic, so a row's bits do not depend on which of them evaluated it; the more games share a launch,
                                          // the more rows it carries (Tail::rows, search_host.cpp tail_rows_for)
constexpr uint32_t kTailLdsNodes = 3072;  // nodes of a game's tree whose statistics the virtual descent stages in LDS (beyond: read in place, not updated)
struct Tail {
    uint32_t* crow;         // [kTailMaxSlots][node_cap] ring row + 1 of a node's evaluation (0: none yet)
    float* cval;            // [kTailMaxSlots][node_cap] its value (for the virtual descents only: expansions recompute it from the row)
    BgState* rows_state;    // [launches][rows] states the tower launch q evaluates
    uint32_t* rows_node;    // [launches][rows] slot << 24 | node
    float* logits;          // [launches][rows][1352] the ring
    float* hv;              // [launches][rows][72]
    uint32_t* n_rows;       // [launches] rows of launch q (0: nothing to evaluate, the launch returns at once)
    uint32_t* n_dem;        // [launches] ... of which demanded (the games whose selected leaf had no evaluation): the bench's accounting
    uint32_t* state;        // [0] next iteration, [1] done, [2] launches that carried rows, [3] rows evaluated on speculation
    uint32_t* bar;          // [2 * launches + 8] one word per meeting of the games' workgroups (zeroed per move-step)
    uint32_t* bar2;         // [launches] the meeting inside the plan of launch q (extra_rows: shares taken before the free rows left over are)
    uint32_t* host;         // pinned host words: [0] next iteration, [1] done, [2] index of the last k_tail launch that finished
    uint32_t launches;      // iterations + 1
    uint32_t iterations;
    uint32_t rollout_steps; // virtual descents per game and launch at most
    uint32_t rows;          // rows of a launch in this move-step (32 / 64 / 128; 512 at 129 ... 256 live games)
    uint32_t child_rows;    // children of a demanded leaf (created ahead: their dice are keyed by the iteration that will expand it) that ride in its launch at most (0: off)
    uint32_t extra_rows;    // candidates a game may find beyond its share of a full launch's rows: they take what other games left free (0: off)
    uint32_t test_skip;     // tests: 1 + the meeting word at which the last game's workgroup does NOT arrive (0: never): every workgroup's bounded
                            // spin runs out, the starved bit is raised, the host repeats the move-step's search launch by launch
};

// ---- free-running search (round 6): 17 ... 800 live games (k_tail keeps <= 16) ---------------------------------------------------------------------------
// Above the tail's reach every MCTS iteration used to cost one network launch sized by the live games -- 300 us for <= 512 boards,
// ~480 ... 520 us for 513 ... 928, 577 us for a full pass of the chip: the rows of a part-empty launch cost up to twice a full one's.  The
// reference couples the games of a call only through `node_selected` (alpha_mcts.rs:151,170) and the stale slots (:142,192-200), so
// every game keeps its OWN iteration counter: a round = one launch of up to `rows` rows (the fused family, rows gathered from the tree
// arena by index: launch_tower_compact) + k_free, where each game takes in its rows, runs iterations for as long as its selected leaf is
// a finished game or has its evaluation (and the flags it needs are final), then lists its wishes -- the leaf it waits for, then the
// unexpanded nodes its virtual PUCT descents end on -- and k_free_pack grants them: every demanded leaf, then the wishes rank by rank
// until the launch is full.  No workgroup ever waits for another one inside a launch (a game that needs a flag another game has not
// published yet simply stops for this round), so nothing has to be co-resident.  Priced before it was built: tests/tools/free_price.*,
// profiles/r06a_*.  Results are bit-identical to the lockstep search: the same operations on the same numbers in the same order per game.
constexpr uint32_t kFreeWish = 24;        // wishes a game may list per round (demanded leaf included)
constexpr uint32_t kFreeMaxSlots = 1024;  // k_free_pack: one thread per game
constexpr uint32_t kFreeBoostMax = 16;
struct Free {
    uint32_t* crow;         // [slots][node_cap] 1 + launch * rows + row of a node's evaluation (0: none); valid while launch + ring > the current launch
    float* cval;            // [slots][node_cap] its value (virtual descents only)
    uint32_t* rows_idx;     // [ring][rows] arena index (slot * node_cap + node) of every row of a launch: the tower gathers its states through it
    BgState* rows_state;    // [ring][rows] the rows' states, dense: what the cluster tower of a launch of at most 128 rows reads (null above: gathered by index)
    float* logits;          // [ring][rows][1352]
    float* hv;              // [ring][rows][72]
    uint32_t* n_rows;       // [launches] rows of launch q
    uint32_t* n_dem;        // [launches] ... of which demanded (a game's selected leaf waiting for its evaluation): the bench's accounting
    uint32_t* grant_off;    // [slots] first row of the slot in the launch planned last ...
    uint32_t* grant_cnt;    // [slots] ... and how many it got
    uint32_t* wish;         // [slots][kFreeWish] nodes, most wanted first
    uint32_t* wish_n;       // [slots] count | 0x80000000 when wish[0] is the demanded leaf | progress << 8 (the packer may favour games behind)
    uint32_t* prog;         // [slots] the iteration whose selection the game has published = its own iteration counter
    uint32_t* first_sel;    // [slots] iteration of the game's first real selection (0xFFFFFFFF: none yet): Q14's count matters only before it
    uint32_t* state;        // [0] all games done, [1] launches that carried rows, [2] rows evaluated on speculation, [4] games not done when the last round was
                            // packed (k_free sizes its budgets by them: the last games of a search have the launches to themselves)
    uint32_t* host;         // pinned: [0] done, [1] last k_free_pack that finished
    uint32_t launches;      // rounds the host sends at most: 4 x (iterations + games) + 66 (search_host.cpp free_launches_for)
    uint32_t iterations;
    uint32_t rows;          // rows of a launch at most (512: pair tower; 1024: one pass of the chip)
    uint32_t ring;          // launches whose rows stay in the ring
    uint32_t lds_nodes;     // nodes of a game's tree staged in LDS (by the workgroups that share a CU)
    uint32_t rollout_steps; // virtual descents per game and round at most
    uint32_t cand_max;      // candidates a game lists at most (< kFreeWish)
    uint32_t lag_boost, lag_step;   // k_free_pack: a game lag_step iterations behind the leader is served one rank earlier, up to lag_boost ranks (<= kFreeBoostMax)
    uint32_t iter_cap;      // iterations a game runs in one launch at most: the launch lasts as long as its busiest game (a game whose leaves are
                            // finished games needs no rows and would run its whole search in the first one)
};

struct SearchParams {
    float dir_eps;
    uint32_t quirks;
};

struct PlayParams {
    uint32_t round_limit;
    float inv_temperature;
    uint32_t quirks;
};

// ---- the arena (diee_arena; versus.rs:160-318) ----------------------------------------------------------------------------------
// Model-vs-model games of one call, all on the device: per round k_arena_split partitions the live games by side to move (stable,
// ascending game index), each side's list is searched in the call's slot space (k_arena_gather -> mcts_run) and its moves are
// played (k_arena_move) before the other side searches: both sides' trees share the slots, and a game is in one list only.
enum ArenaWord {            // Arena::words
    AW_COUNT0 = 0,          // games in player 1's list this round, [1] player 2's, [2] games alive (k_arena_split; what the host reads)
    AW_LIVE = 2,
    AW_WINS1 = 3, AW_WINS2, AW_DRAWS,
    AW_TURNS0 = 6,          // turns player 1 took (skipped ones included), [7] player 2
    AW_MOVES0 = 8,          // ... of which a move was applied, [9] player 2
    AW_RETIRED0 = 10,       // games retired by a move of player 1, [11] player 2
    AW_COUNT = 12
};
struct Arena {
    BgState* state;         // [games]
    BgState* initial;       // [games] the states the games started from
    uint8_t* alive;         // [games]
    int8_t* winner;         // [games] -1 player 1, +1 player 2, 0 none
    uint32_t* retired_round;// [games] round in which the game was retired (0xFFFFFFFF: still alive)
    int8_t* retired_side;   // [games] list it moved in when it was retired (-1: still alive)
    uint32_t* live;         // [games] live list, ascending game index
    uint32_t* list;         // [2][games] this round's lists of the two sides
    uint32_t* words;        // [AW_COUNT]
    uint32_t n_games;
};
// The turn log (diee_arena_ex; Turn, versus.rs:21-26): one record per turn, the layout of diee_turn (include/diee.h).  k_arena_split puts
// every live game into exactly one side's list, so a live game takes exactly one turn per round and its turn index IS the call's round:
// the log is round-major rows of n_games records, game g's turn of round r at row r, record g.  The host allocates the rows in chunks
// as the rounds go by and hands k_arena_move the row of its round; the records of games that are not alive are never written.
struct ArenaTurn {
    int8_t play[4];         // all kNoMove: a skipped turn
    uint8_t roll[2];        // the state's roll before the move
    uint8_t next_roll[2];   // the dice apply_move / skip_turn was given
    int8_t player;          // the state's side to move, -1 / +1
    uint8_t agent;          // DIEE_AGENT_* of the player that moved
    uint8_t second;         // is_second_play before the move
    uint8_t retired;        // the turn retired the game
};
static_assert(sizeof(ArenaTurn) == 12, "diee_turn is 12 bytes");
struct ArenaParams {
    unsigned long long seed;
    uint32_t round, round_limit;
    float inv_temperature;
    uint32_t side;          // 0: player 1's list, 1: player 2's
    uint32_t agent;         // DIEE_AGENT_RANDOM / DIEE_AGENT_MODEL / DIEE_AGENT_MCTS of that player
    ArenaTurn* log;         // [n_games] this round's row of the turn log; null: no log
};

// ---- Agent::Mcts (diee_mcts_vanilla_batch; simple_mcts.rs:10-39, node.rs) ---------------------------------------------------------
// Vanilla UCB1 search with random rollouts, one wavefront per game (vanilla_kernels.hip).  A game's tree is a slab of node_cap =
// iterations + 1 nodes in HBM (an iteration creates at most one node) that persists from launch to launch: a launch runs at most
// `budget` iterations per game, the host launches ceil(iterations / budget) times, and since an iteration reads nothing but the slab
// and the game's own words the result does not depend on the budget.  A node's children are created iterations apart, so they are not
// contiguous: they hang on a list (head = the newest, `next` = the sibling created before it); creation order = ascending node index.
enum VanillaCounter { VC_ITERATIONS = 0, VC_EXPANSIONS, VC_TERMINAL, VC_DEAD_END, VC_ROLLOUTS, VC_PLIES, VC_DECIDED, VC_DEPTH_SUM, VC_COUNT };
constexpr uint32_t kVanillaUnknown = 0xFFFFFFFFu;   // Vanilla::nplays of a node whose plays have not been enumerated yet; the end of a list
struct Vanilla {
    BgState* state;         // [slots][node_cap] Node.state (dice frozen at creation)
    uint32_t* parent;       // [slots][node_cap] local index (the root: kVanillaUnknown)
    uint32_t* nplays;       // [slots][node_cap] legal plays of the node's state = Node.expandable_moves.len() + children.len()
    uint32_t* ncreated;     // [slots][node_cap] children created so far
    uint32_t* visits;       // [slots][node_cap] Node.visits (integers; the reference's f32 counts them exactly)
    float* value;           // [slots][node_cap] Node.value
    uint32_t* play;         // [slots][node_cap] the play that led here (bytes f1, t1, f2, t2)
    uint32_t* head;         // [slots][node_cap] the child created last (kVanillaUnknown: none)
    uint32_t* next;         // [slots][node_cap] the sibling created before this node
    uint32_t* done;         // [slots] iterations the game has run; kVanillaUnknown: it runs none (finished root, root without a play, capacity)
    uint32_t* used;         // [slots] nodes of the slab in use
    BgState* roots;         // [slots] (the caller fills the roots and their RNG keys)
    uint32_t* game_id;      // [slots] RNG key
    uint32_t* round;        // [slots] RNG key
    const float* ln;        // [iterations + 2] ln[k] = (float)log((double)k), built by the host (ln[0] is never read)
    unsigned long long* counters;   // [slots][VC_COUNT] running totals of the slot (the host sums them)
    uint32_t* out_play;     // [slots] the answer: the root's most visited child's play, or EMPTY_MOVE
    uint32_t* overflow;     // capacity flag (bit0: more than kMaxPlays legal plays / the sequence table)
    unsigned long long seed;
    uint32_t node_cap, iterations, round_limit, budget, quirks;
    float c;
};

}  // namespace diee
