// ttt_host.cpp -- tic-tac-toe on the host behind the C ABI (see ttt_host.h for why this game is host work).
// Reference: src/tictactoe/mod.rs:28-100 (rules), src/alphazero/nnet.rs:24-34,57-133 (ResNet, 64 filters x 4 blocks),
// src/mcts/alpha_mcts.rs:14-33,91-202 + node.rs:98-112,157-174 + simple_mcts.rs:96-103 + utils.rs:42-84 + noise.rs:27-34
// (batched search), src/alphazero/alpha_parallel.rs:101-231 + alphazero.rs:129-137 (self-play driver).
// RNG conventions are the engine's (Philox keyed by seed / game / round / purpose, bg_device.h), so that a record of this
// path can be checked against the test oracle exactly like the HIP path's.
#include "ttt_host.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "bg_device.h"
#include "engine.h"
#include "search_host.h"
#include "ttt_arena_device.h"
#include "ttt_device.h"
#include "ttt_search_device.h"
#include "ttt_selfplay_device.h"
#include "ttt_vanilla_device.h"
#include "vanilla_host.h"

namespace diee {
namespace ttt {

// ---- rules -----------------------------------------------------------------------------------------------------------
int valid_moves(const diee_ttt_state& s, uint8_t out[9]) {
    int k = 0;
    for (int i = 0; i < 9; ++i) if (s.board[i] == 0) out[k++] = (uint8_t)i;
    return k;
}
void apply_move(diee_ttt_state& s, uint8_t a) { s.board[a] = s.player; s.player = (int8_t)-s.player; }
void skip_turn(diee_ttt_state& s) { s.player = (int8_t)-s.player; }
bool check_winner(const diee_ttt_state& s, int& winner) {
    static const int L[8][3] = {{0, 1, 2}, {3, 4, 5}, {6, 7, 8}, {0, 3, 6}, {1, 4, 7}, {2, 5, 8}, {0, 4, 8}, {2, 4, 6}};
    for (const auto& l : L) {
        const int a = s.board[l[0]];
        if (a != 0 && a == s.board[l[1]] && a == s.board[l[2]]) { winner = a; return true; }
    }
    for (int i = 0; i < 9; ++i) if (s.board[i] == 0) return false;
    winner = 0;                                                         // a full board without a line: draw, Some(0)
    return true;
}
void planes(const diee_ttt_state& s, float out[27]) {                   // stack([eq(-1), eq(0), eq(1)])
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 9; ++i) out[c * 9 + i] = s.board[i] == c - 1 ? 1.0f : 0.0f;
}

// ---- weights: the blob layout of include/diee.h with this game's sizes ------------------------------------------------
namespace {
struct Cursor {
    size_t off = 0;
    size_t take(size_t n) { const size_t o = off; off += n; return o; }
};
struct Layout {
    size_t init_w, init_b, init_bn, c1w[BLOCKS], c1b[BLOCKS], c2w[BLOCKS], c2b[BLOCKS], bn1[BLOCKS], bn2[BLOCKS];
    size_t pw, pb, pbn, pfw, pfb, vw, vb, vbn, vfw, vfb, total;
};
Layout make_layout() {
    Layout L; Cursor c;
    L.init_w = c.take((size_t)F * CIN * 9); L.init_b = c.take(F); L.init_bn = c.take(4 * F);
    for (int i = 0; i < BLOCKS; ++i) {                                   // ResBlock::new creation order, nnet.rs:38-45
        L.c1w[i] = c.take((size_t)F * F * 9); L.c1b[i] = c.take(F); L.c2w[i] = c.take((size_t)F * F * 9); L.c2b[i] = c.take(F);
        L.bn1[i] = c.take(4 * F); L.bn2[i] = c.take(4 * F);
    }
    L.pw = c.take((size_t)PH * F * 9); L.pb = c.take(PH); L.pbn = c.take(4 * PH); L.pfw = c.take((size_t)A * PH * HW); L.pfb = c.take(A);
    L.vw = c.take((size_t)VH * F * 9); L.vb = c.take(VH); L.vbn = c.take(4 * VH); L.vfw = c.take((size_t)VH * HW); L.vfb = c.take(1);
    L.total = c.off;
    return L;
}
const Layout& layout() { static const Layout L = make_layout(); return L; }
}  // namespace

size_t weights_count() { return layout().total; }

// tch-default initialisation, the same rules as the backgammon blob's (nn_host.cpp random_weights_bg)
void random_weights(uint64_t seed, float* blob) {
    const Layout& L = layout();
    uint32_t tid = 0x77700000u;
    auto uni = [&](size_t off, size_t n, float lo, float hi) {
        for (size_t i = 0; i < n; i += 4) {
            uint32_t o[4];
            philox4x32((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(i / 4), 0u, tid, 0x57E16u, o);
            for (size_t k = 0; k < 4 && i + k < n; ++k) blob[off + i + k] = lo + (hi - lo) * ((float)(o[k] >> 8) * (1.0f / 16777216.0f));
        }
        ++tid;
    };
    auto cst = [&](size_t off, size_t n, float v) { for (size_t i = 0; i < n; ++i) blob[off + i] = v; };
    auto conv = [&](size_t w, size_t b, int cout, int cin) {
        const float bd = 1.0f / std::sqrt((float)(cin * 9));
        uni(w, (size_t)cout * cin * 9, -bd, bd); cst(b, cout, 0.f);
    };
    auto bn = [&](size_t o, int c) { uni(o, c, 0.f, 1.f); cst(o + c, c, 0.f); cst(o + 2 * (size_t)c, c, 0.f); cst(o + 3 * (size_t)c, c, 1.f); };
    conv(L.init_w, L.init_b, F, CIN); bn(L.init_bn, F);
    for (int i = 0; i < BLOCKS; ++i) { conv(L.c1w[i], L.c1b[i], F, F); conv(L.c2w[i], L.c2b[i], F, F); bn(L.bn1[i], F); bn(L.bn2[i], F); }
    conv(L.pw, L.pb, PH, F); bn(L.pbn, PH);
    { const float bd = 1.0f / std::sqrt((float)(PH * HW)); uni(L.pfw, (size_t)A * PH * HW, -bd, bd); uni(L.pfb, A, -bd, bd); }
    conv(L.vw, L.vb, VH, F); bn(L.vbn, VH);
    { const float bd = 1.0f / std::sqrt((float)(VH * HW)); uni(L.vfw, (size_t)VH * HW, -bd, bd); uni(L.vfb, 1, -bd, bd); }
}

Engine::Engine(int device) : device_(device) {}
Engine::~Engine() = default;

namespace {
[[noreturn]] void unsupported_option(const std::string& key) {
    throw EngineError(DIEE_ERR_UNSUPPORTED, "a tic-tac-toe ctx has the options `nn`, `search`, `search_fused` and the read-only `search_last_launches`, `self_play_last_launches`, `arena_last_launches` and `search_fused_lds_iters`; `" + key + "` belongs to a backgammon ctx");
}
}  // namespace

void Engine::set_option(const std::string& key, const std::string& value) {
    if (key == "search") {
        if (value == "host") { dselfplay_.reset(); darena_.reset(); dsearch_.reset(); dvanilla_.reset(); return; }
        if (value != "device") throw EngineError(DIEE_ERR_ARG, "option search: `" + value + "` is neither `host` nor `device`");
        if (!dev_) throw EngineError(DIEE_ERR_ARG, "option search = device needs option nn = device: the device search evaluates the device network");
        if (!dvanilla_) dvanilla_.reset(new DeviceVanilla(*dev_));
        if (!dsearch_) dsearch_.reset(new DeviceSearch(*dev_));              // buffers come with the first search
        if (!darena_) darena_.reset(new DeviceArena(*dev_, *dsearch_, *dvanilla_));
        if (!dselfplay_) dselfplay_.reset(new DeviceSelfPlay(*dev_, *dsearch_));
        return;
    }
    if (key == "search_fused") {                                             // lives in dsearch_: search = host resets it with the rest
        if (value != "0" && value != "1" && value != "2") throw EngineError(DIEE_ERR_ARG, "option search_fused: `" + value + "` is none of `0`, `1`, `2`");
        if (value != "0" && !dsearch_) throw EngineError(DIEE_ERR_ARG, "option search_fused = " + value + " needs option search = device: it names a kernel of the device search");
        if (dsearch_) dsearch_->set_fused((uint32_t)(value[0] - '0'));
        return;
    }
    if (key == "search_last_launches" || key == "self_play_last_launches" || key == "arena_last_launches" || key == "search_fused_lds_iters") throw EngineError(DIEE_ERR_ARG, "option " + key + " is read-only");
    if (key != "nn") unsupported_option(key);
    if (value == "host") {
        if (dsearch_) throw EngineError(DIEE_ERR_ARG, "option nn = host while option search is `device`: set search = host first");
        dev_.reset();
        return;
    }
    if (value != "device") throw EngineError(DIEE_ERR_ARG, "option nn: `" + value + "` is neither `host` nor `device`");
    if (dev_) return;
    std::unique_ptr<DeviceNet> d(new DeviceNet(device_));                // throws DIEE_ERR_HIP without a usable GPU: dev_ stays empty
    dev_ = std::move(d);
    try { if (loaded()) upload(); } catch (...) { dev_.reset(); throw; }
}
std::string Engine::get_option(const std::string& key) const {
    if (key == "search") return dsearch_ ? "device" : "host";
    if (key == "search_fused") return std::to_string(dsearch_ ? dsearch_->fused_level() : 0u);
    if (key == "search_last_launches") return std::to_string(dsearch_ ? dsearch_->last_launches() : 0u);
    if (key == "self_play_last_launches") return std::to_string(dsearch_ ? dsearch_->self_play_launches() : 0u);
    if (key == "arena_last_launches") return std::to_string(darena_ ? darena_->last_launches() : 0u);
    if (key == "search_fused_lds_iters") return std::to_string(kRunLdsIters);
    if (key != "nn") unsupported_option(key);
    return dev_ ? "device" : "host";
}
void Engine::upload() const { dev_->upload(init_, c1_, c2_, pconv_, vconv_, pfc_w_, pfc_b_, vfc_w_, vfc_b_); }

void Engine::load_weights(const float* blob, size_t n) {
    const Layout& L = layout();
    if (n != L.total) throw EngineError(DIEE_ERR_ARG, "weight blob has " + std::to_string(n) + " floats, expected " + std::to_string(L.total));
    // eval-mode BatchNorm (eps 1e-5) folded into the convolution: w' = w * s, b' = (b - mean) * s + beta
    auto fold = [&](Conv& c, size_t w, size_t b, size_t bnp, int cout, int cin) {
        c.cout = cout; c.cin = cin; c.w.assign((size_t)cout * cin * 9, 0.f); c.b.assign(cout, 0.f);
        for (int o = 0; o < cout; ++o) {
            const float s = blob[bnp + o] / std::sqrt(blob[bnp + 3 * (size_t)cout + o] + 1e-5f);
            for (int k = 0; k < cin * 9; ++k) c.w[(size_t)o * cin * 9 + k] = blob[w + (size_t)o * cin * 9 + k] * s;
            c.b[o] = (blob[b + o] - blob[bnp + 2 * (size_t)cout + o]) * s + blob[bnp + (size_t)cout + o];
        }
    };
    fold(init_, L.init_w, L.init_b, L.init_bn, F, CIN);
    for (int i = 0; i < BLOCKS; ++i) { fold(c1_[i], L.c1w[i], L.c1b[i], L.bn1[i], F, F); fold(c2_[i], L.c2w[i], L.c2b[i], L.bn2[i], F, F); }
    fold(pconv_, L.pw, L.pb, L.pbn, PH, F); fold(vconv_, L.vw, L.vb, L.vbn, VH, F);
    pfc_w_.assign(blob + L.pfw, blob + L.pfw + (size_t)A * PH * HW); pfc_b_.assign(blob + L.pfb, blob + L.pfb + A);
    vfc_w_.assign(blob + L.vfw, blob + L.vfw + (size_t)VH * HW); vfc_b_.assign(blob + L.vfb, blob + L.vfb + 1);
    w_.assign(blob, blob + n);
    // a failed upload must not leave "device" answering with the previous network: the ctx falls back to "host" (which holds the new
    // weights, and the host search with it) and the caller gets the HIP error, as in set_option
    if (dev_) { try { upload(); } catch (...) { dselfplay_.reset(); darena_.reset(); dsearch_.reset(); dvanilla_.reset(); dev_.reset(); throw; } }
}

// ---- the network, fp32 ------------------------------------------------------------------------------------------------
namespace {
// y[cout][3][3] = conv3x3(x[cin][3][3], pad 1) + b
void conv3x3(const float* x, const std::vector<float>& w, const std::vector<float>& b, int cout, int cin, float* y) {
    for (int o = 0; o < cout; ++o) {
        float acc[9];
        for (int p = 0; p < 9; ++p) acc[p] = b[o];
        const float* wo = w.data() + (size_t)o * cin * 9;
        for (int c = 0; c < cin; ++c) {
            const float* xc = x + c * 9; const float* wc = wo + c * 9;
            for (int py = 0; py < 3; ++py)
                for (int px = 0; px < 3; ++px) {
                    float s = 0.f;
                    for (int ky = 0; ky < 3; ++ky) {
                        const int yy = py + ky - 1;
                        if (yy < 0 || yy > 2) continue;
                        for (int kx = 0; kx < 3; ++kx) {
                            const int xx = px + kx - 1;
                            if (xx < 0 || xx > 2) continue;
                            s += xc[yy * 3 + xx] * wc[ky * 3 + kx];
                        }
                    }
                    acc[py * 3 + px] += s;
                }
        }
        for (int p = 0; p < 9; ++p) y[o * 9 + p] = acc[p];
    }
}
inline void relu(float* x, int n) { for (int i = 0; i < n; ++i) x[i] = x[i] > 0.f ? x[i] : 0.f; }
}  // namespace

void Engine::forward(const diee_ttt_state* s, uint32_t n, float* policy, float* value) const {
    if (!loaded()) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called");
    if (dev_) { dev_->forward(s, n, policy, value); return; }
    std::vector<float> x(F * 9), h(F * 9), t(F * 9), in(PLANES), ph(PH * 9), vh(VH * 9);
    for (uint32_t i = 0; i < n; ++i) {
        planes(s[i], in.data());
        conv3x3(in.data(), init_.w, init_.b, F, CIN, x.data()); relu(x.data(), F * 9);          // nnet.rs:64-67
        for (int b = 0; b < BLOCKS; ++b) {                                                     // ResBlock::forward_t, nnet.rs:24-34
            conv3x3(x.data(), c1_[b].w, c1_[b].b, F, F, h.data()); relu(h.data(), F * 9);
            conv3x3(h.data(), c2_[b].w, c2_[b].b, F, F, t.data());
            for (int k = 0; k < F * 9; ++k) { const float v = t[k] + x[k]; x[k] = v > 0.f ? v : 0.f; }
        }
        conv3x3(x.data(), pconv_.w, pconv_.b, PH, F, ph.data()); relu(ph.data(), PH * 9);     // policy head, nnet.rs:75-85
        float logit[A], mx = -INFINITY;
        for (int a = 0; a < A; ++a) {
            float acc = pfc_b_[a];
            for (int k = 0; k < PH * HW; ++k) acc += ph[k] * pfc_w_[(size_t)a * PH * HW + k];  // flatten: c * 9 + p
            logit[a] = acc; mx = acc > mx ? acc : mx;
        }
        float sum = 0.f;
        for (int a = 0; a < A; ++a) { logit[a] = std::exp(logit[a] - mx); sum += logit[a]; }
        for (int a = 0; a < A; ++a) policy[(size_t)i * A + a] = logit[a] / sum;
        conv3x3(x.data(), vconv_.w, vconv_.b, VH, F, vh.data()); relu(vh.data(), VH * 9);     // value head, nnet.rs:87-98
        float acc = vfc_b_[0];
        for (int k = 0; k < VH * HW; ++k) acc += vh[k] * vfc_w_[k];
        value[i] = std::tanh(acc);
    }
}

// ---- the batched search: alpha_mcts_parallel on one NodeStore laid out as arrays ----------------------------------------
namespace {
struct Store {                       // NodeStore<TicTacToe>, node_store.rs:9-11 (index = creation order, roots first)
    std::vector<diee_ttt_state> state;
    std::vector<int32_t> parent, first_child, n_children, action;
    std::vector<float> visits, value, prior;
    std::vector<uint8_t> drained;
    int add(const diee_ttt_state& s, int par, int act, float pr) {
        state.push_back(s); parent.push_back(par); first_child.push_back(-1); n_children.push_back(0); action.push_back(act);
        visits.push_back(0.f); value.push_back(0.f); prior.push_back(pr); drained.push_back(0);
        return (int)state.size() - 1;
    }
    size_t size() const { return state.size(); }
};

// Node::alpha_ucb, node.rs:98-112, f32 in this association
inline float ucb(const Store& T, int idx, float c) {
    const float n = T.visits[idx];
    const float q = n == 0.f ? 0.f : T.value[idx] / n;
    const float t = std::sqrt(T.visits[T.parent[idx]]) / (n + 1.0f);
    const float u = c * t;
    const float w = u * T.prior[idx];
    return q + w;
}
// alpha_select_leaf_node + select_alpha, alpha_mcts.rs:14-33: Iterator::max_by keeps the LAST of equal maxima; NaN compares Equal
int select_leaf(const Store& T, int root, float c, int& depth) {
    int idx = root; depth = 0;
    while (T.n_children[idx] != 0) {
        int best = T.first_child[idx];
        float ub = ucb(T, best, c);
        for (int j = 1; j < T.n_children[idx]; ++j) {
            const int ch = T.first_child[idx] + j;
            const float un = ucb(T, ch, c);
            if (!(ub > un)) { best = ch; ub = un; }
        }
        idx = best; ++depth;
    }
    return idx;
}
void backpropagate(Store& T, int idx, float v) {                       // simple_mcts.rs:96-103: same sign at every level
    for (; idx >= 0; idx = T.parent[idx]) { T.visits[idx] += 1.0f; T.value[idx] += v; }
}
// turn_policy_to_probs_tensor (utils.rs:74-84) + alpha_expand_tensor (node.rs:157-174)
void expand(Store& T, int idx, const float* policy_row, diee_stats* st) {
    if (T.drained[idx]) return;
    const diee_ttt_state s = T.state[idx];
    uint8_t mv[9];
    const int k = valid_moves(s, mv);
    float sum = 0.f;
    for (int j = 0; j < k; ++j) sum += policy_row[mv[j]];              // encode(action) = action, mod.rs:100-102
    const int first = (int)T.size();
    for (int j = 0; j < k; ++j) {
        diee_ttt_state ns = s;
        apply_move(ns, mv[j]);
        T.add(ns, idx, mv[j], policy_row[mv[j]] / sum);
    }
    T.first_child[idx] = k ? first : -1; T.n_children[idx] = k; T.drained[idx] = 1;
    if (st) { st->expansions += 1; st->children += (uint64_t)k; if ((uint64_t)k > st->max_children) st->max_children = (uint64_t)k; }
}

void host_search(const Engine& net, Store& T, const diee_ttt_state* roots, int n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step,
                 bool quirks, diee_stats* st) {
    std::vector<float> policy((size_t)n * A), value(n), noise(A);
    std::vector<diee_ttt_state> batch(roots, roots + n);
    net.forward(batch.data(), (uint32_t)n, policy.data(), value.data());                   // forward_policy, :104
    if (st) st->nn_evals += (uint64_t)n;
    dirichlet_host(seed, step, cfg.dir_alpha, A, noise.data());                            // apply_dirichlet, noise.rs:27-34: ONE sample for all rows
    const float eps = cfg.dir_eps, om = 1.0f - eps;
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < A; ++a) {
            const float x = om * policy[(size_t)i * A + a], y = eps * noise[a];
            policy[(size_t)i * A + a] = x + y;
        }
    for (int i = 0; i < n; ++i) T.add(roots[i], -1, -1, 0.f);                              // :110-112
    for (int i = 0; i < n; ++i) { T.visits[i] = 1.0f; expand(T, i, &policy[(size_t)i * A], st); }   // :119-127
    std::vector<int> sel(n, 0);                                                            // :142 vec![0; n]
    std::vector<uint8_t> fresh(n, 0);
    for (uint32_t it = 0; it < cfg.iterations; ++it) {                                     // :149
        bool node_selected = false;
        for (int g = 0; g < n; ++g) {                                                      // :153-168
            int depth = 0, winner = 0;
            const int idx = select_leaf(T, g, cfg.c, depth);
            if (st) { st->selections += 1; st->depth_sum += (uint64_t)depth; }
            fresh[g] = 0;
            if (check_winner(T.state[idx], winner)) {
                const int rp = T.state[g].player;
                backpropagate(T, idx, winner == rp ? 1.0f : (winner == -rp ? -1.0f : 0.0f));
                if (st) st->terminal_hits += 1;
            } else { node_selected = true; sel[g] = idx; fresh[g] = 1; }
        }
        if (!node_selected) continue;                                                      // :170-172
        for (int g = 0; g < n; ++g) batch[g] = T.state[sel[g]];                            // :175-183, stale slots included
        net.forward(batch.data(), (uint32_t)n, policy.data(), value.data());               // :186
        if (st) st->nn_evals += (uint64_t)n;
        for (int slot = 0; slot < n; ++slot) {                                             // :192-200
            if (!quirks && !fresh[slot]) continue;                                         // Q14 off: no stale re-backpropagation
            expand(T, sel[slot], &policy[(size_t)slot * A], st);
            backpropagate(T, sel[slot], value[slot]);
        }
    }
}

// get_prob_tensor_parallel, utils.rs:42-58 (row sums taken over the children in order)
void root_probs(const Store& T, int i, float* row) {
    for (int a = 0; a < A; ++a) row[a] = T.n_children[i] ? 0.f : NAN;
    float sum = 0.f;
    for (int j = 0; j < T.n_children[i]; ++j) sum += T.visits[T.first_child[i] + j];
    for (int j = 0; j < T.n_children[i]; ++j) row[T.action[T.first_child[i] + j]] = T.visits[T.first_child[i] + j] / sum;
}

int weighted_select(const float* w, double u01) {                      // alphazero.rs:129-137, rand WeightedIndex over f64
    double total = 0.0;
    for (int a = 0; a < A; ++a) total += (double)w[a];
    const double x = u01 * total;
    double cum = 0.0;
    int last_nz = 0;
    for (int a = 0; a < A; ++a) {
        if (w[a] != 0.0f) last_nz = a;
        cum += (double)w[a];
        if (cum > x) return a;
    }
    return last_nz;
}
}  // namespace

void Engine::search(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step, bool quirks, diee_stats* st,
                    RootResult& R) const {
    if (dsearch_) { dsearch_->run(roots, n, cfg, seed, step, quirks, st, R); return; }
    Store T;                                                                               // alpha_parallel.rs:137: a fresh NodeStore every search
    host_search(*this, T, roots, (int)n, cfg, seed, step, quirks, st);
    R.probs.resize((size_t)n * A); R.n_children.resize(n); R.root_visits.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        root_probs(T, (int)i, &R.probs[(size_t)i * A]);
        R.n_children[i] = (uint32_t)T.n_children[i];
        R.root_visits[i] = T.visits[i];
    }
}

void Engine::mcts_batch(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, uint32_t step,
                        const uint32_t*, const uint32_t*, uint32_t flags, float* visit_probs, uint32_t* n_children, float* root_visits,
                        diee_stats* stats) const {
    if (stats) memset(stats, 0, sizeof *stats);
    const auto t0 = std::chrono::steady_clock::now();
    RootResult R;
    search(roots, n, cfg, seed, step, (flags & DIEE_FLAG_REF_QUIRKS) != 0, stats, R);
    memcpy(visit_probs, R.probs.data(), R.probs.size() * sizeof(float));
    if (n_children) memcpy(n_children, R.n_children.data(), (size_t)n * sizeof(uint32_t));
    if (root_visits) memcpy(root_visits, R.root_visits.data(), (size_t)n * sizeof(float));
    if (stats) { stats->nn_rows = stats->nn_evals; stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
}

void Engine::self_play(uint32_t n_games, uint32_t first_game_id, const diee_mcts_cfg& cfg, float temperature, uint64_t seed,
                       uint32_t flags, uint32_t max_steps, diee_fragments* out, diee_stats* stats) const {
    if (!loaded()) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called");
    if (out) memset(out, 0, sizeof *out);
    if (stats) memset(stats, 0, sizeof *stats);
    const bool quirks = (flags & DIEE_FLAG_REF_QUIRKS) != 0;
    const float inv_t = (float)(1.0 / (double)temperature);                                // :165 pow_(1.0 / temperature)
    const auto t0 = std::chrono::steady_clock::now();
    // option search_fused = 2: the whole call is one search-and-play launch and the delivery (ttt_selfplay_device.h); the quirks couple the
    // games of a move-step through the live list, so a call under them takes the loop below
    if (dselfplay_ && dsearch_->fused_level() == 2 && !quirks && dselfplay_->serves(n_games, cfg.iterations)) {
        dselfplay_->run(n_games, first_game_id, cfg, temperature, seed, max_steps, out, stats);
        if (stats) stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return;
    }
    struct Frag { int8_t player; float ps[A]; float st[PLANES]; };
    std::vector<diee_ttt_state> states(n_games);
    std::vector<uint32_t> rounds(n_games, 0);
    std::vector<uint8_t> live(n_games, 1);
    std::vector<std::vector<Frag>> mem(n_games);
    std::vector<int8_t> o_outcome; std::vector<float> o_ps, o_state; std::vector<uint32_t> o_game;
    auto flush = [&](uint32_t g, int winner, bool zero) {
        for (const Frag& f : mem[g]) {
            o_outcome.push_back(zero ? 0 : (winner == f.player ? 1 : (winner == -f.player ? -1 : 0)));   // :216-217
            o_ps.insert(o_ps.end(), f.ps, f.ps + A); o_state.insert(o_state.end(), f.st, f.st + PLANES);
            o_game.push_back(first_game_id + g);
        }
    };
    for (uint32_t g = 0; g < n_games; ++g) { memset(&states[g], 0, sizeof states[g]); states[g].player = -1; }   // TicTacToe::new, mod.rs:28-30
    uint32_t n_live = n_games, steps = 0, launches = 0;
    std::vector<diee_ttt_state> roots; std::vector<uint32_t> ids;
    std::vector<float> row(A);
    RootResult R;
    while (n_live > 0 && (max_steps == 0 || steps < max_steps)) {                          // alpha_parallel.rs:129
        roots.clear(); ids.clear();
        for (uint32_t g = 0; g < n_games; ++g) if (live[g]) { roots.push_back(states[g]); ids.push_back(g); }
        search(roots.data(), (uint32_t)roots.size(), cfg, seed, steps, quirks, stats, R);   // :137 a fresh NodeStore every move-step, :146
        if (dsearch_) launches += dsearch_->last_launches();
        for (size_t pi = 0; pi < ids.size(); ++pi) {                                       // :168-224
            const uint32_t g = ids[pi];
            bool removed = false, flushed = false;
            if (rounds[g] >= cfg.round_limit) { flush(g, 0, true); removed = true; flushed = true; }      // :172-180, no `continue`
            if (R.n_children[pi] == 0) {                                                   // :183-189
                rounds[g] += 1; skip_turn(states[g]);
                if (stats) stats->plies += 1;
                if (removed) { live[g] = 0; --n_live; if (stats) stats->games += 1; }
                continue;
            }
            memcpy(row.data(), &R.probs[pi * A], A * sizeof(float));                       // :164
            for (int a = 0; a < A; ++a) row[a] = det_powf(row[a], inv_t);                  // :165, not renormalised (Q17)
            const int a = weighted_select(row.data(), draw_uniform(seed, first_game_id + g, rounds[g], kTagSample, 0u));   // :192
            Frag f; f.player = states[g].player;                                           // :195-199
            memcpy(f.ps, row.data(), sizeof f.ps); planes(states[g], f.st);
            mem[g].push_back(f);
            uint8_t vm[9];                                                                 // :202-210 decode, assert legal, apply
            const int k = valid_moves(states[g], vm);
            bool ok = false;
            for (int j = 0; j < k; ++j) ok = ok || vm[j] == (uint8_t)a;
            if (!ok && stats) stats->illegal_decodes += 1;
            apply_move(states[g], (uint8_t)a);
            rounds[g] += 1;                                                                // :213
            if (stats) stats->plies += 1;
            int winner = 0;
            if (check_winner(states[g], winner)) {                                         // :215-223
                if (!(flushed && !quirks)) flush(g, winner, false);                        // Q18: the reference flushes twice
                removed = true;
            }
            if (removed) { live[g] = 0; --n_live; if (stats) stats->games += 1; }
        }
        ++steps;
    }
    if (dsearch_) dsearch_->report_launches(dsearch_->last_launches(), launches);
    const size_t nf = o_outcome.size();
    if (stats) {
        stats->move_steps = steps; stats->fragments = nf; stats->nn_rows = stats->nn_evals;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!out || nf == 0) return;
    out->outcome = (int8_t*)malloc(nf); out->ps = (float*)malloc(nf * A * sizeof(float));
    out->state = (float*)malloc(nf * PLANES * sizeof(float)); out->game = (uint32_t*)malloc(nf * sizeof(uint32_t));
    if (!out->outcome || !out->ps || !out->state || !out->game) { diee_free_fragments(out); throw std::bad_alloc(); }
    memcpy(out->outcome, o_outcome.data(), nf); memcpy(out->ps, o_ps.data(), nf * A * sizeof(float));
    memcpy(out->state, o_state.data(), nf * PLANES * sizeof(float)); memcpy(out->game, o_game.data(), nf * sizeof(uint32_t));
    out->n = (uint32_t)nf;
}

// ---- Agent::Mcts: mct_search (simple_mcts.rs:10-39) with Node::expand / simulate (node.rs:118-137,176-196), one root at a time ------------
namespace {
struct VNode {                       // node.rs:10-22; expandable_moves is the first n_moves - n_children of the node's empty cells
    diee_ttt_state state;
    int parent, n_children, child[9];
    uint32_t visits;
    float value;
};
inline float result_for(int winner, int player) { return winner == player ? 1.0f : (winner == -player ? -1.0f : 0.0f); }

struct VanillaRoot { uint8_t move; uint32_t n_children; float child_visits[9], child_values[9]; };

VanillaRoot vanilla_search_host(const diee_ttt_state& root, const diee_mcts_cfg& cfg, const std::vector<float>& ln, uint64_t seed, uint32_t game,
                                uint32_t round, bool quirks, diee_vanilla_stats* st) {
    VanillaRoot R{};
    R.move = 10;                                                                           // TicTacToe::EMPTY_MOVE, mod.rs:18
    int winner = 0;
    if (check_winner(root, winner)) return R;                                              // simple_mcts.rs:12-14
    const int player = root.player;
    std::vector<VNode> T;
    T.reserve((size_t)cfg.iterations + 1);
    auto add = [&](const diee_ttt_state& s, int parent) { VNode nd{}; nd.state = s; nd.parent = parent; T.push_back(nd); return (int)T.size() - 1; };
    add(root, -1);
    uint8_t mv[9];
    for (uint32_t it = 0; it < cfg.iterations; ++it) {                                     // :17-37
        int idx = 0;
        uint64_t depth = 0;
        while (T[idx].n_children != 0 && T[idx].n_children == valid_moves(T[idx].state, mv)) {     // :88-94
            const VNode& nd = T[idx];
            const float cl = cfg.c * ln[nd.visits];
            int best = -1;
            float ub = 0.f;
            for (int j = 0; j < nd.n_children; ++j) {                                      // node.rs:86-96, max_by: the last of equal maxima
                const VNode& ch = T[nd.child[j]];
                const float v = (float)ch.visits;
                const float q = ch.value / v;
                const float e = std::sqrt(cl / v);
                const float un = q + e;
                if (best < 0 || !(ub > un)) { best = nd.child[j]; ub = un; }
            }
            idx = best; ++depth;
        }
        st->iterations += 1; st->depth_sum += depth;
        float res = 0.f;
        int from = idx;
        if (check_winner(T[idx].state, winner)) {                                          // :25-30
            res = result_for(winner, player);
            st->terminal_hits += 1;
        } else {
            const int k = valid_moves(T[idx].state, mv);                                   // expand: expandable_moves.pop()
            diee_ttt_state sim = T[idx].state;
            apply_move(sim, mv[k - 1 - T[idx].n_children]);
            from = add(sim, idx);
            T[idx].child[T[idx].n_children++] = from;
            st->expansions += 1; st->rollouts += 1;
            if (quirks) {                                                                  // Q22: the loop looks at the node's own state and plays nothing
                if (cfg.round_limit > 0 && check_winner(sim, winner)) { res = result_for(winner, player); st->rollout_decided += 1; }
            } else {
                for (uint32_t p = 0; p < cfg.round_limit; ++p) {
                    if (check_winner(sim, winner)) { res = result_for(winner, player); st->rollout_decided += 1; break; }
                    const int k1 = valid_moves(sim, mv);
                    int pick = (int)(draw_uniform(seed, game, round, kTagVanilla, (it << 12) | (1u + p)) * (double)k1);
                    pick = pick > k1 - 1 ? k1 - 1 : pick;
                    apply_move(sim, mv[pick]);
                    st->rollout_plies += 1;
                }
            }
        }
        for (int i = from; i >= 0; i = T[i].parent) { T[i].visits += 1u; T[i].value += res; }      // :96-103: the same sign at every level
    }
    const VNode& r = T[0];
    R.n_children = (uint32_t)r.n_children;
    uint32_t bv = 0;
    for (int j = 0; j < r.n_children; ++j) {                                               // :71-86 max_by_key(visits): the last of equal maxima
        const VNode& ch = T[r.child[j]];
        R.child_visits[j] = (float)ch.visits; R.child_values[j] = ch.value;
        if (ch.visits >= bv) {
            bv = ch.visits;
            for (int cidx = 0; cidx < 9; ++cidx) if (r.state.board[cidx] == 0 && ch.state.board[cidx] != 0) R.move = (uint8_t)cidx;
        }
    }
    return R;
}
}  // namespace

void Engine::mcts_vanilla_batch(const diee_ttt_state* roots, uint32_t n, const diee_mcts_cfg& cfg, uint64_t seed, const uint32_t* game_ids,
                                const uint32_t* rounds, uint32_t flags, uint8_t* moves, uint32_t* n_children, float* child_visits,
                                float* child_values, diee_vanilla_stats* stats) const {
    diee_vanilla_stats st{};
    if (stats) *stats = st;
    vanilla_check_cfg(cfg);
    // a node keeps its board at 2 bits per cell and its player in one: what the rules produce from any legal position.  Then a node that
    // is not a finished game always has a move
    for (uint32_t i = 0; i < n; ++i) {
        bool ok = roots[i].player == 1 || roots[i].player == -1;
        for (int cidx = 0; cidx < 9; ++cidx) ok = ok && roots[i].board[cidx] >= -1 && roots[i].board[cidx] <= 1;
        if (!ok) throw EngineError(DIEE_ERR_ARG, "Agent::Mcts: root " + std::to_string(i) + " has a cell or a player outside -1 / 0 / +1");
    }
    if (!n) return;
    const bool quirks = (flags & DIEE_FLAG_REF_QUIRKS) != 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto answer = [&](uint32_t i, uint32_t move, uint32_t nc, const float* cv, const float* cw) {
        moves[i] = (uint8_t)move;
        if (n_children) n_children[i] = nc;
        if (child_visits) memcpy(child_visits + (size_t)i * A, cv, A * sizeof(float));
        if (child_values) memcpy(child_values + (size_t)i * A, cw, A * sizeof(float));
    };
    if (dvanilla_) {
        const VanillaOut* out = dvanilla_->run(roots, n, cfg, seed, game_ids, rounds, quirks);     // throws before anything is written
        for (uint32_t i = 0; i < n; ++i) {
            const VanillaOut& o = out[i];
            answer(i, o.move, o.n_children, o.child_visits, o.child_values);
            st.iterations += o.cnt[kVcIterations]; st.expansions += o.cnt[kVcExpansions]; st.terminal_hits += o.cnt[kVcTerminal];
            st.rollouts += o.cnt[kVcRollouts]; st.rollout_plies += o.cnt[kVcPlies]; st.rollout_decided += o.cnt[kVcDecided];
            st.depth_sum += o.cnt[kVcDepthSum];
        }
    } else {
        std::vector<float> ln((size_t)cfg.iterations + 2, 0.0f);                                   // the table the device search reads
        for (size_t k = 1; k < ln.size(); ++k) ln[k] = (float)std::log((double)k);
        for (uint32_t i = 0; i < n; ++i) {
            const VanillaRoot r = vanilla_search_host(roots[i], cfg, ln, seed, game_ids ? game_ids[i] : i, rounds ? rounds[i] : 0u, quirks, &st);
            answer(i, r.move, r.n_children, r.child_visits, r.child_values);
        }
    }
    if (stats) { *stats = st; stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
}

// ---- the arena: play() / get_actions_for_player (versus.rs:160-318) for TicTacToe -------------------------------------------------------------
void Engine::arena(const Engine* e1, int agent1, const Engine* e2, int agent2, uint32_t n_games, const diee_mcts_cfg& cfg, float temperature,
                   uint64_t seed, uint32_t round_limit, uint32_t max_rounds, const uint32_t flags[2], diee_arena_result* res, int8_t* winner,
                   uint32_t* retired_round, int8_t* retired_side, diee_ttt_state* final_states, diee_stats* stats) const {
    if (res) memset(res, 0, sizeof *res);
    if (stats) memset(stats, 0, 2 * sizeof(diee_stats));
    if (n_games == 0 || round_limit == 0) throw EngineError(DIEE_ERR_ARG, "the arena needs n_games >= 1 and round_limit >= 1");
    if (n_games > (1u << 22)) throw EngineError(DIEE_ERR_ARG, "too many games in flight");
    const Engine* const eng[2] = {e1, e2};
    const int agents[2] = {agent1, agent2};
    bool any_mcts = false;
    for (int s = 0; s < 2; ++s) {
        if (agents[s] != DIEE_AGENT_RANDOM && agents[s] != DIEE_AGENT_MODEL && agents[s] != DIEE_AGENT_MCTS)
            throw EngineError(DIEE_ERR_ARG, "agent: DIEE_AGENT_RANDOM, DIEE_AGENT_MODEL or DIEE_AGENT_MCTS");
        if (agents[s] == DIEE_AGENT_MODEL && !eng[s]) throw EngineError(DIEE_ERR_ARG, "a Model agent needs its ctx");
        if (agents[s] == DIEE_AGENT_MODEL && !eng[s]->loaded()) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called for a Model agent's ctx");
        any_mcts = any_mcts || agents[s] == DIEE_AGENT_MCTS;
    }
    if (any_mcts) vanilla_check_cfg(cfg);
    if (darena_) {
        ArenaArgs a{};
        for (int s = 0; s < 2; ++s) {
            if (eng[s] && (!eng[s]->dsearch_ || eng[s]->device_ != device_))
                throw EngineError(DIEE_ERR_ARG, "the device arena needs every ctx of the call on option search = device and on the hosting ctx's GPU");
            a.agents[s] = agents[s]; a.flags[s] = flags[s];
            a.nets[s] = agents[s] == DIEE_AGENT_MODEL ? &eng[s]->dev_->params() : nullptr;
        }
        a.n_games = n_games; a.cfg = cfg; a.temperature = temperature; a.seed = seed; a.round_limit = round_limit; a.max_rounds = max_rounds;
        // option search_fused = 2: the whole call is one launch of k_ttt_arena_run (ttt_arena_device.h), unless a game outlasts its nine rounds
        if (darena_->serves(a) && darena_->run_one_launch(a, res, winner, retired_round, retired_side, final_states, stats)) return;
        darena_->run(a, res, winner, retired_round, retired_side, final_states, stats);
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const float inv_t = (float)(1.0 / (double)temperature);                                // :283 pow_(1.0 / temp)
    std::vector<diee_ttt_state> states(n_games), roots;
    std::vector<int8_t> win(n_games, 0), rside(n_games, -1);
    std::vector<uint32_t> rround(n_games, 0xFFFFFFFFu), ids, rounds;
    std::vector<uint8_t> moves;
    for (uint32_t g = 0; g < n_games; ++g) { memset(&states[g], 0, sizeof states[g]); states[g].player = g < n_games / 2 ? -1 : 1; }     // :172-174
    diee_stats st[2];
    memset(st, 0, sizeof st);
    diee_arena_result r{};
    RootResult R;
    uint32_t round = 0;
    for (;;) {                                                                             // :191
        std::vector<uint32_t> lists[2];                                                    // :195-196, ascending game index
        for (uint32_t g = 0; g < n_games; ++g) if (rround[g] == 0xFFFFFFFFu) lists[states[g].player == -1 ? 0 : 1].push_back(g);
        if (lists[0].empty() && lists[1].empty()) break;
        if (max_rounds != 0 && round >= max_rounds) break;
        for (int s = 0; s < 2; ++s) {
            ids = lists[s];
            const uint32_t n = (uint32_t)ids.size();
            if (!n) continue;
            roots.clear();
            for (uint32_t g : ids) roots.push_back(states[g]);
            rounds.assign(n, round);
            moves.assign(n, 10);                                                           // TicTacToe::EMPTY_MOVE
            const bool quirks = (flags[s] & DIEE_FLAG_REF_QUIRKS) != 0;
            if (agents[s] == DIEE_AGENT_MODEL) {                                           // :279-299
                eng[s]->search(roots.data(), n, cfg, seed, 2 * round + (uint32_t)s, quirks, &st[s], R);
                st[s].move_steps += 1;
                for (uint32_t k = 0; k < n; ++k) {
                    float row[A];
                    double total = 0.0;
                    for (int c = 0; c < A; ++c) {
                        const float x = R.probs[(size_t)k * A + c];
                        row[c] = det_powf(x > 0.f ? x : 0.f, inv_t);                       // (NaN, the row of a childless root: 0)
                        total += (double)row[c];
                    }
                    if (R.n_children[k] != 0 && total > 0.0)                               // :286-293: else EMPTY_MOVE
                        moves[k] = (uint8_t)weighted_select(row, draw_uniform(seed, ids[k], round, kTagSample, 0u));
                }
            } else if (agents[s] == DIEE_AGENT_MCTS) {                                     // :303-306
                diee_vanilla_stats vs;
                (eng[s] ? eng[s] : this)->mcts_vanilla_batch(roots.data(), n, cfg, seed, ids.data(), rounds.data(), flags[s], moves.data(), nullptr, nullptr,
                                                             nullptr, &vs);
                st[s].move_steps += 1;
                st[s].selections += vs.iterations; st[s].expansions += vs.expansions; st[s].terminal_hits += vs.terminal_hits; st[s].depth_sum += vs.depth_sum;
            } else {                                                                       // :308-317
                for (uint32_t k = 0; k < n; ++k) {
                    uint8_t mv[9];
                    const int count = valid_moves(roots[k], mv);
                    if (!count) continue;
                    const int idx = (int)(draw_uniform(seed, ids[k], round, kTagSample, 0u) * (double)count);
                    moves[k] = mv[idx > count - 1 ? count - 1 : idx];
                }
            }
            for (uint32_t k = 0; k < n; ++k) {                                             // :220-266
                const uint32_t g = ids[k];
                st[s].plies += 1;
                if (moves[k] > 8) { skip_turn(states[g]); continue; }                      // :225-228: no winner / round-limit check
                apply_move(states[g], moves[k]);                                           // :230
                st[s].fragments += 1;
                int w = 0;
                if (!check_winner(states[g], w) && round + 1 < round_limit) continue;      // :233-237 (round_count was incremented at :219)
                win[g] = (int8_t)w; rround[g] = round; rside[g] = (int8_t)s;
                st[s].games += 1;
                (w < 0 ? r.wins_p1 : w > 0 ? r.wins_p2 : r.draws) += 1;
            }
        }
        ++round;                                                                           // :219
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int s = 0; s < 2; ++s) { st[s].nn_rows = st[s].nn_evals; st[s].seconds = secs; }
    r.rounds = round; r.seconds = secs;
    if (winner) memcpy(winner, win.data(), n_games);
    if (retired_round) memcpy(retired_round, rround.data(), (size_t)n_games * sizeof(uint32_t));
    if (retired_side) memcpy(retired_side, rside.data(), n_games);
    if (final_states) memcpy(final_states, states.data(), (size_t)n_games * sizeof(diee_ttt_state));
    if (stats) memcpy(stats, st, sizeof st);
    if (res) *res = r;
}

}  // namespace ttt
}  // namespace diee
