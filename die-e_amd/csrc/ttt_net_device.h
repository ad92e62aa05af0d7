// ttt_net_device.h -- the tic-tac-toe ResNet as ONE device function, net_eval: the body of k_ttt_net (ttt_kernels.hip, where the design is
// described), shared with k_ttt_search (ttt_search_kernels.hip), which evaluates the selected leaves of its 16 games inside the search
// launch.  Both kernels inline the same statements, so a board's policy and value are the same bits in either kernel, in any row: that is
// what makes the device search bit-exact against the host search over the device network.
#pragma once
#include <hip/hip_runtime.h>

#include "nn_common.h"
#include "ttt_device.h"
#include "ttt_host.h"

namespace diee {
namespace ttt {

#ifdef __HIP_DEVICE_COMPILE__
#define DIEE_TTT_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define DIEE_TTT_NO_PK_F32
#endif

constexpr int kB = kBoardsPerGroup, kRows = 9 * kB, kRowBytes = 144, kActBytes = kRows * kRowBytes;
constexpr int kHeadCh = 35, kHeadFloats = kHeadCh * 9;              // per board: 32 policy channels, then 3 value channels, x 9 positions
constexpr int kFragsPerConv = 18 * 64;                              // uint4 of one N-tile of a 64-channel conv
static_assert(kB == 16, "an M-tile is one board position of the workgroup's boards");

// the LDS of one workgroup's evaluation (62 KB); a kernel declares it once, __shared__
struct NetLds {
    __attribute__((aligned(16))) unsigned char x[kActBytes];        // trunk
    __attribute__((aligned(16))) unsigned char h[kActBytes];        // hidden
    __attribute__((aligned(16))) float head[kB * kHeadFloats];
    uint32_t cells[kB * 3];                                         // board[9], player, 2 bytes of padding per board
    float logit[kB * 9];
};

__device__ __forceinline__ constexpr bool tap_on_board(int p, int t) {
    const int y = p / 3 + t / 3 - 1, x = p % 3 + t % 3 - 1;
    return y >= 0 && y < 3 && x >= 0 && x < 3;
}
__device__ __forceinline__ constexpr int tap_source(int p, int t) { return p + (t / 3 - 1) * 3 + (t % 3 - 1); }

// A function without the attribute is not inlined into one that has it (the feature sets differ) and would stay a real call, so the
// kernels call nothing from the runtime headers that is more than a builtin: this is __syncthreads() spelled out, and 16-byte LDS stores
// go through u32x4, a plain vector.  The build must show 0 bytes of scratch for k_ttt_net and k_ttt_search.
__device__ __forceinline__ DIEE_TTT_NO_PK_F32 __attribute__((convergent)) void group_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ DIEE_TTT_NO_PK_F32 void load_frags(const uint4* w, int lane, uint4 (&f)[18]) {
#pragma unroll
    for (int i = 0; i < 18; ++i) f[i] = w[i * 64 + lane];
}

// acc[p] = conv3x3 of the 64-channel activations `src` for this wave's N-tile, without bias
__device__ __forceinline__ DIEE_TTT_NO_PK_F32 void conv64(const unsigned char* src, int lane, const uint4 (&w)[18], f32x4 (&acc)[9]) {
    bf16x8 a[9][2];
    const unsigned char* base = src + (lane & 15) * kRowBytes + (lane >> 4) * 16;
#pragma unroll
    for (int s = 0; s < 9; ++s)
#pragma unroll
        for (int c = 0; c < 2; ++c) a[s][c] = *(const bf16x8*)(base + s * 16 * kRowBytes + c * 64);
#pragma unroll
    for (int p = 0; p < 9; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const bf16x8 b = __builtin_bit_cast(bf16x8, w[t * 2 + c]);
#pragma unroll
            for (int p = 0; p < 9; ++p)
                if (tap_on_board(p, t)) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a[tap_source(p, t)][c], acc[p], 0, 0, 0);
        }
}

// bias, optional residual from `res` (bf16, same rows), ReLU, bf16 store of channels n0 .. n0 + 3 of this lane's row of every M-tile
__device__ __forceinline__ DIEE_TTT_NO_PK_F32 void store_act(const f32x4 (&acc)[9], const float* bias, int n0, int lane, const unsigned char* res, unsigned char* dst) {
    const float4 bv = *(const float4*)(bias + n0);
    const int off = (lane & 15) * kRowBytes + n0 * 2;
#pragma unroll
    for (int p = 0; p < 9; ++p) {
        float v[4] = {acc[p][0] + bv.x, acc[p][1] + bv.y, acc[p][2] + bv.z, acc[p][3] + bv.w};
        if (res) {
            const uint2 r = *(const uint2*)(res + p * 16 * kRowBytes + off);
            v[0] += bf2f((uint16_t)(r.x & 0xFFFFu)); v[1] += bf2f((uint16_t)(r.x >> 16));
            v[2] += bf2f((uint16_t)(r.y & 0xFFFFu)); v[3] += bf2f((uint16_t)(r.y >> 16));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
        uint2 o;
        o.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
        o.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
        *(uint2*)(dst + p * 16 * kRowBytes + off) = o;
    }
}

// The network over the 16 boards of S.cells.  A thread whose `cell_slot` is >= 0 brings one word of it, S.cells[cell_slot] = cell_word (48
// threads in all: 3 words per board), stored in here BEHIND the first weight requests so that those are in flight while the caller's
// own loads complete.  Every thread of the 256 calls it; on return thread b < 16 holds board b's softmax policy and tanh value, the
// others hold nothing.  S may be reused as soon as the caller has passed a barrier of its own.
__device__ __forceinline__ DIEE_TTT_NO_PK_F32 void net_eval(const NetParams& P, NetLds& S, int tid, int cell_slot, uint32_t cell_word, float (&policy)[9],
                                                            float& value) {
    const int lane = tid & 63, wave = tid >> 6;
    // this wave's first trunk weights are on their way while the planes are built
    uint4 w[18], wn[18];
    load_frags(P.w_trunk + (size_t)wave * kFragsPerConv, lane, w);
    const uint4 w_init = P.w_init[wave * 64 + lane];
    if (cell_slot >= 0) S.cells[cell_slot] = cell_word;
    group_barrier();

    // ---- planes as an im2col tile in h: row (p, b), k = 3 * tap + c = [board[source] == c - 1], 0 off the board and for k >= 27 --------------
    if (tid < kRows) {
        const int p = tid >> 4, b = tid & 15;
        const signed char* cells = (const signed char*)(S.cells + b * 3);
        uint32_t pk[16];
#pragma unroll
        for (int k = 0; k < 32; k += 2) {
            uint32_t two = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int kk = k + j, t = kk / 3, c = kk % 3;
                if (kk < 27) {
                    const int y = p / 3 + t / 3 - 1, x = p % 3 + t % 3 - 1;
                    const bool on = y >= 0 && y < 3 && x >= 0 && x < 3;
                    const int cell = on ? cells[on ? y * 3 + x : 0] : 2;              // 2 matches no plane
                    two |= (cell == c - 1 ? 0x3F80u : 0u) << (16 * j);                // bf16 1.0
                }
            }
            pk[k / 2] = two;
        }
        u32x4* row = (u32x4*)(S.h + tid * kRowBytes);
#pragma unroll
        for (int q = 0; q < 4; ++q) row[q] = u32x4{pk[4 * q], pk[4 * q + 1], pk[4 * q + 2], pk[4 * q + 3]};
    }
    group_barrier();

    const int n0 = wave * 16 + (lane >> 4) * 4;                      // this lane's four output channels of a trunk conv
    f32x4 acc[9];
    // ---- initial conv: one k-step, nothing to skip (the im2col tile holds the padding) -------------------------------------------------------
    {
        const bf16x8 b = __builtin_bit_cast(bf16x8, w_init);
        const unsigned char* base = S.h + (lane & 15) * kRowBytes + (lane >> 4) * 16;
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const bf16x8 a = *(const bf16x8*)(base + p * 16 * kRowBytes);
            acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
        store_act(acc, P.bias + kBiasInit, n0, lane, nullptr, S.x);
    }
    group_barrier();

    // ---- trunk: conv L = 2 * block + {0, 1}; even: x -> h, odd: h -> x with the residual x ----------------------------------------------------
    const int head_tile = wave < 3 ? wave : 2;                       // wave 3 has no head tile: it fetches tile 2 and drops it
#pragma unroll 1
    for (int L = 0; L < 2 * BLOCKS; ++L) {
        const uint4* next = L + 1 < 2 * BLOCKS ? P.w_trunk + ((size_t)(L + 1) * 4 + wave) * kFragsPerConv : P.w_head + (size_t)head_tile * kFragsPerConv;
        load_frags(next, lane, wn);
        const bool second = (L & 1) != 0;
        conv64(second ? S.h : S.x, lane, w, acc);
        store_act(acc, P.bias + kBiasTrunk + L * F, n0, lane, second ? S.x : nullptr, second ? S.x : S.h);
#pragma unroll
        for (int i = 0; i < 18; ++i) w[i] = wn[i];
        group_barrier();
    }

    // ---- head convs: ReLU(conv + bias) in fp32 to head[board][c * 9 + p] -----------------------------------------------------------------
    if (wave < 3) {
        conv64(S.x, lane, w, acc);
        const int c0 = (lane >> 4) * 4;                              // channel within the tile
        const float* bias = P.bias + (wave < 2 ? kBiasPolicy + wave * 16 : kBiasValue);
        const float4 bv = *(const float4*)(bias + c0);
        const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
        float* out = S.head + (lane & 15) * kHeadFloats + (wave < 2 ? wave * 16 : 32) * 9;
#pragma unroll
        for (int p = 0; p < 9; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = acc[p][i] + bb[i];
                if (wave < 2 || c0 + i < VH) out[(c0 + i) * 9 + p] = v > 0.f ? v : 0.f;
            }
    }
    group_barrier();

    // ---- policy FC: thread (board, action), k = 0 .. 287 in order -----------------------------------------------------------------------
    if (tid < kB * 9) {
        const int b = tid / 9, a = tid % 9;
        const float* h = S.head + b * kHeadFloats;
        const float* wr = P.pfc_w + a * (PH * HW);
        float s = P.pfc_b[a];
#pragma unroll 8
        for (int k = 0; k < PH * HW; ++k) s += h[k] * wr[k];
        S.logit[tid] = s;
    }
    group_barrier();
    // ---- softmax and value: one thread per board --------------------------------------------------------------------------------------
    if (tid < kB) {
        float e[9], mx = -INFINITY, sum = 0.f;
#pragma unroll
        for (int a = 0; a < 9; ++a) { e[a] = S.logit[tid * 9 + a]; mx = e[a] > mx ? e[a] : mx; }
#pragma unroll
        for (int a = 0; a < 9; ++a) { e[a] = expf(e[a] - mx); sum += e[a]; }
#pragma unroll
        for (int a = 0; a < 9; ++a) policy[a] = e[a] / sum;
        const float* h = S.head + tid * kHeadFloats + PH * HW;
        float s = P.vfc_b[0];
#pragma unroll
        for (int k = 0; k < VH * HW; ++k) s += h[k] * P.vfc_w[k];
        value = tanhf(s);
    }
}

}  // namespace ttt
}  // namespace diee
