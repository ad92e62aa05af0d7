// ttt_device.h -- the tic-tac-toe network on the device (option "nn" = "device" of a tic-tac-toe ctx): the 64-filter 4-block ResNet of
// ttt_host.h evaluated by ONE launch of k_ttt_net (ttt_kernels.hip) per Engine::forward.  The search stays on the host and calls forward as
// before.  Nothing here is touched, and no HIP call is made, until the option is set.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/diee.h"
#include "ttt_host.h"

namespace diee {
namespace ttt {

// The packed network, resident on the device.  Convolutions are bf16 A-operand fragments of v_mfma_f32_16x16x32_bf16 in the order the
// kernel streams them, [conv][N-tile of 16 output channels][k-step][lane][8]: lane l, element e holds w[o = 16 * tile + (l & 15)][k], k =
// 32 * step + 8 * (l >> 4) + e.  For the 64-channel convs k = 64 * tap + c (step = 2 * tap + c / 32); for the initial conv k = 3 * tap + c
// padded from 27 to one step of 32.  Biases and both FCs stay fp32.
struct NetParams {
    const uint4* w_init;      // [4][1][64]
    const uint4* w_trunk;     // [8 convs: block 0 conv 1, block 0 conv 2, ...][4][18][64]
    const uint4* w_head;      // [3 tiles: policy 0 .. 15, policy 16 .. 31, value 0 .. 2 padded to 16][18][64]
    const float* bias;        // init 64 | trunk 8 x 64 | policy 32 | value 16 (3 used)
    const float* pfc_w;       // [9][288]
    const float* pfc_b;       // [9]
    const float* vfc_w;       // [27]
    const float* vfc_b;       // [1]
};
constexpr int kBiasInit = 0, kBiasTrunk = 64, kBiasPolicy = 64 + 8 * 64, kBiasValue = kBiasPolicy + 32, kBiasCount = kBiasValue + 16;
constexpr int kBoardsPerGroup = 16;                  // B: boards of one workgroup of k_ttt_net

// ttt_kernels.hip: policy [n][9] softmax, value [n] tanh; ceil(n / B) workgroups, no workgroup waits for another
void launch_ttt_net(hipStream_t st, const NetParams& P, const diee_ttt_state* states, uint32_t n, float* policy, float* value);

class DeviceNet {
public:
    explicit DeviceNet(int device);                  // EngineError(DIEE_ERR_HIP) if `device` is no usable GPU
    ~DeviceNet();
    DeviceNet(const DeviceNet&) = delete;
    DeviceNet& operator=(const DeviceNet&) = delete;
    // rounds the folded convolutions to bf16 (nearest even), packs and uploads them
    void upload(const Conv& init, const Conv* c1, const Conv* c2, const Conv& pconv, const Conv& vconv, const std::vector<float>& pfc_w,
                const std::vector<float>& pfc_b, const std::vector<float>& vfc_w, const std::vector<float>& vfc_b);
    void forward(const diee_ttt_state* s, uint32_t n, float* policy, float* value);     // synchronous
    // what the device search (ttt_search_device.h) shares with the network: the ctx's one stream and the packed weights
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }
    const NetParams& params() const { return params_; }
    bool ready() const { return weights_ != nullptr; }

private:
    void reserve(uint32_t n);
    int device_;
    hipStream_t stream_ = nullptr;
    void* weights_ = nullptr;                        // one allocation holding everything NetParams points at
    NetParams params_{};
    void *d_in_ = nullptr, *d_out_ = nullptr, *h_in_ = nullptr, *h_out_ = nullptr;     // states | policy, value; h_*: page-locked staging
    uint32_t cap_ = 0;
};

}  // namespace ttt
}  // namespace diee
