// ttt_device.cpp -- host side of the tic-tac-toe device network (ttt_device.h): packing, buffers, one stream, the launch.
#include "ttt_device.h"

#include <cstring>
#include <string>

#include "engine.h"
#include "ttt_host.h"

namespace diee {
namespace ttt {

namespace {
uint16_t bf16_rne(float f) {                         // what the kernel's own conversion does: round to nearest even, NaN stays NaN
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
constexpr size_t kFrag = 64 * 8;                     // bf16 of one fragment: 64 lanes x 8
// tiles x steps fragments of a 3x3 conv over 64 channels (cin == F) or of the initial conv (cin == CIN, one padded step)
void pack_conv(const Conv& c, int tiles, uint16_t* out) {
    const int steps = c.cin == F ? 18 : 1;
    for (int tile = 0; tile < tiles; ++tile)
        for (int step = 0; step < steps; ++step)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int o = 16 * tile + (l & 15), k = 32 * step + 8 * (l >> 4) + e;
                    const int tap = c.cin == F ? k / F : k / CIN, ch = c.cin == F ? k % F : k % CIN;
                    const bool live = o < c.cout && tap < 9;             // padded output channels and padded k are zero
                    out[((size_t)(tile * steps + step) * 64 + l) * 8 + e] = live ? bf16_rne(c.w[((size_t)o * c.cin + ch) * 9 + tap]) : (uint16_t)0;
                }
}
}  // namespace

DeviceNet::DeviceNet(int device) : device_(device) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        throw EngineError(DIEE_ERR_HIP, "option nn = device: no usable GPU " + std::to_string(device) +
                                            (e != hipSuccess ? std::string(" (") + hipGetErrorString(e) + ")" : std::string()));
    }
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
}

DeviceNet::~DeviceNet() {
    if (hipSetDevice(device_) != hipSuccess) return;
    if (stream_) { (void)hipStreamSynchronize(stream_); (void)hipStreamDestroy(stream_); }
    if (weights_) (void)hipFree(weights_);
    if (d_in_) (void)hipFree(d_in_);
    if (d_out_) (void)hipFree(d_out_);
    if (h_in_) (void)hipHostFree(h_in_);
    if (h_out_) (void)hipHostFree(h_out_);
}

void DeviceNet::upload(const Conv& init, const Conv* c1, const Conv* c2, const Conv& pconv, const Conv& vconv, const std::vector<float>& pfc_w,
                       const std::vector<float>& pfc_b, const std::vector<float>& vfc_w, const std::vector<float>& vfc_b) {
    constexpr size_t nInit = 4 * kFrag, nTrunk = 2 * BLOCKS * 4 * 18 * kFrag, nHead = 3 * 18 * kFrag, nBf = nInit + nTrunk + nHead;
    constexpr size_t nPfw = (size_t)A * PH * HW, nVfw = (size_t)VH * HW, nF32 = kBiasCount + nPfw + A + nVfw + 1;
    std::vector<unsigned char> img(nBf * 2 + nF32 * 4, 0);               // (nBf * 2 is a multiple of 16: the floats stay aligned)
    uint16_t* bf = (uint16_t*)img.data();
    pack_conv(init, 4, bf);
    for (int b = 0; b < BLOCKS; ++b) {
        pack_conv(c1[b], 4, bf + nInit + (size_t)(2 * b) * 4 * 18 * kFrag);
        pack_conv(c2[b], 4, bf + nInit + (size_t)(2 * b + 1) * 4 * 18 * kFrag);
    }
    pack_conv(pconv, 2, bf + nInit + nTrunk);
    pack_conv(vconv, 1, bf + nInit + nTrunk + 2 * 18 * kFrag);
    float* f = (float*)(img.data() + nBf * 2);
    memcpy(f + kBiasInit, init.b.data(), F * sizeof(float));
    for (int b = 0; b < BLOCKS; ++b) {
        memcpy(f + kBiasTrunk + (2 * b) * F, c1[b].b.data(), F * sizeof(float));
        memcpy(f + kBiasTrunk + (2 * b + 1) * F, c2[b].b.data(), F * sizeof(float));
    }
    memcpy(f + kBiasPolicy, pconv.b.data(), PH * sizeof(float));
    memcpy(f + kBiasValue, vconv.b.data(), VH * sizeof(float));
    memcpy(f + kBiasCount, pfc_w.data(), nPfw * sizeof(float));
    memcpy(f + kBiasCount + nPfw, pfc_b.data(), A * sizeof(float));
    memcpy(f + kBiasCount + nPfw + A, vfc_w.data(), nVfw * sizeof(float));
    f[kBiasCount + nPfw + A + nVfw] = vfc_b[0];

    HIPCHK(hipSetDevice(device_));
    if (!weights_) HIPCHK(hipMalloc(&weights_, img.size()));
    HIPCHK(hipStreamSynchronize(stream_));
    HIPCHK(hipMemcpy(weights_, img.data(), img.size(), hipMemcpyHostToDevice));
    const uint4* w = (const uint4*)weights_;
    const float* df = (const float*)((const unsigned char*)weights_ + nBf * 2);
    params_.w_init = w;
    params_.w_trunk = w + nInit / 8;
    params_.w_head = w + (nInit + nTrunk) / 8;
    params_.bias = df;
    params_.pfc_w = df + kBiasCount;
    params_.pfc_b = df + kBiasCount + nPfw;
    params_.vfc_w = df + kBiasCount + nPfw + A;
    params_.vfc_b = df + kBiasCount + nPfw + A + nVfw;
}

void DeviceNet::reserve(uint32_t n) {
    if (n <= cap_) return;
    uint32_t cap = cap_ ? cap_ : 1024;
    while (cap < n) cap = cap > 0x7FFFFFFFu ? n : cap * 2;
    HIPCHK(hipStreamSynchronize(stream_));
    if (d_in_) { (void)hipFree(d_in_); d_in_ = nullptr; }
    if (d_out_) { (void)hipFree(d_out_); d_out_ = nullptr; }
    if (h_in_) { (void)hipHostFree(h_in_); h_in_ = nullptr; }
    if (h_out_) { (void)hipHostFree(h_out_); h_out_ = nullptr; }
    cap_ = 0;
    const size_t in = (size_t)cap * sizeof(diee_ttt_state), out = (size_t)cap * (A + 1) * sizeof(float);
    HIPCHK(hipMalloc(&d_in_, in));
    HIPCHK(hipMalloc(&d_out_, out));
    HIPCHK(hipHostMalloc(&h_in_, in));
    HIPCHK(hipHostMalloc(&h_out_, out));
    cap_ = cap;
}

void DeviceNet::forward(const diee_ttt_state* s, uint32_t n, float* policy, float* value) {
    if (n == 0) return;
    if (!weights_) throw EngineError(DIEE_ERR_NO_WEIGHTS, "diee_load_weights has not been called");
    HIPCHK(hipSetDevice(device_));
    reserve(n);
    const size_t in = (size_t)n * sizeof(diee_ttt_state), np = (size_t)n * A;
    memcpy(h_in_, s, in);
    HIPCHK(hipMemcpyAsync(d_in_, h_in_, in, hipMemcpyHostToDevice, stream_));
    float* d_policy = (float*)d_out_;
    float* d_value = d_policy + np;
    launch_ttt_net(stream_, params_, (const diee_ttt_state*)d_in_, n, d_policy, d_value);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out_, d_out_, (np + n) * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    memcpy(policy, h_out_, np * sizeof(float));
    memcpy(value, (const float*)h_out_ + np, (size_t)n * sizeof(float));
}

}  // namespace ttt
}  // namespace diee
