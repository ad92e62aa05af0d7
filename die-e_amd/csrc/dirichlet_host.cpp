// dirichlet_host.cpp -- the host Dirichlet sampler of the root noise (noise.rs:27-34), for both games.
#include <cmath>
#include <vector>

#include "bg_device.h"
#include "search_host.h"

namespace diee {

namespace {

// Dirichlet(alpha * 1_n): Gamma(alpha,1) draws normalised, as rand_distr 0.4.3 does (Cargo.toml:19,
// call site noise.rs:29-30): shape < 1 via Gamma(shape+1) * U^(1/shape), shape >= 1 by
// Marsaglia-Tsang; normals by Box-Muller.  Drawn on the HOST (like the reference) from Philox.
struct DirRng {
    uint64_t seed; uint32_t step; uint32_t n;
    double u01() {
        uint32_t o[4];
        philox4x32((uint32_t)seed, (uint32_t)(seed >> 32), n++, step, kTagDirichlet, 0u, o);
        const uint64_t x = ((uint64_t)o[1] << 32) | o[0];
        return ((double)(x >> 12) + 0.5) * (1.0 / 4503599627370496.0);
    }
    double normal() {
        const double u1 = u01(), u2 = u01();
        return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
    }
    double gamma_large(double shape) {
        const double d = shape - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * d);
        for (;;) {
            const double x = normal(), vc = 1.0 + c * x;
            if (vc <= 0.0) continue;
            const double v = vc * vc * vc, u = u01(), x2 = x * x;
            if (u < 1.0 - 0.0331 * x2 * x2 || std::log(u) < 0.5 * x2 + d * (1.0 - v + std::log(v))) return d * v;
        }
    }
};

}  // namespace

void dirichlet_host(uint64_t seed, uint32_t step, float alpha, int n, float* out) {
    DirRng r{seed, step, 0};
    const double a = (double)alpha;
    std::vector<double> g((size_t)n);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        double v;
        if (a < 1.0) { const double u = r.u01(); v = r.gamma_large(a + 1.0) * std::pow(u, 1.0 / a); }
        else v = r.gamma_large(a);
        g[(size_t)i] = v; sum += v;
    }
    for (int i = 0; i < n; ++i) out[i] = (float)(g[(size_t)i] / sum);
}

}  // namespace diee
