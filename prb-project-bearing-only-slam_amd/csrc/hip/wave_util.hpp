// Wavefront helpers shared by the solver's kernels (mf_*.hpp) and the covariance kernels
// (pair_cov.hip, node_cov.hip): lane broadcast, wave-level synchronisation, global -> LDS staging.
#pragma once

#include <hip/hip_runtime.h>

namespace bos {
namespace dev {

// lane l's double, broadcast to the wave (l uniform)
__device__ __forceinline__ double readlane_d(double x, int l) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Copy n doubles global -> LDS by one wavefront, 8 independent loads in flight per lane
// (NTL: non-temporal loads, the L panel policy of mf_device.hpp LD_L).
template <int U = 8, bool NTL = false> __device__ __forceinline__ void stage_lds(double* dst, const double* src, int n, int lane) {
    for (int e0 = 0; e0 < n; e0 += 64 * U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + 64 * u + lane;
            v[u] = e < n ? (NTL ? __builtin_nontemporal_load(src + e) : src[e]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + 64 * u + lane;
            if (e < n) dst[e] = v[u];
        }
    }
}

}  // namespace dev
}  // namespace bos
