// The prior kernel of the GN step (prior.hpp): one thread per prior, pose priors first and landmark
// priors after them. Memory-bound and tiny: a thread loads its record in whole vectors (consecutive
// threads read consecutive records), gathers its node's state from the caches the J+H build reads,
// forms A and g in T (host/prior.hpp) and does a plain read-add-write on the node's diagonal block
// and b segment, which the J+H launch before it on the stream has just written.
#include "prior.hpp"

#include "../host/prior.hpp"

namespace bos {
namespace dev {

namespace {

template <typename T> struct alignas(4 * sizeof(T)) P4 { T x, y, z, w; };
template <typename T> struct alignas(2 * sizeof(T)) P2 { T x, y; };

template <typename T> __global__ __launch_bounds__(kPriorBlock) void prior_kernel(const PriorParams<T> P) {
    __shared__ double sh[kPriorBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kPriorBlock + threadIdx.x;
    double rho = 0.0;
    if (t < P.n_pose) {
        const int p = P.idx[t];
        const P4<T>* r = reinterpret_cast<const P4<T>*>(P.pose_rec + (int64_t)kPriorPoseRec * t);
        const P4<T> r0 = r[0], r1 = r[1], r2 = r[2];
        const int64_t o = 6 * (int64_t)p;
        if (p >= 0 && p < P.NP && o + 5 < P.nval) {
            const P2<T> xy = *reinterpret_cast<const P2<T>*>(P.pc + 4 * (int64_t)p);
            const T th = P.pth[p];
            const T m[3] = {r0.x, r0.y, r0.z};
            const T u[6] = {r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
            T A[6], g[3];
            rho = (double)bos::prior_pose_terms<T>(xy.x, xy.y, th, m, u, A, g);
            T* h = P.hval + o;
            T* b = P.b + 3 * (int64_t)p;
#pragma unroll
            for (int v = 0; v < 6; ++v) h[v] = h[v] + A[v];
#pragma unroll
            for (int v = 0; v < 3; ++v) b[v] = b[v] + g[v];
        }
    } else if (t < (int64_t)P.n_pose + P.n_lm) {
        const int64_t k = t - P.n_pose;
        const int l = P.idx[t];
        const P2<T>* r = reinterpret_cast<const P2<T>*>(P.lm_rec + (int64_t)kPriorLmRec * k);
        const P2<T> r0 = r[0], r1 = r[1], r2 = r[2];
        const int64_t o = P.off_ldiag + 3 * (int64_t)l;
        if (l >= 0 && l < P.NL && o + 2 < P.nval) {
            const P2<T> xy = *reinterpret_cast<const P2<T>*>(P.lc + 2 * (int64_t)l);
            const T m[2] = {r0.x, r0.y};
            const T u[3] = {r1.x, r1.y, r2.x};
            T A[3], g[2];
            rho = (double)bos::prior_landmark_terms<T>(xy.x, xy.y, m, u, A, g);
            T* h = P.hval + o;
            T* b = P.b + 3 * (int64_t)P.NP + 2 * (int64_t)l;
#pragma unroll
            for (int v = 0; v < 3; ++v) h[v] = h[v] + A[v];
            b[0] = b[0] + g[0];
            b[1] = b[1] + g[1];
        }
    }
    // the workgroup's sum of rho in a fixed order: butterfly inside a wave, then the waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rho += __shfl_xor(rho, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = rho;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0;
        for (int w = 0; w < kPriorBlock / 64; ++w) c += sh[w];
        P.part[blockIdx.x] = c;
    }
}

}  // namespace

template <typename T> hipError_t launch_priors(const PriorParams<T>& p, hipStream_t s) {
    const int64_t n = (int64_t)p.n_pose + p.n_lm;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((prior_kernel<T>), dim3((unsigned)prior_parts(n)), dim3(kPriorBlock), 0, s, p);
    return hipGetLastError();
}

template hipError_t launch_priors<double>(const PriorParams<double>&, hipStream_t);
template hipError_t launch_priors<float>(const PriorParams<float>&, hipStream_t);

}  // namespace dev
}  // namespace bos
