// Kernels of bos_cost / bos_optimize (lm.hpp). All of them are short streaming passes next to the
// factorization they surround; none waits for another workgroup.
#include "lm.hpp"

#include <algorithm>

#include "../host/bos_math.hpp"
#include "../host/prior.hpp"
#include "kernels.hpp"

namespace bos {
namespace dev {

namespace {

__device__ __forceinline__ double lm_nan_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

// Sum over the workgroup in a fixed order (butterfly inside a wave, the waves in order): every
// thread must call it; thread 0 gets the sum. sh: kLmBlock / 64 doubles, reusable after the call.
template <int BLOCK = kLmBlock> __device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < BLOCK / 64; ++w) t += sh[w];
    __syncthreads();
    return t;
}

template <int BLOCK = kLmBlock> __device__ __forceinline__ double block_max(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = lm_nan_max(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < BLOCK / 64; ++w) t = lm_nan_max(t, sh[w]);
    __syncthreads();
    return t;
}

__device__ __forceinline__ void copy_words(const CopySet& C) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        uint32_t* d = C.dst[a];
        const uint32_t* s = C.src[a];
        for (int64_t i = t; i < C.words[a]; i += stride) d[i] = s[i];
    }
}

// rho of edge i (bearings, then odometry edges); false for a self-loop or an index outside the state
__device__ __forceinline__ bool edge_rho(const CostParams& P, int64_t i, double& rho) {
    if (i < P.Mb) {
        const int p = P.b_pose[i], l = P.b_lm[i];
        if (p < 0 || p >= P.NP || l < 0 || l >= P.NL) return false;
        const double th = P.pose[3 * (int64_t)p + 2];
        double gx, gy;
        const double e = bos::bearing_error<double>(P.pose[3 * (int64_t)p], P.pose[3 * (int64_t)p + 1], cos(th), sin(th),
                                                    P.lm[2 * (int64_t)l], P.lm[2 * (int64_t)l + 1], P.b_z[i], gx, gy);
        const double w = P.b_w ? P.b_w[i] : 1.0;
        rho = e * w * e;
        return true;
    }
    const int64_t k = i - P.Mb;
    const int a = P.o_src[k], d = P.o_dst[k];
    if (a == d || a < 0 || a >= P.NP || d < 0 || d >= P.NP) return false;
    const double* xs = P.pose + 3 * (int64_t)a;
    const double* xd = P.pose + 3 * (int64_t)d;
    const double* z = P.o_z + 3 * k;
    const double* u = P.o_om + 6 * k;
    double e[3], J[18];
    bos::odometry_error_jacobian<double>(xs[0], xs[1], xs[2], cos(xs[2]), sin(xs[2]), xd[0], xd[1], xd[2], z[0], z[1], z[2], e,
                                         J);
    const double Oe0 = u[0] * e[0] + u[1] * e[1] + u[2] * e[2];
    const double Oe1 = u[1] * e[0] + u[3] * e[1] + u[4] * e[2];
    const double Oe2 = u[2] * e[0] + u[4] * e[1] + u[5] * e[2];
    rho = e[0] * Oe0 + e[1] * Oe1 + e[2] * Oe2;
    return true;
}

// rho of prior k (pose priors, then landmark priors) at the master state; false for a node outside the state
__device__ __forceinline__ bool prior_rho(const CostParams& P, int64_t k, double& rho) {
    const int node = P.pr_idx[k];
    if (k < P.n_pose_priors) {
        if (node < 0 || node >= P.NP) return false;
        const double* x = P.pose + 3 * (int64_t)node;
        const double* r = P.pr_pose + 9 * k;
        rho = bos::prior_pose_rho<double>(x[0], x[1], x[2], r, r + 3);
        return true;
    }
    if (node < 0 || node >= P.NL) return false;
    const double* l = P.lm + 2 * (int64_t)node;
    const double* r = P.pr_lm + 5 * (k - P.n_pose_priors);
    rho = bos::prior_landmark_rho<double>(l[0], l[1], r, r + 2);
    return true;
}

__global__ __launch_bounds__(kLmBlock) void lm_cost_kernel(const CostParams P) {
    __shared__ double sh[kLmBlock / 64];
    const int64_t edges = (int64_t)P.Mb + P.Mo, total = edges + P.n_pose_priors + P.n_lm_priors;
    const int64_t stride = (int64_t)gridDim.x * kLmBlock;
    double f = 0.0, chi = 0.0, nr = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLmBlock + threadIdx.x; i < total; i += stride) {
        double rho;
        if (i >= edges) {   // a prior: h(rho) = rho
            if (!prior_rho(P, i - edges, rho)) continue;
            f += rho;
            chi += rho;
            continue;
        }
        if (!edge_rho(P, i, rho)) continue;
        const bool rob = rho > P.kt;
        f += bos::lm_huber(rho, P.kt, rob ? sqrt(P.kt * rho) : 0.0);
        chi += rho;
        nr += rob ? 1.0 : 0.0;
    }
    f = block_sum(f, sh);
    chi = block_sum(chi, sh);
    nr = block_sum(nr, sh);
    if (threadIdx.x == 0 && (int)blockIdx.x < P.n_parts) {
        P.part_F[blockIdx.x] = f;
        P.part_chi[blockIdx.x] = chi;
        P.part_nrob[blockIdx.x] = (int32_t)nr;
    }
}

template <typename T>
__global__ __launch_bounds__(kLmBlock) void lm_damping_kernel(T* hval, int64_t nval, int64_t off_ldiag,
                                                              const int32_t* lane_pose, int n_groups, int NP,
                                                              const int32_t* lane_lm, int n_lm_lanes, int NL,
                                                              const LmControl* ctl, const CopySet backup) {
    copy_words(backup);
    const int64_t i = (int64_t)blockIdx.x * kLmBlock + threadIdx.x;
    const T lam = (T)ctl->st.lambda;
    if (i < n_groups) {
        const int p = lane_pose ? lane_pose[i] : (int)i;
        const int64_t o = 6 * (int64_t)p;
        if (p >= 0 && p < NP && o + 5 < nval) {
            hval[o] += lam;
            hval[o + 2] += lam;
            hval[o + 5] += lam;
        }
    } else if (i < (int64_t)n_groups + n_lm_lanes) {
        const int l = lane_lm[i - n_groups];
        const int64_t o = off_ldiag + 3 * (int64_t)l;
        if (l >= 0 && l < NL && o + 2 < nval) {
            hval[o] += lam;
            hval[o + 2] += lam;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kLmBlock) void lm_model_kernel(const double* x, const T* b, const int32_t* elim_ref, int64_t n,
                                                            int64_t nb, double* part_xx, double* part_xb) {
    __shared__ double sh[kLmBlock / 64];
    const int64_t stride = (int64_t)gridDim.x * kLmBlock;
    double xx = 0.0, xb = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLmBlock + threadIdx.x; i < n; i += stride) {
        const int32_t r = elim_ref[i];
        const double v = x[i];
        xx += v * v;
        if (r >= 0 && r < nb) xb += v * (double)b[r];
    }
    xx = block_sum(xx, sh);
    xb = block_sum(xb, sh);
    if (threadIdx.x == 0) {
        part_xx[blockIdx.x] = xx;
        part_xb[blockIdx.x] = xb;
    }
}

__global__ __launch_bounds__(kLmBlock) void lm_copy_kernel(const CopySet C, const LmControl* flag) {
    if (flag && flag->restore != 1) return;
    copy_words(C);
}

__global__ __launch_bounds__(kLmDecideBlock) void lm_decide_kernel(const DecideParams P) {
    constexpr int B = kLmDecideBlock;
    __shared__ double sh[B / 64];
    double f = 0.0, c = 0.0, r = 0.0, xx = 0.0, xb = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < P.n_cost; i += B) {
        f += P.part_F[i];
        c += P.part_chi[i];
        r += (double)P.part_nrob[i];
    }
    if (P.mode == 0) {
        for (int i = threadIdx.x; i < P.n_model; i += B) {
            xx += P.part_xx[i];
            xb += P.part_xb[i];
        }
        for (int i = threadIdx.x; i < P.n_max; i += B) m = lm_nan_max(m, P.max_part[i]);
    }
    f = block_sum<B>(f, sh);
    c = block_sum<B>(c, sh);
    r = block_sum<B>(r, sh);
    xx = block_sum<B>(xx, sh);
    xb = block_sum<B>(xb, sh);
    m = block_max<B>(m, sh);
    if (threadIdx.x != 0) return;
    LmControl* ctl = P.ctl;
    const double F = f + P.F_const;
    ctl->cost_eval = F;
    ctl->chi2 = c + P.chi_const;
    ctl->n_robust = (int32_t)r + P.nrob_const;
    if (P.mode == 1) ctl->st.cost = ctl->cost_start = F;
    if (P.mode == 0) {
        const int32_t inf = P.info ? *P.info : 0;
        if (P.info) *P.info = 0;
        if ((inf & kStepAbort) && !ctl->st.done) {   // no solution, no update: freeze, the host fails the call
            ctl->aborted = 1;
            ctl->st.done = 1;
            ctl->restore = 1;
        } else {
            const double lam = P.lambda_fp32 ? (double)(float)ctl->st.lambda : ctl->st.lambda;
            const double pred = lam * xx + xb;
            bos_lm_iteration rec;
            const int32_t slot = ctl->st.iteration;
            const bool counted = bos::lm_rule_apply(ctl->st, ctl->opt, F, pred, m, inf & ~kStepAbort, &rec);
            ctl->restore = rec.accepted ? 0 : 1;
            if (counted && P.trace && slot >= 0 && slot < ctl->trace_cap) P.trace[slot] = rec;
        }
    }
    ctl->seq += 1;
    if (P.mirror) {   // the summary, then (after a system-scope release) its sequence number
        LmControl* mr = P.mirror;
        mr->st = ctl->st;
        mr->cost_eval = ctl->cost_eval;
        mr->chi2 = ctl->chi2;
        mr->cost_start = ctl->cost_start;
        mr->n_robust = ctl->n_robust;
        mr->restore = ctl->restore;
        mr->aborted = ctl->aborted;
        __threadfence_system();
        __hip_atomic_store(&mr->seq, ctl->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

hipError_t launch_lm_cost(const CostParams& p, hipStream_t s) {
    if (p.n_parts <= 0) return hipSuccess;
    hipLaunchKernelGGL(lm_cost_kernel, dim3(p.n_parts), dim3(kLmBlock), 0, s, p);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_lm_damping(T* hval, int64_t nval, int64_t off_ldiag, const int32_t* lane_pose, int n_groups, int NP,
                             const int32_t* lane_lm, int n_lm_lanes, int NL, const LmControl* ctl, const CopySet& backup,
                             hipStream_t s) {
    const int64_t n = std::max<int64_t>((int64_t)n_groups + n_lm_lanes, 1);
    hipLaunchKernelGGL((lm_damping_kernel<T>), dim3((unsigned)((n + kLmBlock - 1) / kLmBlock)), dim3(kLmBlock), 0, s, hval,
                       nval, off_ldiag, lane_pose, n_groups, NP, lane_lm, n_lm_lanes, NL, ctl, backup);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_lm_model(const double* x, const T* b, const int32_t* elim_ref, int64_t n, int64_t nb, double* part_xx,
                           double* part_xb, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((lm_model_kernel<T>), dim3((unsigned)lm_model_parts(n)), dim3(kLmBlock), 0, s, x, b, elim_ref, n, nb,
                       part_xx, part_xb);
    return hipGetLastError();
}

hipError_t launch_lm_copy(const CopySet& c, const LmControl* flag, hipStream_t s) {
    int64_t most = 0;
    for (int a = 0; a < 5; ++a) most = most > c.words[a] ? most : c.words[a];
    if (most <= 0) return hipSuccess;
    int64_t blocks = (most + kLmBlock - 1) / kLmBlock;
    if (blocks > 4096) blocks = 4096;   // grid-stride beyond
    hipLaunchKernelGGL(lm_copy_kernel, dim3((unsigned)blocks), dim3(kLmBlock), 0, s, c, flag);
    return hipGetLastError();
}

hipError_t launch_lm_decide(const DecideParams& p, hipStream_t s) {
    hipLaunchKernelGGL(lm_decide_kernel, dim3(1), dim3(kLmDecideBlock), 0, s, p);
    return hipGetLastError();
}

template hipError_t launch_lm_damping<double>(double*, int64_t, int64_t, const int32_t*, int, int, const int32_t*, int, int,
                                              const LmControl*, const CopySet&, hipStream_t);
template hipError_t launch_lm_damping<float>(float*, int64_t, int64_t, const int32_t*, int, int, const int32_t*, int, int,
                                             const LmControl*, const CopySet&, hipStream_t);
template hipError_t launch_lm_model<double>(const double*, const double*, const int32_t*, int64_t, int64_t, double*, double*,
                                            hipStream_t);
template hipError_t launch_lm_model<float>(const double*, const float*, const int32_t*, int64_t, int64_t, double*, double*,
                                           hipStream_t);

}  // namespace dev
}  // namespace bos
