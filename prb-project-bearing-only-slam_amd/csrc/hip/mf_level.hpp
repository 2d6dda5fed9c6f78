// The level fallback kernels: one 256-thread workgroup per front of any size, the front in LDS (up to
// kLdsCapM rows) or in global scratch. They take the fronts above kMfBlkMaxM rows (fallback plans),
// the blocked class when mf_factor_blk cannot get its LDS, and every workgroup front's backward step.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mf_device.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

constexpr int kLdsCapM = 90;   // larger fronts up to 90 x 90 doubles (64.8 KB) are factored in LDS

__global__ __launch_bounds__(kMfBlock) void mf_factor_level(const MfArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int s = a.level[blockIdx.x];
    const int k = a.k[s], r = a.r[s], m = k + r;
    const int tid = threadIdx.x;
    const int64_t so = a.scratch_off[s];
    double* F = so < 0 ? lds : a.scratch + so;
    const int64_t mm = (int64_t)m * m;
    for (int64_t e = tid; e < mm; e += kMfBlock) F[e] = 0.0;
    __syncthreads();
    // scatter H entries (each front position receives at most one entry)
    for (int q = a.amap_ptr[s] + tid; q < a.amap_ptr[s + 1]; q += kMfBlock) F[a.amap_dst[q]] = a.A[a.amap_src[q]];
    __syncthreads();
    // extend-add children's update matrices, one child at a time (lower triangle)
    for (int ci = a.child_ptr[s]; ci < a.child_ptr[s + 1]; ++ci) {
        const int c = a.child[ci];
        const int rc = a.r[c];
        const int32_t* map = a.rmap + a.rmap_off[c];
        const double* Uc = a.U + a.U_off[c];
        for (int j = tid >> 6; j < rc; j += kMfBlock / 64) {
            const int64_t pj = (int64_t)map[j] * m;
            const double* uj = Uc + pk(j, j, rc) - j;
            for (int i = j + (tid & 63); i < rc; i += 64) F[map[i] + pj] += uj[i];
        }
        __syncthreads();
    }
    // right-looking partial Cholesky of the first k columns
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = 0; j < k; ++j) {
        double d = F[j + (int64_t)j * m];
        if (!(d > 0.0)) {
            if (tid == 0) atomicAdd(a.info, 1);
            d = 1e-300;
        }
        const double ljj = sqrt(d);
        const double inv = 1.0 / ljj;
        __syncthreads();
        if (tid == 0) F[j + (int64_t)j * m] = ljj;
        for (int i = j + 1 + tid; i < m; i += kMfBlock) F[i + (int64_t)j * m] *= inv;
        __syncthreads();
        for (int l = j + 1 + wave; l < m; l += kMfBlock / 64) {
            const double flj = F[l + (int64_t)j * m];
            double* col = F + (int64_t)l * m;
            const double* cj = F + (int64_t)j * m;
            for (int i = l + lane; i < m; i += 64) col[i] -= cj[i] * flj;
        }
        __syncthreads();
    }
    // write the L panel (m x k) and the update matrix (r x r)
    double* Ls = a.L + a.L_off[s];
    const int64_t nL = (int64_t)m * k;
    for (int64_t e = tid; e < nL; e += kMfBlock) Ls[e] = F[e];
    double* Us = a.U + a.U_off[s];
    for (int j = wave; j < r; j += kMfBlock / 64) {
        double* uj = Us + pk(j, j, r) - j;
        const double* fj = F + (k + (int64_t)(k + j) * m);
        for (int i = j + lane; i < r; i += 64) uj[i] = fj[i];
    }
}

// forward substitution L y = b for one level (bottom-up); x holds b on entry, y on exit for the
// supernode's own dofs; u receives the r-vector passed to the parent
__global__ __launch_bounds__(kMfBlock) void mf_forward_level(const MfArgs a) {
    extern __shared__ __attribute__((aligned(16))) double w[];
    const int s = a.level[blockIdx.x];
    const int k = a.k[s], r = a.r[s], m = k + r;
    const int tid = threadIdx.x;
    const int c0 = a.col0[s];
    for (int i = tid; i < m; i += kMfBlock) w[i] = i < k ? a.x[c0 + i] : 0.0;
    __syncthreads();
    for (int ci = a.child_ptr[s]; ci < a.child_ptr[s + 1]; ++ci) {
        const int c = a.child[ci];
        const int rc = a.r[c];
        const int32_t* map = a.rmap + a.rmap_off[c];
        const double* uc = a.u + a.u_off[c];
        for (int t = tid; t < rc; t += kMfBlock) w[map[t]] += uc[t];
        __syncthreads();
    }
    const double* Ls = a.L + a.L_off[s];
    for (int j = 0; j < k; ++j) {
        const double yj = w[j] / Ls[j + (int64_t)j * m];
        __syncthreads();
        if (tid == 0) w[j] = yj;
        for (int i = j + 1 + tid; i < m; i += kMfBlock) w[i] -= Ls[i + (int64_t)j * m] * yj;
        __syncthreads();
    }
    for (int i = tid; i < m; i += kMfBlock) {
        if (i < k) a.x[c0 + i] = w[i];
        else a.u[a.u_off[s] + (i - k)] = w[i];
    }
}

// backward substitution L^T x = y for one level (top-down): the rows below the supernode are
// ancestors' dofs whose solution is already final in x
__global__ __launch_bounds__(kMfBlock) void mf_backward_level(const MfArgs a) {
    extern __shared__ __attribute__((aligned(16))) double w[];   // [0,k): y / x,  [k,2k): t
    const int s = a.level[blockIdx.x];
    const int k = a.k[s], r = a.r[s], m = k + r;
    const int tid = threadIdx.x;
    const int c0 = a.col0[s];
    const double* Ls = a.L + a.L_off[s];
    const int32_t* fi = a.findex + a.findex_off[s];
    double* t = w + k;
    // t_j = sum_{i >= k} L[i, j] x[findex[i]]
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = wave; j < k; j += kMfBlock / 64) {
        double acc = 0.0;
        for (int i = k + lane; i < m; i += 64) acc += Ls[i + (int64_t)j * m] * a.x[fi[i]];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) t[j] = acc;
    }
    if (k <= 64) {
        // L11 staged in LDS (column i at stride k + 1) by all waves, then the triangular solve on
        // wave 0 alone, lane i holding t_i: no barrier and no global load in the sequential chain
        // (config 2's separators: k = 20-40, 16-21 us per launch with a barrier pair and a global
        // diagonal load per column). Same operations in the same order: bit-identical x.
        double* S = t + k;
        for (int e = tid; e < k * k; e += kMfBlock) {
            const int i = e / k, j = e - i * k;
            if (j >= i) S[j + i * (k + 1)] = Ls[j + (int64_t)i * m];
        }
        __syncthreads();
        if (wave) return;
        const bool on = lane < k;
        double ti = on ? t[lane] : 0.0;
        const double wi = on ? a.x[c0 + lane] : 0.0;
        const double di = on ? S[lane * (k + 2)] : 1.0;
        double xi = 0.0;
        for (int j = k - 1; j >= 0; --j) {
            const double xj = readlane_d(wi - ti, j) / readlane_d(di, j);
            if (lane == j) xi = xj;
            if (lane < j) ti += S[j + lane * (k + 1)] * xj;
        }
        if (on) {
            a.x[c0 + lane] = xi;
            if (a.xtag[s]) tag_pair(a.xg + 2 * (int64_t)(c0 + lane), xi, *a.epoch);
        }
        return;
    }
    for (int j = tid; j < k; j += kMfBlock) w[j] = a.x[c0 + j];
    __syncthreads();
    for (int j = k - 1; j >= 0; --j) {
        const double xj = (w[j] - t[j]) / Ls[j + (int64_t)j * m];
        __syncthreads();
        if (tid == 0) w[j] = xj;
        for (int i = tid; i < j; i += kMfBlock) t[i] += Ls[j + (int64_t)i * m] * xj;
        __syncthreads();
    }
    for (int j = tid; j < k; j += kMfBlock) a.x[c0 + j] = w[j];
    if (a.xtag[s]) {
        const uint32_t ep = *a.epoch;
        for (int j = tid; j < k; j += kMfBlock) tag_pair(a.xg + 2 * (int64_t)(c0 + j), w[j], ep);
    }
}

}  // namespace

}  // namespace dev
}  // namespace bos
