// The backward substitution's wave kernels: one wavefront per front (per level, or the backward flow
// over the tree's top) and the folded landmarks' launch. The workgroup fronts' per-level backward step is
// mf_level.hpp mf_backward_level.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mf_device.hpp"
#include "mf_flow.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

// Backward substitution of one front by one wavefront (any m); LDS: x_own[k] | t[k] | x_rows[r] |
// L panel (m x k). The rows below the supernode are ancestors' dofs, already final in x.
// The L panel and the front's own forward results do not depend on the ancestors, so the flow
// kernel stages them before it waits for the parent (FLOW: f and parent set).
constexpr int kBwdRegK = 32;   // fronts with k <= this solve their triangle from registers

template <int MODE>
__device__ __forceinline__ void backward_front(const MfArgs& a, int s, double* w, int lane, const Flow* f,
                                               const int32_t* parent) {
    constexpr bool COH = MODE == kModeFlow;
    const int k = a.k[s], r = a.r[s], m = k + r;
    const int c0 = a.col0[s];
    const int32_t* fi = a.findex + a.findex_off[s];
    double* t = w + k;
    double* xs = w + 2 * k;
    double* Lw = w + 2 * k + r;
    // where the first 64 rows' x live (static); clamped, branch-free reads (see assemble_wave)
    const int xi0 = fi[k + min(lane, max(r - 1, 0))];
    unsigned long long* const stp = f ? f->stamps : a.stamps_b;
    fstamp(stp, s, 0);
    if constexpr (MODE == kModeLevel) {
        // per-level launch: the parents' x are final (earlier launches), so the front's own
        // right-hand side and the first 64 rows' x are loaded beside the panel, all in flight at once
        const double y0v = a.x[c0 + min(lane, k - 1)], xr0v = a.x[xi0];
        const double y0 = lane < k ? y0v : 0.0;
        const double xr0 = lane < r ? xr0v : 0.0;
        stage_lds<16, true>(Lw, a.L + a.L_off[s], m * k, lane);
        if (lane < k) w[lane] = y0;
        for (int j = 64 + lane; j < k; j += 64) w[j] = a.x[c0 + j];
        fstamp(stp, s, 1);
        fstamp(stp, s, 2);
        if (lane < r) xs[lane] = xr0;
        for (int i = 64 + lane; i < r; i += 64) xs[i] = a.x[fi[k + i]];
    } else {
        stage_lds<8, true>(Lw, a.L + a.L_off[s], m * k, lane);
        for (int j = lane; j < k; j += 64) w[j] = a.x[c0 + j];
        fstamp(stp, s, 1);
        if (parent[s] >= 0 && f->fid[parent[s]] == f->id) {
            // the rows are dofs of ancestors, whose x every backward front publishes as tagged
            // granules (xg): one lane probes the parent's first dof, then the rows are swept until
            // every tag is this step's epoch (no completion flag)
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            probe_granule(a.xg + 2 * (int64_t)a.col0[parent[s]] + 1, f->epoch, t0, a.info);
            for (uint32_t it = 0;; ++it) {
                bool ok = true;
                const double v0 = untag_pair(a.xg + 2 * (int64_t)xi0, f->epoch, ok);
                if (lane < r) xs[lane] = v0;
                for (int i = 64 + lane; i < r; i += 64) xs[i] = untag_pair(a.xg + 2 * (int64_t)fi[k + i], f->epoch, ok);
                if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
                if ((it & 15) == 15) {
                    const bool stalled = (__hip_atomic_load(a.info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kStall) != 0;
                    if (stalled || __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) {
                        if (lane == 0) atomicOr(a.info, kStall);
                        break;
                    }
                }
                __builtin_amdgcn_s_sleep(1);
            }
        } else {   // the parent finished in an earlier launch (or none): final x
            if (lane < r) xs[lane] = ldc<COH>(a.x + xi0);
            for (int i = 64 + lane; i < r; i += 64) xs[i] = ldc<COH>(a.x + fi[k + i]);
        }
        fstamp(stp, s, 2);
    }
    wave_sync();
    if (k <= 64) {
        // lane j < k: t_j = sum_i L[k + i, j] x[fi[k + i]] in row order, then the triangular
        // solve in registers: x_j = (y_j - t_j) / L_jj broadcast from lane j, t_i += L[j, i] x_j
        const bool own = lane < k;
        double tj = 0.0;
        if (own)
            for (int i = 0; i < r; ++i) tj += Lw[k + i + lane * m] * xs[i];
        // 1 / L_jj by every lane at once, off the sequential chain below
        const double yv = own ? w[lane] : 0.0, rjj = own ? 1.0 / Lw[lane + lane * m] : 1.0;
        double xv = 0.0;
        // per-level launches only: in the backward flow the register form measured slower (solve +6 us,
        // profiles/r05_backward_flow_registers_ab.txt)
        if (MODE == kModeLevel && k <= kBwdRegK) {
            // the lane's column of the k x k block in registers, read from LDS before the chain, so
            // each step of the sequential chain is arithmetic and a lane read only
            double lr[kBwdRegK];
#pragma unroll
            for (int j = 0; j < kBwdRegK; ++j) lr[j] = own && j < k ? Lw[j + lane * m] : 0.0;
#pragma unroll
            for (int j = kBwdRegK - 1; j >= 0; --j) {
                if (j < k) {   // uniform
                    const double xj = readlane_d((yv - tj) * rjj, j);
                    if (lane == j) xv = xj;
                    else if (lane < j) tj += lr[j] * xj;
                }
            }
        } else {
            for (int j = k - 1; j >= 0; --j) {
                const double xj = readlane_d((yv - tj) * rjj, j);
                if (lane == j) xv = xj;
                else if (lane < j) tj += Lw[j + lane * m] * xj;
            }
        }
        if (own) stc<COH>(a.x + c0 + lane, xv);
        if (a.xtag[s] && own) tag_pair(a.xg + 2 * (int64_t)(c0 + lane), xv, *a.epoch);
        wave_sync();
        fstamp(stp, s, 3);
        return;
    }
    // t_j = sum_i L[k + i, j] x[fi[k + i]]: fixed-order wave reduction per column
    for (int j = 0; j < k; ++j) {
        double v = 0.0;
        for (int i = lane; i < r; i += 64) v += Lw[k + i + j * m] * xs[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) t[j] = v;
    }
    wave_sync();
    for (int j = k - 1; j >= 0; --j) {
        const double xj = (w[j] - t[j]) / Lw[j + j * m];
        wave_sync();
        if (lane == 0) w[j] = xj;
        for (int i = lane; i < j; i += 64) t[i] += Lw[j + i * m] * xj;
        wave_sync();
    }
    for (int j = lane; j < k; j += 64) stc<COH>(a.x + c0 + j, w[j]);
    if (a.xtag[s]) {
        const uint32_t ep = *a.epoch;
        for (int j = lane; j < k; j += 64) tag_pair(a.xg + 2 * (int64_t)(c0 + j), w[j], ep);
    }
    wave_sync();
}

__global__ __launch_bounds__(64) void mf_backward_wave(const MfArgs a) {
    extern __shared__ __attribute__((aligned(16))) double w[];
    backward_front<kModeLevel>(a, a.level[blockIdx.x], w, threadIdx.x, nullptr, nullptr);
}

// Backward substitution of the folded landmarks (k = 2), kFoldLanes lanes each (rows of the
// landmark's two L columns across the lanes, coalesced): t = L21^T x_rows reduced over the lanes,
// then x1 = (y1 - t1) / L11, x0 = (y0 - t0 - L10 x1) / L00. A lane takes up to four rows per pass
// with every load of the pass issued at once (row indices and L values, then the x gathers), and
// the landmark's own values are loaded before them: the launch is latency bound (few dependent
// hops per landmark, 200k landmarks), so fewer lanes per landmark with more loads in flight each
// beat one row per lane.
// (one lane per landmark from a packed record measured slower: DESIGN.md §4)
#ifndef BOS_MF_FOLD_LANES
#define BOS_MF_FOLD_LANES 4
#endif
// measured: 22 us at 4 lanes, 23 at 8, 34 at 16 (config 3); round 5: 2 / 8 lanes +10 / +3 us of solve
constexpr int kFoldLanes = BOS_MF_FOLD_LANES;
__global__ __launch_bounds__(kMfBlock) void mf_backward_fold(const MfArgs a) {
    const int g = (blockIdx.x * kMfBlock + threadIdx.x) / kFoldLanes;
    const int q0 = threadIdx.x % kFoldLanes;
    const bool valid = g < a.count;
    const int s = valid ? a.level[g] : 0;
    const int r = valid ? a.r[s] : 0, m = 2 + r;
    const double* Ls = a.L + (valid ? a.L_off[s] : 0);
    const int32_t* fi = a.findex + (valid ? a.findex_off[s] : 0) + 2;
    const int c0 = valid ? a.col0[s] : 0;
    const bool head = valid && q0 == 0;
    // the landmark's own values, read by all its lanes (one address: no extra traffic) so no branch
    // holds a wait; only the head lane uses them
    const double y0v = a.x[c0], y1v = a.x[c0 + 1], L00v = LD_LF(Ls, 0), L10v = LD_LF(Ls, 1), L11v = LD_LF(Ls, m + 1);
    const double y0 = head ? y0v : 0.0, y1 = head ? y1v : 0.0;
    const double L00 = head ? L00v : 1.0, L10 = head ? L10v : 0.0, L11 = head ? L11v : 1.0;
    double t0 = 0.0, t1 = 0.0;
    const int rl = r > 0 ? r - 1 : 0;   // reads of rows past r are clamped (and their products dropped)
    for (int q = q0; q < r; q += 4 * kFoldLanes) {
        int idx[4];
        double la[4], lb[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int qq = min(q + u * kFoldLanes, rl);
            idx[u] = fi[qq];
            la[u] = LD_LF(Ls, 2 + qq);
            lb[u] = LD_LF(Ls, m + 2 + qq);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = a.x[idx[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = q + u * kFoldLanes < r;
            t0 += ok ? la[u] * xv[u] : 0.0;
            t1 += ok ? lb[u] * xv[u] : 0.0;
        }
    }
#pragma unroll
    for (int o = kFoldLanes / 2; o > 0; o >>= 1) {
        t0 += __shfl_xor(t0, o, kFoldLanes);
        t1 += __shfl_xor(t1, o, kFoldLanes);
    }
    if (head) {
        const double x1 = (y1 - t1) / L11;
        t0 += L10 * x1;
        a.x[c0] = (y0 - t0) / L00;
        a.x[c0 + 1] = x1;
    }
}

__global__ __launch_bounds__(64) void mf_backward_flow(const MfArgs a, const Flow f_in, const int32_t* parent) {
    extern __shared__ __attribute__((aligned(16))) double w[];
    Flow f = f_in;
    f.epoch = *f_in.epoch_src;
    for (int it = 0; it <= f.n; ++it) {
        const int t = next_ticket(f.ticket);
        if (t >= f.n) break;
        const int s = f.order[t];
        backward_front<kModeFlow>(a, s, w, threadIdx.x, &f, parent);
        // (no completion flag: the children poll the tagged x granules themselves)
        fstamp(f.stamps, s, 4);
    }
    leave_flow(f);
}

}  // namespace

}  // namespace dev
}  // namespace bos
