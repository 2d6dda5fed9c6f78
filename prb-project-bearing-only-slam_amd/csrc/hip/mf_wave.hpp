// The wave-front kernels: one wavefront per front of m <= kMfWaveMaxM rows. The register pivot loop
// (factor_front_reg: class 16 per level, classes 16 and 32 of the mixed launch, the factor flow), the
// panel kernel (factor_front_pan: classes 48 and 64), the mixed launch that packs a level's blocked and
// wave fronts into one grid, and the factor flow.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/plan.hpp"
#include "mf_blk.hpp"
#include "mf_device.hpp"
#include "mf_flow.hpp"
#include "mf_fold.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

// One wavefront per front with m <= MAXM, the factorization in registers: lane i holds row i of
// the (lower) front in a compile-time-indexed array; each column step broadcasts the pivot column
// through a small LDS buffer (one store per lane, broadcast reads). LDS otherwise only stages the
// assembly. F: packed front (MAXM (MAXM + 1) / 2), colbuf: 2 MAXM.

// Factorization of one front fused with its forward elimination: w (LDS, m doubles) receives the
// front's right-hand side (x of its own dofs) plus the children's u-vectors, extend-added with
// their update matrices; after the partial Cholesky, lane i eliminates with its row of L (still in
// registers): y_j = w_j / L_jj, w_i -= L_ij y_j. y goes to x, the remaining w (rows >= k) to the
// front's u-vector for its parent.
template <int MAXM, int MODE, bool F32>
__device__ __forceinline__ void factor_front_reg(const MfArgs& a, int s, double* F, double* colbuf,
                                                 double* wv, FoldBuf* fb, int lane, const Flow* f) {
    constexpr bool COH = MODE == kModeFlow;
    const int k = a.k[s], r = a.r[s], m = k + r;
    const int nfold = a.fold_cnt[s];
    const int c0 = a.col0[s];
    const int aq0 = a.amap_ptr[s], aq1 = a.amap_ptr[s + 1];   // the assembly's range, loaded up front
    const int np = m * (m + 1) / 2;
    double xo = a.x[c0 + min(lane, k - 1)];   // right-hand side of the own dofs (k < 64; unconditional read)
    // output offsets up front: their loads complete during the assembly instead of before the pivots
    double* Ls = a.L + a.L_off[s];
    double* Us = a.U + a.U_off[s];
    double* us = a.u + a.u_off[s];
    // The first two (non-folded) children's structure is loaded up front, in flight during the
    // assembly and the fold. Everything up to the extend-add depends on H only, so the flow kernel
    // waits for the children after it: on the critical path a front's assembly and fold overlap
    // its children's work.
    const int cb = a.child_ptr[s] + nfold, ce = a.child_ptr[s + 1];
    ChildPre p0, p1;
    if (cb < ce) child_meta(a, a.child[cb], lane, p0);
    if (cb + 1 < ce) child_meta(a, a.child[cb + 1], lane, p1);
    // the folded landmarks first (their W uses F's LDS): F and the u-vector accumulator wv start
    // from minus their contribution, the assembly then adds H
    const bool fold = nfold > 0;
    unsigned long long* const stp = f ? f->stamps : a.stamps_f;
    fstamp(stp, s, 0);
    if (fold) {
        FoldAcc<MAXM> facc;
        fold_children<MAXM, F32>(a, s, F, fb, m, lane, facc);
        wave_sync();
        fold_store<MAXM>(facc, F, wv, m, lane);
    } else {
        for (int e = lane; e < np; e += 64) F[e] = 0.0;
        for (int i = lane; i < m; i += 64) wv[i] = 0.0;    // children's u-vectors accumulate here
    }
    wave_sync();
    fstamp(stp, s, 1);
    assemble_wave(a, aq0, aq1, F, lane, fold);
    wave_sync();
    // the own right-hand side has arrived by now (the assembly waited for its loads): pin it here,
    // so that the compiler does not leave its wait (one memory latency) in front of the pivots
    asm volatile("" : "+v"(xo));
    xo = lane < k ? xo : 0.0;
    fstamp(stp, s, 2);
    // children of this flow hand over tagged granules (child_sweep polls the data itself); children of
    // earlier launches are final (kernel boundary): plain reads
    uint32_t ep = 0;
    if constexpr (MODE == kModeFlow) ep = f->epoch;
    fstamp(stp, s, 3);
#ifdef BOS_MF_PIVOT_CYCLES
    unsigned long long* const cst = stp ? g_pivot_bwd : nullptr;
    cstamp(cst, s, 1);
#endif
    // extend-add, children in list order (deterministic)
    if (cb < ce) {
        if (MODE == kModeFlow && p0.G) child_sweep(p0, ep, lane, a.info);
        else child_vals<COH>(lane, p0);
    }
    if (cb + 1 < ce) {
        if (MODE == kModeFlow && p1.G) child_sweep(p1, ep, lane, a.info);
        else child_vals<COH>(lane, p1);
    }
#ifdef BOS_MF_PIVOT_CYCLES
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the children's values have arrived
    cstamp(cst, s, 2);
#endif
    if (cb < ce) extend_child<COH>(a, p0, F, wv, m, lane, ep);
    if (cb + 1 < ce) extend_child<COH>(a, p1, F, wv, m, lane, ep);
    for (int ci = cb + 2; ci < ce; ++ci) {
        ChildPre pq;
        child_meta(a, a.child[ci], lane, pq);
        if (MODE == kModeFlow && pq.G) child_sweep(pq, ep, lane, a.info);
        else child_vals<COH>(lane, pq);
        extend_child<COH>(a, pq, F, wv, m, lane, ep);
    }
#ifdef BOS_MF_PIVOT_CYCLES
    cstamp(cst, s, 3);
#endif
    const bool live = lane < m;
    const int lrow = min(lane, m - 1);
    double row[MAXM];
#if defined(BOS_MF_PIVOT_CYCLES) && defined(BOS_MF_ROWS_STAMPS)
    cstamp(cst, s, 5);   // (diagnostic: slots 5 / 6 split the row loads instead of timing pivot steps)
#endif
#pragma unroll
    for (int c0 = 0; c0 < MAXM; c0 += 8) {   // whole groups of 8 past m skipped by a scalar branch
#if defined(BOS_MF_PIVOT_CYCLES) && defined(BOS_MF_ROWS_STAMPS)
        if (c0 == 8) cstamp(cst, s, 6);
#endif
        if (c0 < m) {
            // branch-free: every lane reads a position of the LDS front (the column clamped to m - 1:
            // for a row i < m and a column c' < m, 0 <= pk32(i, c', m) < np, also above the diagonal;
            // unclamped, m <= 3 would give negative positions), the group's eight reads
            // under one wait. A predicated read per
            // entry compiled to an exec-mask branch with its own wait each (~2 500 cycles for the rows
            // of a 24-row front); the empty asm keeps the reads out of such branches. Entries above
            // the diagonal, of rows >= m (copies of row m - 1) and of columns >= m are scratch that no
            // stored or broadcast value ever reads, so they are taken as read: selecting zeros there
            // held 48 loop-invariant lane masks that the compiler spilled to VGPR lanes and read back
            // per column. (All columns read at once, without the groups' waits and zero fills: rows
            // 1 500 -> 1 260 cycles at the top, 3 430 -> 2 830 at level 0, solve unchanged,
            // profiles/r05_rows_all_at_once_ab.txt.)
            double v[8];
#pragma unroll
            for (int c = c0; c < c0 + 8; ++c) v[c - c0] = c < MAXM ? F[pk32(lrow, min(c, m - 1), m)] : 0.0;
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]),
                         "+v"(v[7]));
#pragma unroll
            for (int c = c0; c < c0 + 8 && c < MAXM; ++c) row[c] = v[c - c0];
        } else {
#pragma unroll
            for (int c = c0; c < c0 + 8 && c < MAXM; ++c) row[c] = 0.0;
        }
    }
    fstamp(stp, s, 4);
    double wi = live ? wv[lane] + xo : 0.0;   // forward elimination, fused into the pivot loop
    // Right-looking, with a rotating register window: before step j, row[t] holds column j + t of
    // this lane's row, so the pivot column is always row[0] and the update of column j + 1 + t is
    // written to row[t] (the shift costs nothing). The pivot loop is a real loop — one copy of its
    // body instead of MAXM unrolled ones keeps the kernel inside the instruction cache. Column j
    // (rows > j) is broadcast through a double-buffered LDS column indexed by t; entries above the
    // diagonal, rows >= m and columns >= m are scratch, so the updates need no predicates.
    const int kf = k;
    int nbad = 0;   // non-positive pivots (uniform), reported once per front
    double* Lj = Ls + lane;
    int j = 0;
#ifdef BOS_MF_PIVOT_CYCLES
    cstamp(cst, s, 0);
#endif
    // Two pivots per step: column j + 1 is brought up to date in registers (L(j+1, j) by readlane),
    // both columns go through ONE LDS broadcast as pairs, and the trailing columns take a rank-2
    // update; the window rotates by two.
    {
#pragma nounroll
        for (; j + 1 < kf; j += 2) {
            double d0 = readlane_d(row[0], j);
            const bool bad0 = !(d0 > 0.0);
            nbad += bad0;
            d0 = bad0 ? 1e-300 : d0;
            const double inv0 = rsqrt_nr(d0), l00 = d0 * inv0;
            const double l0 = lane == j ? l00 : row[0] * inv0;   // L[i, j]
            const double lj1 = readlane_d(l0, j + 1);            // L[j+1, j]
            const double f1 = fma(-l0, lj1, row[1]);             // column j+1 after pivot j
            double d1 = readlane_d(f1, j + 1);
            const bool bad1 = !(d1 > 0.0);
            nbad += bad1;
            d1 = bad1 ? 1e-300 : d1;
            const double inv1 = rsqrt_nr(d1), l11 = d1 * inv1;
            const double l1 = lane == j + 1 ? l11 : f1 * inv1;   // L[i, j+1]
            double2* cp = reinterpret_cast<double2*>(colbuf);   // (L[l, j], L[l, j+1]), l = j + 2 + t
            if (lane > j + 1 && lane < m) cp[lane - j - 2] = make_double2(l0, l1);
            if (live) {
                if (lane >= j) ST_L(Lj, 0, l0);
                if (lane >= j + 1) ST_L(Lj, m, l1);
            }
            Lj += 2 * m;
            const double y0 = readlane_d(wi, j) * inv0;          // forward steps j, j + 1
            if (lane == j) wi = y0;
            else if (lane > j) wi -= l0 * y0;
            const double y1 = readlane_d(wi, j + 1) * inv1;
            if (lane == j + 1) wi = y1;
            else if (lane > j + 1) wi -= l1 * y1;
            wave_sync();
            const int nt = m - j - 2;                            // live columns after this step
#pragma unroll
            for (int t0 = 0; t0 < MAXM - 2; t0 += 8) {
                if (t0 < nt) {
                    // the group's eight pairs read at once (one LDS latency per group; pairs past the
                    // live columns are scratch), the empty asm keeps the compiler from interleaving a
                    // wait per pair: two-pivot step 1 269 -> 1 037 cycles at m = 18, 1 818 -> 1 554 at
                    // m = 42 (tools/pivot_probe2.hip, profiles/r05_pivot_step_anatomy.txt)
                    double2 c[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) c[u] = t0 + u < MAXM - 2 ? cp[t0 + u] : make_double2(0.0, 0.0);
#pragma unroll
                    for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(c[u].x), "+v"(c[u].y));
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (t0 + u < MAXM - 2) row[t0 + u] = fma(-l1, c[u].y, fma(-l0, c[u].x, row[t0 + u + 2]));
                }
            }
            __builtin_amdgcn_wave_barrier();   // the next step's pair stores stay after these reads
#ifdef BOS_MF_PIVOT_CYCLES
#ifdef BOS_MF_ROWS_STAMPS
            if (j / 2 < 1) cstamp(cst, s, 4 + j / 2);
#else
            if (j / 2 < 3) cstamp(cst, s, 4 + j / 2);
#endif
#endif
        }
    }
#pragma nounroll
    for (; j < kf; ++j) {
        double* col = colbuf + (j & 1) * MAXM;
        if (lane > j && lane < m) col[lane - j - 1] = row[0];
        // the pivot straight from lane j's register (no LDS round trip on the critical path; the
        // column's LDS broadcast lands meanwhile), 1 / sqrt(d) by v_rsq_f64 + two Newton steps
        double d = readlane_d(row[0], j);
        wave_sync();
        // the first 8 column entries are read before the pivot arithmetic (no branch between), so
        // their LDS latency overlaps it
        double c0v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c0v[u] = u < MAXM ? col[u] : 0.0;
        const bool bad = !(d > 0.0);
        nbad += bad;
        d = bad ? 1e-300 : d;
        const double inv = rsqrt_nr(d), ljj = d * inv;
        const double lij = lane == j ? ljj : row[0] * inv;   // L[i, j]
        if (live && lane >= j) ST_L(Lj, 0, lij);
        Lj += m;
        // forward step: y_j = w_j / L_jj, w_i -= L_ij y_j
        const double yj = readlane_d(wi, j) * inv;
        if (lane == j) wi = yj;
        else if (lane > j) wi -= lij * yj;
        const double g = lij * inv;                          // L[i, j] / L[j, j]
        const int nt = m - j - 1;                            // live columns after this step (uniform)

#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u < MAXM - 1) row[u] = fma(-g, c0v[u], row[u + 1]);   // -= L[i,j] L[l,j], l = j + 1 + t
#pragma unroll
        for (int t0 = 8; t0 < MAXM - 1; t0 += 8) {
            if (t0 < nt) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int t = t0 + u;
                    if (t < MAXM - 1) row[t] = fma(-g, col[t], row[t + 1]);
                }
            }
        }
    }
#ifdef BOS_MF_PIVOT_CYCLES
    cstamp(cst, s, 7);
#endif
    if (nbad && lane == 0) atomicAdd(a.info, nbad);
    fstamp(stp, s, 5);
    // the update matrix: row[t] holds column k + t; for a parent in this flow as tagged granules
    // (update matrix, then u-vector), else plain (coherent) stores
    unsigned long long* const G = (MODE == kModeFlow && a.ug_off[s] >= 0) ? a.Ug + a.ug_off[s] : nullptr;
    if (G) {
#pragma unroll
        for (int t0 = 0; t0 < MAXM; t0 += 8) {
            if (t0 < r) {
#pragma unroll
                for (int t = t0; t < t0 + 8 && t < MAXM; ++t)
                    if (live && lane >= k && t <= lane - k) tag_pair(G + 2 * pk(lane - k, t, r), row[t], ep);
            }
        }
    } else {
#pragma unroll
        for (int t0 = 0; t0 < MAXM; t0 += 8) {
            if (t0 < r) {
#pragma unroll
                for (int t = t0; t < t0 + 8 && t < MAXM; ++t)
                    if (live && lane >= k && t <= lane - k) stc<COH>(Us + pk(lane - k, t, r), row[t]);
            }
        }
    }
    if (live) {
        if (lane < k) a.x[c0 + lane] = wi;
        else if (G) tag_pair(G + 2 * ((int64_t)r * (r + 1) / 2 + (lane - k)), wi, ep);
        else stc<COH>(us + (lane - k), wi);
    }
    wave_sync();
}

// (class 48 bounded to 4 waves per SIMD spills and measured slower)
template <int MAXM, bool F32>
__global__ __launch_bounds__(64, 1) void mf_factor_reg(const MfArgs a) {
    __shared__ __attribute__((aligned(16))) double F[MAXM * (MAXM + 1) / 2];
    __shared__ __attribute__((aligned(16))) double colbuf[2 * MAXM];
    __shared__ __attribute__((aligned(16))) double wv[MAXM];
    __shared__ FoldBuf fb;
    factor_front_reg<MAXM, kModeLevel, F32>(a, a.level[blockIdx.x], F, colbuf, wv, &fb, threadIdx.x, nullptr);
}

// Level-launch wave fronts with the pivots on register panels and the trailing update on f64 MFMA
// (VERDICT r05 next 1). factor_front_reg holds a lane's whole front row in registers (row[MAXM]): at
// class 48 that is 96 of the kernel's 147 VGPRs and caps level 0 (10 350 fronts, k ~ 18, m ~ 42) at 3
// waves per SIMD. Here a lane holds only the KP columns of the current panel: the pivot loop (the
// same two-pivot steps, LDS pair broadcast) runs over the panel's columns, the L columns go to global
// memory as before and into the front's LDS triangle in place of the columns they replace, and the
// rest of the front, still in LDS, takes A22 -= L21 L21^T in 16 x 16 tiles on v_mfma_f64_16x16x4f64
// (the fold's W W^T pattern); the last panel's tiles go straight to the update matrix. The prologue
// (fold, assembly, children) is factor_front_reg's, with the children's structure read after the
// fold instead of before it (its registers would be live across the fold).
template <int MAXM, int KP, bool F32>
__device__ __forceinline__ void factor_front_pan(const MfArgs& a, int s, double* F, double* colbuf, double* wv,
                                                 FoldBuf* fb, int lane) {
    const int k = a.k[s], r = a.r[s], m = k + r;
    const int nfold = a.fold_cnt[s];
    const int c0 = a.col0[s];
    const int aq0 = a.amap_ptr[s], aq1 = a.amap_ptr[s + 1];
    const int np = m * (m + 1) / 2;
    double xo = a.x[c0 + min(lane, k - 1)];
    double* Ls = a.L + a.L_off[s];
    double* Us = a.U + a.U_off[s];
    double* us = a.u + a.u_off[s];
    const int cb = a.child_ptr[s] + nfold, ce = a.child_ptr[s + 1];
    unsigned long long* const stp = a.stamps_f;
    fstamp(stp, s, 0);
    if (nfold > 0) {
        FoldAcc<MAXM> facc;
        fold_children<MAXM, F32>(a, s, F, fb, m, lane, facc);
        wave_sync();
        fold_store<MAXM>(facc, F, wv, m, lane);
    } else {
        for (int e = lane; e < np; e += 64) F[e] = 0.0;
        for (int i = lane; i < m; i += 64) wv[i] = 0.0;
    }
    wave_sync();
    fstamp(stp, s, 1);
    ChildPre p0c, p1c;   // (structure in flight during the assembly)
    if (cb < ce) child_meta(a, a.child[cb], lane, p0c);
    if (cb + 1 < ce) child_meta(a, a.child[cb + 1], lane, p1c);
    assemble_wave(a, aq0, aq1, F, lane, nfold > 0);
    wave_sync();
    asm volatile("" : "+v"(xo));
    xo = lane < k ? xo : 0.0;
    fstamp(stp, s, 2);
    fstamp(stp, s, 3);
    if (cb < ce) child_vals<false>(lane, p0c);
    if (cb + 1 < ce) child_vals<false>(lane, p1c);
    if (cb < ce) extend_child<false>(a, p0c, F, wv, m, lane);
    if (cb + 1 < ce) extend_child<false>(a, p1c, F, wv, m, lane);
    for (int ci = cb + 2; ci < ce; ++ci) {
        ChildPre pq;
        child_meta(a, a.child[ci], lane, pq);
        child_vals<false>(lane, pq);
        extend_child<false>(a, pq, F, wv, m, lane);
    }
    fstamp(stp, s, 4);
    const bool live = lane < m;
    const int lrow = min(lane, m - 1);
    double wi = live ? wv[lane] + xo : 0.0;   // forward elimination, fused into the pivot loop
    int nbad = 0;
    double2* cp = reinterpret_cast<double2*>(colbuf);
    for (int p0 = 0; p0 < k; p0 += KP) {
        const int nb = min(KP, k - p0);
        // row[t] = F(lane, p0 + t) (column clamped to m - 1: branch-free reads, one wait; entries
        // above the diagonal, of rows >= m and columns past the panel are scratch)
        double row[KP];
#pragma unroll
        for (int t0 = 0; t0 < KP; t0 += 8) {
            double v[8];
#pragma unroll
            for (int t = t0; t < t0 + 8; ++t) v[t - t0] = F[pk32(lrow, min(p0 + t, m - 1), m)];
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]),
                         "+v"(v[7]));
#pragma unroll
            for (int t = t0; t < t0 + 8; ++t) row[t] = v[t - t0];
        }
        double* Lj = Ls + lane + (int64_t)p0 * m;
        int j = 0;   // pivot p0 + j; before step j, row[t] holds column p0 + j + t
#pragma nounroll
        for (; j + 1 < nb; j += 2) {
            const int J = p0 + j;
            double d0 = readlane_d(row[0], J);
            const bool bad0 = !(d0 > 0.0);
            nbad += bad0;
            d0 = bad0 ? 1e-300 : d0;
            const double inv0 = rsqrt_nr(d0), l00 = d0 * inv0;
            const double l0 = lane == J ? l00 : row[0] * inv0;   // L[i, J]
            const double lj1 = readlane_d(l0, J + 1);
            const double f1 = fma(-l0, lj1, row[1]);
            double d1 = readlane_d(f1, J + 1);
            const bool bad1 = !(d1 > 0.0);
            nbad += bad1;
            d1 = bad1 ? 1e-300 : d1;
            const double inv1 = rsqrt_nr(d1), l11 = d1 * inv1;
            const double l1 = lane == J + 1 ? l11 : f1 * inv1;   // L[i, J + 1]
            // pairs of the panel's later rows (the rank-2 update of its remaining columns)
            if (lane > J + 1 && lane < p0 + nb) cp[lane - J - 2] = make_double2(l0, l1);
            if (live) {
                if (lane >= J) {
                    ST_L(Lj, 0, l0);
                    F[pk32(lane, J, m)] = l0;   // L21 for the trailing update (column J is consumed)
                }
                if (lane >= J + 1) {
                    ST_L(Lj, m, l1);
                    F[pk32(lane, J + 1, m)] = l1;
                }
            }
            Lj += 2 * m;
            const double y0 = readlane_d(wi, J) * inv0;          // forward steps J, J + 1
            if (lane == J) wi = y0;
            else if (lane > J) wi -= l0 * y0;
            const double y1 = readlane_d(wi, J + 1) * inv1;
            if (lane == J + 1) wi = y1;
            else if (lane > J + 1) wi -= l1 * y1;
            wave_sync();
            const int nt = nb - j - 2;                           // panel columns left after this step
#pragma unroll
            for (int t0 = 0; t0 < KP - 2; t0 += 8) {
                if (t0 < nt) {
                    double2 c[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) c[u] = t0 + u < KP - 2 ? cp[t0 + u] : make_double2(0.0, 0.0);
#pragma unroll
                    for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(c[u].x), "+v"(c[u].y));
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (t0 + u < KP - 2) row[t0 + u] = fma(-l1, c[u].y, fma(-l0, c[u].x, row[t0 + u + 2]));
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (j < nb) {   // the panel's last column (odd nb)
            const int J = p0 + j;
            double d = readlane_d(row[0], J);
            const bool bad = !(d > 0.0);
            nbad += bad;
            d = bad ? 1e-300 : d;
            const double inv = rsqrt_nr(d), ljj = d * inv;
            const double lij = lane == J ? ljj : row[0] * inv;
            if (live && lane >= J) {
                ST_L(Lj, 0, lij);
                F[pk32(lane, J, m)] = lij;
            }
            const double yj = readlane_d(wi, J) * inv;
            if (lane == J) wi = yj;
            else if (lane > J) wi -= lij * yj;
        }
        wave_sync();
        // trailing block, rows / columns [t0, m): A22 -= L21 L21^T (L21 = rows >= t0 of the panel's L
        // columns, now in F) in 16 x 16 tiles; the last panel's result is the update matrix
        const int t0 = p0 + nb, T = m - t0;
        if (T > 0) {
            const bool last = t0 == k;
            const int nbt = (T + 15) >> 4;
            for (int bi = 0; bi < nbt; ++bi)
                for (int bj = 0; bj <= bi; ++bj) {
                    const int ra = t0 + 16 * bi + (lane & 15), rb = t0 + 16 * bj + (lane & 15);
                    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
                    for (int kk = 0; kk < nb; kk += 4) {
                        const int cc = kk + (lane >> 4);
                        const int col = p0 + min(cc, nb - 1);
                        const double av = F[pk32(min(ra, m - 1), col, m)];
                        const double bv = F[pk32(min(rb, m - 1), col, m)];
                        const bool ok = cc < nb;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ok && ra < m ? av : 0.0, ok && rb < m ? bv : 0.0,
                                                                   acc, 0, 0, 0);
                    }
                    const int jj = t0 + 16 * bj + (lane & 15);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ii = t0 + 16 * bi + (lane >> 4) + 4 * e;
                        if (ii < m && jj <= ii) {
                            const double v = F[pk32(ii, jj, m)] - acc[e];
                            if (last) Us[pk(ii - k, jj - k, r)] = v;
                            else F[pk32(ii, jj, m)] = v;
                        }
                    }
                }
            wave_sync();
        }
    }
    if (nbad && lane == 0) atomicAdd(a.info, nbad);
    fstamp(stp, s, 5);
    if (live) {
        if (lane < k) a.x[c0 + lane] = wi;
        else us[lane - k] = wi;
    }
    wave_sync();
}

// The class-48 level launches take the panel kernel, and the class-64 ones too (config 2's
// separators of 49-64 rows; config 3's side-stream class), with panels of kPanelKP columns.
#ifndef BOS_MF_PAN_KP
#define BOS_MF_PAN_KP 24
#endif
constexpr int kPanelKP = BOS_MF_PAN_KP;
// waves per SIMD the panel kernel is compiled for. Its register peak is the fold (the panel's rows
// alone take 92 VGPRs, the fold 132), so it stays at mf_factor_reg<48>'s 3 waves per SIMD; bounded to 4
// it spills 3 registers (14 in fp64) and measured no faster. Measured (config 3, tools/gn_ab.py, two
// rounds, profiles/r06_panel_ab.txt): solve 439.6 / 442.8 us with mf_factor_reg, 439.0 / 439.8 with
// 16-column panels at 4 waves, 433.7 / 432.0 with 24 columns at 3 waves (one panel for most level-0
// fronts, k ~ 18), 433.6 / 434.4 with 32.
#ifndef BOS_MF_PAN_WAVES
#define BOS_MF_PAN_WAVES 3
#endif

template <int MAXM, int KP> struct WaveLds {
    double F[MAXM * (MAXM + 1) / 2];
    double colbuf[2 * (KP > 0 ? KP : MAXM)];
    double wv[MAXM];
    FoldBuf fb;
};
template <int MAXM, int KP, bool F32>
__global__ __launch_bounds__(64, MAXM > 48 ? 2 : BOS_MF_PAN_WAVES) void mf_factor_pan(const MfArgs a) {
    __shared__ __attribute__((aligned(16))) double F[MAXM * (MAXM + 1) / 2];
    __shared__ __attribute__((aligned(16))) double colbuf[2 * KP];
    __shared__ __attribute__((aligned(16))) double wv[MAXM];
    __shared__ FoldBuf fb;
    factor_front_pan<MAXM, KP, F32>(a, a.level[blockIdx.x], F, colbuf, wv, &fb, threadIdx.x);
}

// One wave front of class 3, 2, 1 or 0 with its LDS at slot (mf_factor_mixb)
template <int MAXM, int KP, bool F32>
__device__ __forceinline__ void wave_front(const MfArgs& a, int s, char* slot, int lane) {
    auto* L = reinterpret_cast<WaveLds<MAXM, KP>*>(slot);
    if constexpr (KP > 0)
        factor_front_pan<MAXM, KP, F32>(a, s, L->F, L->colbuf, L->wv, &L->fb, lane);
    else
        factor_front_reg<MAXM, kModeLevel, F32>(a, s, L->F, L->colbuf, L->wv, &L->fb, lane, nullptr);
}

// A level with blocked fronts (65-128 rows, config 2's separators) and few fronts in all: ONE launch
// of four-wave workgroups instead of the blocked launch on a second side stream beside the wave
// fronts (each level then paid a fork and a join, ~10 us per level at config 2). The first n4
// workgroups each factor one blocked front (factor_front_blk, the whole dynamic LDS), each of the
// others one wave front of class 3, 2, 1 or 0 on its first wave (the other three leave at once; two
// wave fronts in one workgroup computed wrong factors). Registers are the blocked
// path's (1 wave per SIMD), so the host uses it only when the level fits the GPU in one round (one
// workgroup per CU); dynamic LDS max(blocked front, one class-64 front).
template <bool F32>
__global__ __launch_bounds__(kMfBlock) void mf_factor_mixb(const MfArgs a, const int32_t* blk_list, int n4, int4 n, int4 o) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x;
    if (b < n4) {   // (uniform per workgroup)
        factor_front_blk<F32>(a, blk_list[b], lds);
        return;
    }
#ifdef BOS_DIAG_PAIR   // (diagnostics: class-2 fronts two per workgroup, on waves 0 and BOS_DIAG_PAIR)
    {
        const int wv = threadIdx.x >> 6;
        int i = b - n4;
        if (i >= n.w && i - n.w < (n.z + 1) / 2) {
            const int j = 2 * (i - n.w) + (wv == BOS_DIAG_PAIR ? 1 : 0);
            if ((wv == 0 || wv == BOS_DIAG_PAIR) && j < n.z)
                wave_front<48, kPanelKP, F32>(a, a.level[o.z + j],
                                              reinterpret_cast<char*>(lds) + wv * 10400 * 1, threadIdx.x & 63);
            return;
        }
    }
#endif
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    char* slot = reinterpret_cast<char*>(lds);
    const int32_t* lst = a.level;
    int i = b - n4;
    if (i < n.w) { wave_front<64, kPanelKP, F32>(a, lst[o.w + i], slot, lane); return; }
    i -= n.w;
#ifdef BOS_DIAG_PAIR
    i -= (n.z + 1) / 2;
#else
    if (i < n.z) { wave_front<48, kPanelKP, F32>(a, lst[o.z + i], slot, lane); return; }
    i -= n.z;
#endif
    if (i < n.y) { wave_front<32, 0, F32>(a, lst[o.y + i], slot, lane); return; }
    i -= n.y;
    if (i < n.x) wave_front<16, 0, F32>(a, lst[o.x + i], slot, lane);
}
#ifdef BOS_DIAG_PAIR
constexpr int kMixbWaveLds = 4 * 10400;
static_assert(sizeof(WaveLds<48, kPanelKP>) <= 10400, "diagnostic slot");
#else
constexpr int kMixbWaveLds = (int)sizeof(WaveLds<64, kPanelKP>);
#endif

// The flow kernel instantiates one register class only: inlining all four merged their register
// demands (256 VGPRs + AGPRs, 1 wave per SIMD), out-of-line calls spilled, and forcing 4 waves per
// SIMD spilled too (all measured slower); 2 waves per SIMD (no spills) measured faster than 3 (a
// few spilled registers). Fronts of the flow range are <= kFlowMaxM (mf_create picks the range
// accordingly).
constexpr int kFlowMaxM = kMfFlowMaxM;

template <bool F32>
__device__ __forceinline__ void factor_flow_body(const MfArgs& a, const Flow& f) {
    __shared__ __attribute__((aligned(16))) double F[kFlowMaxM * (kFlowMaxM + 1) / 2];
    __shared__ __attribute__((aligned(16))) double colbuf[2 * kFlowMaxM];
    __shared__ __attribute__((aligned(16))) double wv[kFlowMaxM];
    __shared__ FoldBuf fb;
    const int lane = threadIdx.x;
    // a wave takes at most n + 1 tickets: the loop is bounded (an unbounded for (;;) version of
    // this kernel never terminated on gfx950 / ROCm 7.2)
    for (int it = 0; it <= f.n; ++it) {
        const int t = next_ticket(f.ticket);
        if (t >= f.n) break;
        const int s = f.order[t];
        factor_front_reg<kFlowMaxM, kModeFlow, F32>(a, s, F, colbuf, wv, &fb, lane, &f);   // m <= kFlowMaxM
        // (no completion flag: a parent in this flow polls the tagged granules themselves)
        fstamp(f.stamps, s, 6);
        fstamp(f.stamps, s, 7);
    }
    leave_flow(f);
}

template <bool F32>
__global__ __launch_bounds__(64, 2) void mf_factor_flow(const MfArgs a, const Flow f_in) {
    Flow f = f_in;
    f.epoch = *f_in.epoch_src;
    factor_flow_body<F32>(a, f);
}

}  // namespace

}  // namespace dev
}  // namespace bos
