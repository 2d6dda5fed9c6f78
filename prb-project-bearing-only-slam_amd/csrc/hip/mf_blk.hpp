// The blocked kernel: fronts of kMfWaveMaxM < m <= kMfBlkMaxM rows, one 256-thread workgroup each, with
// the workgroup form of the fold. factor_front_blk is also the blocked half of the mixed launch
// (mf_wave.hpp mf_factor_mixb).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/plan.hpp"
#include "mf_device.hpp"
#include "mf_fold.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

// Larger fronts (kMfWaveMaxM < m <= kBlkMaxM: config 2's separators, m ~ 60-100): one 256-thread
// workgroup per front, the whole m x m front in LDS (column-major, leading dimension m, as the plan's
// amap_dst), a blocked right-looking partial Cholesky of its k columns fused with the forward step.
// Per panel of kBlkNb columns: wave 0 factors the panel with its rows in registers (two rows per lane,
// pivots broadcast by v_readlane, no barrier inside the panel) and carries the forward elimination
// along; then all four waves update the trailing lower triangle, A22 -= L21 L21^T, in 16 x 16 tiles
// on f64 MFMA (v_mfma_f64_16x16x4f64, the fold's W W^T pattern). The children's u-vectors are
// extend-added with their update matrices (no separate forward launch). mf_factor_level (with
// mf_forward_level) kept the front in global scratch above 90 rows and took ~140 us per level launch
// at config 2; it remains for m > kBlkMaxM (fallback plans).
#ifndef BOS_MF_BLK_NB   // (A/B builds: the blocked kernel's panel width, a multiple of 4)
#define BOS_MF_BLK_NB 16
#endif
constexpr int kBlkMaxM = kMfBlkMaxM, kBlkNb = BOS_MF_BLK_NB;
static_assert(kBlkNb % 4 == 0 && kBlkNb <= 64, "panel width: MFMA steps of 4 columns, one pair per lane");
constexpr int kBlkTiles = 9;   // 16 x 16 lower tiles per wave: (8 * 9 / 2 = 36 for 128 rows) / 4 waves
// dynamic LDS of a front of m rows: F (m x m), w (kBlkMaxM), the fold's chunk y and landmark count,
// the panel's column broadcast (kBlkNb)
inline int blk_lds_bytes(int m) { return (m * m + kBlkMaxM + 2 * fold_chunk_landmarks(kBlkMaxM) + 2 + 2 * kBlkNb) * 8; }
// children whose update matrices the blocked kernel prefetches (values and front positions, kBlkXU per
// thread: r <= 63), issued before the fold; more (or larger) children take the plain loop
constexpr int kBlkXCh = 2, kBlkXU = 8;

// The folded landmark children of a workgroup front (Schur ordering), the workgroup form of
// fold_children: per chunk (<= kFoldChunk observing poses, <= fold_chunk_landmarks(m) landmarks)
// wave 0's lanes take the chunk's records — the landmarks' 2 x 2 factors, L panels and forward steps,
// the chunk's W (front position x 2 columns per landmark, LDS aliasing F) and y — with the next
// chunk's records and values in flight; then every wave accumulates its 16 x 16 tiles of W W^T on f64
// MFMA (registers, acc[u]: tile wave + 4 u) and each row's thread -W y (wacc). The caller stores
// minus both into the front before its assembly.
template <bool F32>
__device__ __forceinline__ void fold_children_wg(const MfArgs& a, int s, double* W, double* ybuf, int* nlb, int m,
                                                 int tid, dbl4 acc[kBlkTiles], double& wacc) {
    constexpr int cap = fold_chunk_landmarks(kBlkMaxM);
    constexpr int WS = 2 * cap + 1;   // W row stride (odd: no bank conflicts)
    // the wave index as a scalar: branches on it are uniform, so a value loaded on wave 0's path lands in
    // its loop-carried register (a divergent branch merged the paths with copies that waited for the loads)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nbt = (m + 15) >> 4, ntiles = nbt * (nbt + 1) / 2;
#pragma unroll
    for (int u = 0; u < kBlkTiles; ++u) acc[u] = dbl4{0.0, 0.0, 0.0, 0.0};
    wacc = 0.0;
    for (int e = tid; e < m * WS; e += kMfBlock) W[e] = 0.0;
    if (tid < 2 * cap) ybuf[tid] = 0.0;
    const int ch0 = a.fold_cptr[s], ch1 = a.fold_cptr[s + 1];
    int nbad = 0;
    ChunkTable tb;
    auto rec = [&](int c, int cnt, int4& q0, int4& q1) {
        const int q = tb.at(c) + min(lane, max(cnt - 1, 0));
        q0 = fold_rec_load(a, q, 0);
        q1 = fold_rec_load(a, q, 1);
    };
    auto len = [&](int c) { return c < ch1 ? tb.at(c + 1) - tb.at(c) : 0; };
    // Wave 0 alone walks the records (the other waves wait at the barrier), so no other wave hides its
    // memory latency: the values are loaded two chunks ahead and the records three, in two register
    // sets that alternate by chunk (the loop is unrolled by two, so a set keeps its registers: a
    // rotation of loop-carried registers made the compiler copy the freshly loaded values at the
    // chunk's end, a copy that waits for the loads).
    struct Set {
        FoldValsT<F32> v;   // values of the chunk this set holds
        int4 m;             // its records' second half (meta)
        int n;              // its rows
        int4 p0, p1;        // records of the chunk that refills the set next
        int np;
    } A, B;
    // (every wave issues the record and value loads, wave 0 alone uses them: loads under a branch on
    // the wave left the registers to be merged with the other waves' path at the branch's end — copies
    // that waited for the loads)
    tb.load(a, ch0, lane);
    {
        int4 q0;
        A.n = len(ch0);
        rec(ch0, A.n, q0, A.m);
        A.v = fold_vals<F32>(a, q0, A.m, lane < A.n);
        B.n = len(ch0 + 1);
        rec(ch0 + 1, B.n, q0, B.m);
        B.v = fold_vals<F32>(a, q0, B.m, lane < B.n);
        A.np = len(ch0 + 2);
        rec(ch0 + 2, A.np, A.p0, A.p1);
    }
    // the prologue's loads waited for here: the loop's top is then reached only from its back edge with
    // loads pending, and waits there for the values of two chunks ago alone (see fold_children)
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();   // (W cleared)
    // chunk ch from set X; X is refilled with chunk ch + 2's values, Y's records with chunk ch + 3's
#ifdef BOS_MF_BLK_FOLD_CYCLES   // (diagnostics: wave 0's cycles per chunk phase, tools/blk_fold_cycles.py)
    unsigned long long cyc[5] = {0, 0, 0, 0, 0};
    auto now = [&]() {
        unsigned long long t;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
        __builtin_amdgcn_sched_barrier(0);
        return t;
    };
#define BLK_CYC(i, t) cyc[i] += (t)
#else
#define BLK_CYC(i, t)
#endif
    auto chunk = [&](int ch, Set& X, Set& Y) {
        int pos = 0, lml = 0, ncur = 0;
#ifdef BOS_MF_BLK_FOLD_CYCLES
        const unsigned long long c0 = now();
#endif
        if (ch + 4 - tb.base > 63) tb.reload(a, ch, lane);
        FoldVals d = fold_decode(X.v);
        // the decoded values formed here, before the loads into X's registers are issued (left to
        // the compiler, the selects sank to their uses and X.v stayed live past the new loads)
        asm volatile("" : "+v"(d.h[0]), "+v"(d.h[1]), "+v"(d.h[2]), "+v"(d.h[3]), "+v"(d.h[4]), "+v"(d.h[5]),
                     "+v"(d.a00), "+v"(d.a10), "+v"(d.a11), "+v"(d.x0), "+v"(d.x1));
        const int4 q1 = X.m;
        ncur = X.n;
        // the records first, then the values: the memory counter retires in order, so the next
        // chunk's wait for these records must not include these values
        Y.np = len(ch + 3);
        rec(ch + 3, Y.np, Y.p0, Y.p1);
        X.v = fold_vals<F32>(a, X.p0, X.p1, lane < X.np);
        X.m = X.p1;
        X.n = X.np;
        if (wave == 0) {
            const int t = q1.z & 63, rc = (q1.z >> 6) & 63;
            pos = (q1.z >> kFoldPosShift) & kFoldPosMask;
            lml = (q1.z >> kFoldLmShift) & 63;
            const bool mine = lane < ncur;
            // as fold_chunk: every lane issues the same stores (a lane past the chunk's rows holds its
            // last row's record and values: the owners' bits to the owners' addresses)
            double d0 = d.a00;
            const bool bad0 = !(d0 > 0.0);
            d0 = bad0 ? 1e-300 : d0;
            const double i0 = rsqrt_nr(d0), l00 = d0 * i0;
            const double l10 = d.a10 * i0;
            double d1 = d.a11 - l10 * l10;
            const bool bad1 = !(d1 > 0.0);
            d1 = bad1 ? 1e-300 : d1;
            const double i1 = rsqrt_nr(d1), l11 = d1 * i1;
            const double y0 = d.x0 * i0, y1 = (d.x1 - l10 * y0) * i1;
            const int mc = 2 + rc;
            double* Lc = a.L + q1.w;
            const bool head = mine && t == 0;
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const double lt0 = d.h[2 * g] * i0;
                const double lt1 = (d.h[2 * g + 1] - lt0 * l10) * i1;
                ST_LF(Lc, 2 + t + g, lt0);
                ST_LF(Lc, mc + 2 + t + g, lt1);
                if (mine) {
                    W[(pos + g) * WS + 2 * lml] = lt0;
                    W[(pos + g) * WS + 2 * lml + 1] = lt1;
                }
            }
            ST_LF(Lc, 0, l00);
            ST_LF(Lc, 1, l10);
            ST_LF(Lc, mc + 1, l11);
            a.x[q1.y] = y0;
            a.x[q1.y + 1] = y1;
            nbad += head ? (int)bad0 + (int)bad1 : 0;
            if (head) {
                ybuf[2 * lml] = y0;
                ybuf[2 * lml + 1] = y1;
            }
            const int nl = __builtin_amdgcn_readlane(lml, ncur - 1) + 1;   // landmarks of this chunk
            // the 16-row blocks the chunk's W rows span (its poses are a band of the front's rows):
            // W W^T is zero outside them
            int lo = mine ? pos : 1 << 20, hi = mine ? pos + 2 : -1;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, __shfl_xor(lo, o));
                hi = max(hi, __shfl_xor(hi, o));
            }
            if (lane == 0) {
                nlb[0] = nl;
                nlb[1] = lo >> 4;
                nlb[2] = hi >> 4;
            }
        }
#ifdef BOS_MF_BLK_FOLD_CYCLES
        const unsigned long long c1 = now();
#endif
        __syncthreads();
#ifdef BOS_MF_BLK_FOLD_CYCLES
        const unsigned long long c2 = now();
#endif
        const int kc = 2 * nlb[0], blo = nlb[1], bhi = nlb[2];
        // The chunk's W columns past kc are zero (never written in this chunk, cleared after the last)
        // and y is finite there (zeroed before the first chunk), so both loops run over all 2 cap
        // columns with every LDS read issued up front: the same sums in the same order (the extra
        // terms add exact zeros), one LDS latency instead of one per column.
        if (tid < m && (tid >> 4) >= blo && (tid >> 4) <= bhi) {   // u-vector part: -(W y) at this thread's row
            // (in two halves: all 4 cap reads at once held 112 registers at the kernel's peak)
            double wsum = 0.0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                double wr[cap], yr[cap];
#pragma unroll
                for (int q = 0; q < cap; ++q) {
                    wr[q] = W[tid * WS + h * cap + q];
                    yr[q] = ybuf[h * cap + q];
                }
#pragma unroll
                for (int q = 0; q < cap; ++q) wsum += wr[q] * yr[q];
            }
            wacc -= wsum;
        }
        // W W^T, 4 columns per MFMA step: tile (bi, bj) of wave + 4 u; lane l feeds row 16 b + (l & 15),
        // column 4 st + (l >> 4) of W as A (block row bi) and as B (block row bj)
#pragma unroll
        for (int u = 0; u < kBlkTiles; ++u) {
            const int q = wave + 4 * u;
            int bi = 0;
            while ((bi + 1) * (bi + 2) / 2 <= q) ++bi;
            const int bj = q - bi * (bi + 1) / 2;
            if (q < ntiles && bi <= bhi && bj >= blo) {   // (uniform) tiles the chunk's W rows reach
                const int ra = min(16 * bi + (lane & 15), m - 1), rb = min(16 * bj + (lane & 15), m - 1);
                const bool oka = 16 * bi + (lane & 15) < m, okb = 16 * bj + (lane & 15) < m;
                double av[cap / 2], bv[cap / 2];
#pragma unroll
                for (int st = 0; st < cap / 2; ++st) {
                    const int cc = 4 * st + (lane >> 4);
                    av[st] = W[ra * WS + cc];
                    bv[st] = W[rb * WS + cc];
                }
#pragma unroll
                for (int st = 0; st < cap / 2; ++st)
                    if (4 * st < kc)   // (uniform)
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(oka ? av[st] : 0.0, okb ? bv[st] : 0.0, acc[u], 0, 0, 0);
            }
        }
#ifdef BOS_MF_BLK_FOLD_CYCLES
        const unsigned long long c3 = now();
#endif
        __syncthreads();
#ifdef BOS_MF_BLK_FOLD_CYCLES
        const unsigned long long c4 = now();
        BLK_CYC(0, c1 - c0); BLK_CYC(1, c2 - c1); BLK_CYC(2, c3 - c2); BLK_CYC(3, c4 - c3); BLK_CYC(4, 1);
#endif
        if (wave == 0 && lane < ncur) {   // clear this chunk's W entries (wave 0 writes the next chunk's after)
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                W[(pos + g) * WS + 2 * lml] = 0.0;
                W[(pos + g) * WS + 2 * lml + 1] = 0.0;
            }
        }
    };
    for (int ch = ch0; ch < ch1; ch += 2) {   // (uniform over the workgroup)
        chunk(ch, A, B);
        if (ch + 1 >= ch1) break;   // (a break: the loop's back edge always follows chunk ch + 1)
        chunk(ch + 1, B, A);
    }
#ifdef BOS_MF_BLK_FOLD_CYCLES
    if (tid == 0 && g_pivot_bwd)
        for (int i = 0; i < 5; ++i) g_pivot_bwd[8 * (int64_t)s + i] = cyc[i];
#endif
#undef BLK_CYC
    if (wave == 0 && nbad) atomicAdd(a.info, nbad);
}

template <bool F32>
__device__ __forceinline__ void factor_front_blk(const MfArgs& a, const int s, double* lds) {
    const int k = a.k[s], r = a.r[s], m = k + r;   // m <= kBlkMaxM (mf_create / the launch check it)
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    // LDS: the small buffers first (fixed, 16-byte aligned offsets), then the front
    double* colbuf = lds;                                             // panel pair broadcast (kBlkNb pairs)
    double* ybuf = colbuf + 2 * kBlkNb;                               // the fold's y of one chunk
    int* nlb = reinterpret_cast<int*>(ybuf + 2 * fold_chunk_landmarks(kBlkMaxM));   // chunk: landmarks, row blocks
    double* w = ybuf + 2 * fold_chunk_landmarks(kBlkMaxM) + 2;        // right-hand side, then the forward results
    double* F = w + kBlkMaxM;                                         // m x m, column-major
    static_assert((2 * kBlkNb + 2 * fold_chunk_landmarks(kBlkMaxM) + 2 + kBlkMaxM) % 2 == 0, "F 16-byte aligned");
    const int c0 = a.col0[s];
    const int nfold = a.fold_cnt[s];
    // the non-folded children (pose separators, typically 2): their update matrices and u-vectors,
    // with their positions in this front (emap), loaded now and in flight during the fold
    const int cb = a.child_ptr[s] + nfold, ce = a.child_ptr[s + 1];
    const int nx = min(ce - cb, kBlkXCh);
    double xv[kBlkXCh][kBlkXU], xuv[kBlkXCh];
    int xp[kBlkXCh][kBlkXU], xum[kBlkXCh], xne[kBlkXCh];
#pragma unroll
    for (int i = 0; i < kBlkXCh; ++i) {
        xne[i] = 0;
        if (i < nx) {   // uniform
            const int c = a.child[cb + i];
            const int rc = a.r[c], ne = rc * (rc + 1) / 2;
            xne[i] = ne;
            const double* Uc = a.U + a.U_off[c];
            const int16_t* ec = a.emap + a.emap_off[c];
#pragma unroll
            for (int u = 0; u < kBlkXU; ++u) {
                const int e = min(tid + kMfBlock * u, ne - 1);   // clamped (see assemble_wave)
                xv[i][u] = Uc[e];
                xp[i][u] = ec[e];
            }
            const int t = min(tid, rc - 1);
            xuv[i] = a.u[a.u_off[c] + t];
            xum[i] = tid < rc ? a.rmap[a.rmap_off[c] + t] : -1;
        }
    }
    // diagnostics (bos_debug_solver_stamps): the per-front phases of tools/solver_stamps.py
    auto stamp = [&](int q) {
        if (a.stamps_f && tid == 0) a.stamps_f[8 * (int64_t)s + q] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);
    double wacc = 0.0;
    if (nfold > 0) {
        // the folded landmarks first (their W uses F's LDS); F and w then start from minus their
        // contribution, each lower entry written once by the wave holding its tile
        dbl4 acc[kBlkTiles];
        fold_children_wg<F32>(a, s, F, ybuf, nlb, m, tid, acc, wacc);
        for (int e = tid; e < m * m; e += kMfBlock) F[e] = 0.0;
        __syncthreads();
        const int nbt = (m + 15) >> 4, ntiles = nbt * (nbt + 1) / 2;
#pragma unroll
        for (int u = 0; u < kBlkTiles; ++u) {
            const int q = wave + 4 * u;
            if (q < ntiles) {
                int bi = 0;
                while ((bi + 1) * (bi + 2) / 2 <= q) ++bi;
                const int bj = q - bi * (bi + 1) / 2;
                const int j = 16 * bj + (lane & 15);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 16 * bi + (lane >> 4) + 4 * e;
                    if (i < m && j <= i) F[i + j * m] = -acc[u][e];
                }
            }
        }
    } else {
        for (int e = tid; e < m * m; e += kMfBlock) F[e] = 0.0;
    }
    if (tid < m) w[tid] = (tid < k ? a.x[c0 + tid] : 0.0) + wacc;   // (m <= kBlkMaxM < kMfBlock)
    __syncthreads();
    stamp(1);
    for (int q = a.amap_ptr[s] + tid; q < a.amap_ptr[s + 1]; q += kMfBlock) F[a.amap_dst[q]] += a.A[a.amap_src[q]];
    __syncthreads();
    stamp(2);
    stamp(3);
    // the other children one at a time (deterministic): update matrix into F, u-vector into w
#pragma unroll
    for (int i = 0; i < kBlkXCh; ++i) {
        if (i < nx) {   // uniform
#pragma unroll
            for (int u = 0; u < kBlkXU; ++u)
                if (tid + kMfBlock * u < xne[i]) F[xp[i][u]] += xv[i][u];
            if (xum[i] >= 0) w[xum[i]] += xuv[i];
            if (xne[i] > kMfBlock * kBlkXU) {   // entries past the prefetched ones (r > 63)
                const int c = a.child[cb + i];
                const double* Uc = a.U + a.U_off[c];
                const int16_t* ec = a.emap + a.emap_off[c];
                for (int e = kMfBlock * kBlkXU + tid; e < xne[i]; e += kMfBlock) F[ec[e]] += Uc[e];
            }
            __syncthreads();
        }
    }
    for (int ci = cb + nx; ci < ce; ++ci) {
        const int c = a.child[ci];
        const int rc = a.r[c];
        const int32_t* map = a.rmap + a.rmap_off[c];
        const double* Uc = a.U + a.U_off[c];
        for (int j = wave; j < rc; j += kMfBlock / 64) {
            const int pj = map[j] * m;
            const double* uj = Uc + pk(j, j, rc) - j;
            for (int i = j + lane; i < rc; i += 64) F[map[i] + pj] += uj[i];
        }
        const double* uc = a.u + a.u_off[c];
        for (int t = tid; t < rc; t += kMfBlock) w[map[t]] += uc[t];
        __syncthreads();
    }
    stamp(4);
    double* Ls = a.L + a.L_off[s];
    int nbad = 0;
    for (int p0 = 0; p0 < k; p0 += kBlkNb) {
        const int nb = min(kBlkNb, k - p0);
        if (wave == 0) {
            // lane l holds rows p0 + l and p0 + 64 + l of the panel's columns (m - p0 <= 128 rows); the
            // reads are clamped to valid positions (one wait for all), the values past the front zero.
            // Columns past nb hold copies of column nb - 1: updated like the others, never a pivot,
            // never stored.
            const int ia = p0 + lane, ib = p0 + 64 + lane;
            const bool va = ia < m, vb = ib < m;
            const int ra = min(ia, m - 1), rb = min(ib, m - 1);
            double pa[kBlkNb], pb[kBlkNb];
#pragma unroll
            for (int c = 0; c < kBlkNb; ++c) {
                const int cc = p0 + min(c, nb - 1);
                pa[c] = F[ra + cc * m];
                pb[c] = F[rb + cc * m];
            }
            asm volatile("" : "+v"(pa[0]), "+v"(pb[0]));
#pragma unroll
            for (int c = 0; c < kBlkNb; ++c) {
                pa[c] = va ? pa[c] : 0.0;
                pb[c] = vb ? pb[c] : 0.0;
            }
            double wa = va ? w[ia] : 0.0, wb = vb ? w[ib] : 0.0;
            // two pivots per step (as factor_front_reg): column j + 1 brought up to date in registers,
            // both columns' panel rows through ONE LDS broadcast as pairs, then a rank-2 update
#pragma unroll
            for (int j = 0; j < kBlkNb; j += 2) {
                if (j + 1 < nb) {   // uniform
                    double d0 = readlane_d(pa[j], j);
                    const bool bad0 = !(d0 > 0.0);
                    nbad += bad0;
                    d0 = bad0 ? 1e-300 : d0;
                    const double inv0 = rsqrt_nr(d0), l00 = d0 * inv0;
                    const double la0 = lane < j ? 0.0 : lane == j ? l00 : pa[j] * inv0;   // L[i, p0 + j]
                    const double lb0 = pb[j] * inv0;
                    const double lj1 = readlane_d(la0, j + 1);                           // L[p0 + j + 1, p0 + j]
                    const double fa = fma(-la0, lj1, pa[j + 1]), fb = fma(-lb0, lj1, pb[j + 1]);
                    double d1 = readlane_d(fa, j + 1);
                    const bool bad1 = !(d1 > 0.0);
                    nbad += bad1;
                    d1 = bad1 ? 1e-300 : d1;
                    const double inv1 = rsqrt_nr(d1), l11 = d1 * inv1;
                    const double la1 = lane < j + 1 ? 0.0 : lane == j + 1 ? l11 : fa * inv1;
                    const double lb1 = fb * inv1;
                    pa[j] = la0;
                    pb[j] = lb0;
                    pa[j + 1] = la1;
                    pb[j + 1] = lb1;
                    if (lane < kBlkNb) reinterpret_cast<double2*>(colbuf)[lane] = make_double2(la0, la1);
                    const double y0 = readlane_d(wa, j) * inv0;   // forward steps
                    wa = lane == j ? y0 : lane > j ? fma(-la0, y0, wa) : wa;
                    wb = fma(-lb0, y0, wb);
                    const double y1 = readlane_d(wa, j + 1) * inv1;
                    wa = lane == j + 1 ? y1 : lane > j + 1 ? fma(-la1, y1, wa) : wa;
                    wb = fma(-lb1, y1, wb);
                    wave_sync();
                    double2 cbv[kBlkNb];
#pragma unroll
                    for (int c = j + 2; c < kBlkNb; ++c) cbv[c] = reinterpret_cast<const double2*>(colbuf)[c];
#pragma unroll
                    for (int c = j + 2; c < kBlkNb; ++c) {
                        pa[c] = fma(-la1, cbv[c].y, fma(-la0, cbv[c].x, pa[c]));
                        pb[c] = fma(-lb1, cbv[c].y, fma(-lb0, cbv[c].x, pb[c]));
                    }
                    __builtin_amdgcn_wave_barrier();   // the next step's broadcast stays after these reads
                } else if (j < nb) {   // the panel's last column (odd nb): nothing left to update
                    double d = readlane_d(pa[j], j);
                    const bool bad = !(d > 0.0);
                    nbad += bad;
                    d = bad ? 1e-300 : d;
                    const double inv = rsqrt_nr(d), ljj = d * inv;
                    const double la = lane < j ? 0.0 : lane == j ? ljj : pa[j] * inv;
                    const double lb = pb[j] * inv;
                    pa[j] = la;
                    pb[j] = lb;
                    const double y = readlane_d(wa, j) * inv;
                    wa = lane == j ? y : lane > j ? fma(-la, y, wa) : wa;
                    wb = fma(-lb, y, wb);
                }
            }
#pragma unroll
            for (int c = 0; c < kBlkNb; ++c) {
                if (c < nb) {
                    if (va) {
                        F[ia + (p0 + c) * m] = pa[c];
                        ST_L(Ls, ia + (p0 + c) * m, pa[c]);
                    }
                    if (vb) {
                        F[ib + (p0 + c) * m] = pb[c];
                        ST_L(Ls, ib + (p0 + c) * m, pb[c]);
                    }
                }
            }
            if (va) w[ia] = wa;
            if (vb) w[ib] = wb;
        }
        __syncthreads();
        // trailing lower triangle, rows / columns [t0, m): 16 x 16 tiles (bi >= bj) over the waves
        const int t0 = p0 + nb, nbt = (m - t0 + 15) >> 4, ntiles = nbt * (nbt + 1) / 2;
        for (int q = wave; q < ntiles; q += kMfBlock / 64) {
            int bi = 0;
            while ((bi + 1) * (bi + 2) / 2 <= q) ++bi;
            const int bj = q - bi * (bi + 1) / 2;
            const int ra = t0 + 16 * bi + (lane & 15), rb = t0 + 16 * bj + (lane & 15);
            dbl4 acc = {0.0, 0.0, 0.0, 0.0};
            // every operand read issued up front (clamped positions, masked values), then the MFMAs
            double av[kBlkNb / 4], bv[kBlkNb / 4];
#pragma unroll
            for (int st = 0; st < kBlkNb / 4; ++st) {
                const int cc = min(4 * st + (lane >> 4), nb - 1);
                av[st] = F[min(ra, m - 1) + (p0 + cc) * m];
                bv[st] = F[min(rb, m - 1) + (p0 + cc) * m];
            }
#pragma unroll
            for (int st = 0; st < kBlkNb / 4; ++st) {
                if (4 * st < nb) {   // (uniform)
                    const bool okc = 4 * st + (lane >> 4) < nb;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(okc && ra < m ? av[st] : 0.0, okc && rb < m ? bv[st] : 0.0,
                                                               acc, 0, 0, 0);
                }
            }
            const int col = t0 + 16 * bj + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = t0 + 16 * bi + (lane >> 4) + 4 * e;
                if (row < m && row >= col) F[row + col * m] -= acc[e];
            }
        }
        __syncthreads();
    }
    stamp(5);
    if (tid == 0 && nbad) atomicAdd(a.info, nbad);
    // the update matrix (packed lower r x r), the forward results: own dofs to x, the rest to u
    double* Us = a.U + a.U_off[s];
    for (int j = wave; j < r; j += kMfBlock / 64) {
        double* uj = Us + pk(j, j, r) - j;
        const double* fj = F + (k + (k + j) * m);
        for (int i = j + lane; i < r; i += 64) uj[i] = fj[i];
    }
    for (int i = tid; i < m; i += kMfBlock) {
        if (i < k) a.x[c0 + i] = w[i];
        else a.u[a.u_off[s] + (i - k)] = w[i];
    }
    stamp(6);
}

template <bool F32>
__global__ __launch_bounds__(kMfBlock) void mf_factor_blk(const MfArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    factor_front_blk<F32>(a, a.level[blockIdx.x], lds);
}

}  // namespace

}  // namespace dev
}  // namespace bos
