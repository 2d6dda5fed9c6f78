// The wave fold: a wave front's folded landmark children (Schur ordering) eliminated by the front's own
// wavefront before its assembly. Shared by every wave-front kernel (mf_wave.hpp); the blocked kernel's
// workgroup form (mf_blk.hpp fold_children_wg) reuses the records, values and chunk table.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../host/plan.hpp"
#include "mf_device.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

// LDS of one wave's fold chunk: the y (forward-step) values of its landmarks, two per landmark
struct FoldBuf {
    double y[2 * fold_chunk_landmarks(kMfWaveMaxM)];
};

// The folded landmarks' contribution to the front, lower 16 x 16 blocks of W W^T (f64 MFMA
// accumulators: lane l holds rows (l >> 4) + 4 v, column l & 15 of each block) and, per
// position lane, the u-vector part -W y.
template <int MAXM>
struct FoldAcc {
    static constexpr int NB = (MAXM + 15) / 16, NP = NB * (NB + 1) / 2;
    dbl4 d[NP];
    double w;
};

// Folded landmark children (Schur ordering) of front s, eliminated by its wave: per chunk (whole
// children, <= 64 row groups, <= fold_chunk_landmarks(m) landmarks) lane q takes one observing pose
// of landmark c — its 3 rows t, t + 1, t + 2 (one 32-byte record: sources of the pose-landmark
// block and of the landmark's 2 x 2 block, the landmark's col0 / r / L offset, the rows' first
// position in this front and c's index in the chunk), factors the 2 x 2 block, forms L[t + g,
// 0..1], the landmark's forward step y, and writes the landmark's L panel and y. The rows also form
// the chunk's W (front position x 2 columns per landmark, in LDS that the front's F uses later) and
// its y; W W^T accumulates in f64 MFMA registers (the landmarks' update matrices -L21 L21^T,
// summed) and -W y in the position lanes (their u-vectors). The caller subtracts both once the
// front is assembled. Nothing goes through global memory and the result is deterministic.
__device__ __forceinline__ int4 fold_rec_load(const MfArgs& a, int q, int half) {
    return reinterpret_cast<const int4*>(a.fold_rec + (int64_t)kFoldRec * q)[half];
}

// The values one chunk's row groups need (the pose-landmark block, 3 x 2, the landmark's 2 x 2
// block and right-hand side), gathered for chunk c + 1 while chunk c is processed.
struct FoldVals {
    double h[6];   // (row g, column j) at 2 g + j
    double a00, a10, a11, x0, x1;
};
// The same from the fp32 build (F32: mf_set_fold_source): the bearing's factored block (J_theta,
// J_lx, J_ly) and the landmark's 2 x 2 block as loaded, and the entries' presence in flags;
// fold_decode forms the doubles the fp64 copy would hold (products in fp32, as
// gather_f64_factored_kernel expands them), so the result is bit-identical.
struct FoldVals32 {
    float jt, jx, jy, a00, a10, a11;
    int flags;   // block present << 0 | a00, a10, a11 present << 2, 3, 4
    double x0, x1;
};
// The fp64 build's values as loaded and their presence in flags (as FoldVals32): the selects are
// applied by fold_decode when the chunk is processed, so the loads stay in flight until then (a
// select right after the loads made the wave wait for them in the chunk that issued them, one
// memory latency per chunk: config 2's blocked-front folds, 33 us at level 0)
struct FoldVals64 {
    double h[6], a00, a10, a11, x0, x1;
    int flags;   // block present << 0 | a00, a10, a11 present << 2, 3, 4
};
template <bool F32> using FoldValsT = typename std::conditional<F32, FoldVals32, FoldVals64>::type;

__device__ __forceinline__ FoldVals fold_decode(const FoldVals64& v) {
    FoldVals d;
    const bool blk = v.flags & 1;
#pragma unroll
    for (int e = 0; e < 6; ++e) d.h[e] = blk ? v.h[e] : 0.0;
    d.a00 = (v.flags & 4) ? v.a00 : 0.0;
    d.a10 = (v.flags & 8) ? v.a10 : 0.0;
    d.a11 = (v.flags & 16) ? v.a11 : 0.0;
    d.x0 = v.x0;
    d.x1 = v.x1;
    return d;
}
__device__ __forceinline__ FoldVals fold_decode(const FoldVals32& v) {
    FoldVals d;
    const bool blk = v.flags & 1;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const float p = g == 0 ? -v.jx : g == 1 ? -v.jy : v.jt;   // J_p = (-J_lx, -J_ly, J_theta)
        d.h[2 * g] = blk ? (double)(p * v.jx) : 0.0;
        d.h[2 * g + 1] = blk ? (double)(p * v.jy) : 0.0;
    }
    d.a00 = (v.flags & 4) ? (double)v.a00 : 0.0;
    d.a10 = (v.flags & 8) ? (double)v.a10 : 0.0;
    d.a11 = (v.flags & 16) ? (double)v.a11 : 0.0;
    d.x0 = v.x0;
    d.x1 = v.x1;
    return d;
}

template <bool F32>
__device__ __forceinline__ FoldValsT<F32> fold_vals(const MfArgs& a, const int4& r0, const int4& r1, bool mine) {
    if constexpr (F32) {
        // records index the fp64 layout: the block of slot q at pl_lo + 6 q, held factored at
        // pl_lo + 3 q of the fp32 array (mf_set_fold_source checked the records)
        const int q = max(r0.x - (int)a.pl_lo, 0) / 6;
        const float* f = a.A32 + a.pl_lo + 3 * (int64_t)q;
        FoldVals32 v;
        v.jt = f[0];
        v.jx = f[1];
        v.jy = f[2];
        v.a00 = a.A32[max(r0.z, 0)];
        v.a10 = a.A32[max(r0.w, 0)];
        v.a11 = a.A32[max(r1.x, 0)];
        v.x0 = a.x[r1.y];   // (a lane past the chunk's groups reads its last group's: see fold_chunk)
        v.x1 = a.x[r1.y + 1];
        v.flags = (r0.x >= 0 ? 1 : 0) | (r0.z >= 0 ? 4 : 0) | (r0.w >= 0 ? 8 : 0) | (r1.x >= 0 ? 16 : 0);
        return v;
    } else {
    // every load unconditional (indices clamped to valid ones), the value selected afterwards: a
    // predicated load would be a branch with its wait inside, and the next chunk's values must stay
    // in flight while the current chunk is processed
    // (selected by fold_decode, see FoldVals64)
    const int b = max(r0.x, 0);
    FoldVals64 v;
#pragma unroll
    for (int e = 0; e < 6; ++e) v.h[e] = a.A[b + e];
    v.a00 = a.A[max(r0.z, 0)];
    v.a10 = a.A[max(r0.w, 0)];
    v.a11 = a.A[max(r1.x, 0)];
    v.x0 = a.x[r1.y];   // (lanes past the groups: their last group's)
    v.x1 = a.x[r1.y + 1];
    v.flags = (r0.x >= 0 ? 1 : 0) | (r0.z >= 0 ? 4 : 0) | (r0.w >= 0 ? 8 : 0) | (r1.x >= 0 ? 16 : 0);
    return v;
    }
}

// The chunk boundaries of a front (fold_chunk[c], c uniform) from one register holding 64 of them
// (lane i: fold_chunk[base + i]), re-read only when a front has more chunks than that: the loop then
// needs no dependent load per chunk (a vector load whose value decides the next loads would make
// the wave wait for every load issued before it, the prefetched values included).
struct ChunkTable {
    int base, v;
    __device__ __forceinline__ void load(const MfArgs& a, int b, int lane) {
        base = b;
        v = a.fold_chunk[b + lane];   // padded array (kMfPad): in bounds
    }
    // the same inside the chunk loop, waited for on the spot: a load left pending on this rarely taken
    // path would make the compiler wait for every outstanding load at the loop's top on every path
    __device__ __forceinline__ void reload(const MfArgs& a, int b, int lane) {
        load(a, b, lane);
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) (expcnt, lgkmcnt: no wait)
    }
    // fold_chunk[c] for c in [base, base + 64)
    __device__ __forceinline__ int at(int c) const { return __builtin_amdgcn_readlane(v, c - base); }
};

// One fold chunk's elimination (values v, records' meta q1, n rows): the landmarks' 2 x 2 factors, L
// panels and forward steps, the chunk's W in LDS, and W W^T / -W y accumulated.
template <int MAXM, typename VALS>
__device__ __forceinline__ void fold_chunk(const MfArgs& a, double* W, FoldBuf* fb, int m, int lane,
                                           FoldAcc<MAXM>& acc, const VALS& vraw, const int4& q1, int n,
                                           bool first, int s, int& nbad) {
    const FoldVals v = fold_decode(vraw);
    constexpr int NB = FoldAcc<MAXM>::NB;
    constexpr int WS = 2 * fold_chunk_landmarks(MAXM) + 1;   // W row stride (odd: no bank conflicts)
    const int nbm = (m + 15) >> 4;
    const int t = q1.z & 63, rc = (q1.z >> 6) & 63, pos = (q1.z >> kFoldPosShift) & kFoldPosMask,
              lml = (q1.z >> kFoldLmShift) & 63;
    const bool mine = lane < n;
    const int nl = __builtin_amdgcn_readlane(lml, n - 1) + 1;   // landmarks of this chunk
    const int col0 = q1.y;
    const int64_t loff = q1.w;
    // Every lane issues the same global stores: a store under a divergent branch leaves the number of
    // memory operations after the next chunk's loads unknown to the compiler, which then waits for
    // all of them (vmcnt(0)) at the top of every chunk instead of for the loads alone. A lane past
    // the chunk's rows holds the record and values of its last row, and every row of a landmark the
    // landmark's values, so the extra stores write the owners' values, bit for bit, to the owners'
    // addresses (a shared sink instead was measured 17 us slower: every wave of the GPU wrote the
    // same lines).
    {
        double d0 = v.a00;
        const bool bad0 = !(d0 > 0.0);
        d0 = bad0 ? 1e-300 : d0;
        const double i0 = rsqrt_nr(d0), l00 = d0 * i0;
        const double l10 = v.a10 * i0;
        double d1 = v.a11 - l10 * l10;
        const bool bad1 = !(d1 > 0.0);
        d1 = bad1 ? 1e-300 : d1;
        const double i1 = rsqrt_nr(d1), l11 = d1 * i1;
        const double y0 = v.x0 * i0, y1 = (v.x1 - l10 * y0) * i1;
        const int mc = 2 + rc;
        double* Lc = a.L + loff;
        const bool head = mine && t == 0;
        double lt0[3], lt1[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            lt0[g] = v.h[2 * g] * i0;
            lt1[g] = (v.h[2 * g + 1] - lt0[g] * l10) * i1;
            ST_LF(Lc, 2 + t + g, lt0[g]);
            ST_LF(Lc, mc + 2 + t + g, lt1[g]);
        }
        ST_LF(Lc, 0, l00);
        ST_LF(Lc, 1, l10);
        ST_LF(Lc, mc + 1, l11);
        a.x[col0] = y0;
        a.x[col0 + 1] = y1;
        nbad += head ? (int)bad0 + (int)bad1 : 0;
        if (head) {
            fb->y[2 * lml] = y0;
            fb->y[2 * lml + 1] = y1;
        }
        if (mine) {
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                W[(pos + g) * WS + 2 * lml] = lt0[g];
                W[(pos + g) * WS + 2 * lml + 1] = lt1[g];
            }
        }
    }
    wave_sync();
    const int kc = 2 * nl;
    if (lane < m) {   // u-vector part: -(W y) at this lane's position
        double w = 0.0;
        for (int q = 0; q < kc; ++q) w += W[lane * WS + q] * fb->y[q];
        acc.w -= w;
    }
    // W W^T, 4 columns per MFMA step; lane l feeds row 16 b + (l & 15), column 4 st + (l >> 4)
    // of W to the blocks of row b (as A) and of column b (as B, the same values)
    for (int st = 0; 4 * st < kc; ++st) {
        double av[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) av[b] = b < nbm ? W[(16 * b + (lane & 15)) * WS + 4 * st + (lane >> 4)] : 0.0;
        int q = 0;
#pragma unroll
        for (int bi = 0; bi < NB; ++bi)
#pragma unroll
            for (int bj = 0; bj <= bi; ++bj, ++q)
                if (bi < nbm) acc.d[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[bi], av[bj], acc.d[q], 0, 0, 0);
    }
    wave_sync();
    if (mine) {   // clear this chunk's W entries for the next chunk
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            W[(pos + g) * WS + 2 * lml] = 0.0;
            W[(pos + g) * WS + 2 * lml + 1] = 0.0;
        }
    }
    wave_sync();
}

template <int MAXM, bool F32>
__device__ __forceinline__ void fold_children(const MfArgs& a, int s, double* W, FoldBuf* fb, int m, int lane,
                                              FoldAcc<MAXM>& acc) {
    constexpr int WS = 2 * fold_chunk_landmarks(MAXM) + 1;
    static_assert(MAXM * WS <= MAXM * (MAXM + 1) / 2, "W fits the front's LDS triangle");
    static_assert(fold_chunk_landmarks(MAXM) % 2 == 0, "the W W^T steps (4 columns) stay inside W's rows");
#pragma unroll
    for (int q = 0; q < FoldAcc<MAXM>::NP; ++q) acc.d[q] = dbl4{0.0, 0.0, 0.0, 0.0};
    acc.w = 0.0;
    for (int e = lane; e < MAXM * WS; e += 64) W[e] = 0.0;
    const int ch0 = a.fold_cptr[s], ch1 = a.fold_cptr[s + 1];
    int nbad = 0;   // non-positive 2 x 2 pivots of the folded landmarks (head lanes)
    ChunkTable tb;
    tb.load(a, ch0, lane);
    // chunk c: rows [at(c), at(c + 1)); records of a lane past the chunk's rows (or of a chunk past
    // the front's last) are read at a valid index and never used
    auto rec = [&](int c, int n, int4& q0, int4& q1) {
        const int q = tb.at(c) + min(lane, max(n - 1, 0));
        q0 = fold_rec_load(a, q, 0);
        q1 = fold_rec_load(a, q, 1);
    };
    auto len = [&](int c) { return c < ch1 ? tb.at(c + 1) - tb.at(c) : 0; };
    int n = len(ch0);
    int4 r0, r1;
    rec(ch0, n, r0, r1);
    FoldValsT<F32> v = fold_vals<F32>(a, r0, r1, lane < n);
    // next chunk's records, then (inside the loop) its values, both one chunk ahead
    int nn = len(ch0 + 1);
    int4 n0, n1;
    rec(ch0 + 1, nn, n0, n1);
    // Wait for the prologue's loads here: the loop's top then needs no wait on either path (from the
    // back edge, the next chunk's records precede only the last chunk's stores). Left to the
    // compiler, the top waits for every outstanding load and store (vmcnt(0)) because on the entry
    // path the records are the last loads issued.
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    for (int ch = ch0; ch < ch1; ++ch) {
        if (ch + 3 - tb.base > 63) tb.reload(a, ch, lane);   // (uniform; fronts with > 60 chunks only)
        const FoldValsT<F32> cur = v;
        const int4 q1 = r1;
        const int ncur = n;
        // chunk ch + 1: values now (its records arrived during chunk ch - 1), records of ch + 2
        v = fold_vals<F32>(a, n0, n1, lane < nn);
        r0 = n0;
        r1 = n1;
        const int n2 = len(ch + 2);
        rec(ch + 2, n2, n0, n1);
        fold_chunk<MAXM>(a, W, fb, m, lane, acc, cur, q1, ncur, ch == ch0, s, nbad);
        n = nn;
        nn = n2;
    }
    if (nbad) atomicAdd(a.info, nbad);
}

// The front before its assembly: every lower entry of F and of wv set to minus the folded
// landmarks' contribution (each entry once).
template <int MAXM>
__device__ __forceinline__ void fold_store(const FoldAcc<MAXM>& acc, double* F, double* wv, int m, int lane) {
    constexpr int NB = FoldAcc<MAXM>::NB;
    const int nbm = (m + 15) >> 4;
    int q = 0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
        for (int bj = 0; bj <= bi; ++bj, ++q) {
            if (bi < nbm) {
                const int j = 16 * bj + (lane & 15);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 16 * bi + (lane >> 4) + 4 * e;
                    if (i < m && j <= i) F[pk32(i, j, m)] = -acc.d[q][e];
                }
            }
        }
    if (lane < m) wv[lane] = acc.w;
}

}  // namespace

}  // namespace dev
}  // namespace bos
