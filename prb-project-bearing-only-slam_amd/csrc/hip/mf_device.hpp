// Device primitives every multifrontal kernel family shares (hip/multifrontal.hip is the translation
// unit): the kernel argument block, packed-front indexing, the L panel cache policy, coherent and
// tagged hand-off accesses, the wave assembly of H, the pivot reciprocal root and the diagnostic stamps.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bos {
namespace dev {

namespace {

constexpr int kMfBlock = 256;
#ifdef BOS_MF_PIVOT_CYCLES
__device__ unsigned long long* g_pivot_bwd;   // diagnostic build: the stamp buffer's backward half
#endif

// Structure arrays carry kMfPad zeroed elements after their end: the kernels read clamped indices
// unconditionally (branch-free loads, see assemble_wave) and may touch up to one chunk / 64 lanes past
// a range's last element.
constexpr int64_t kMfPad = 64;

__device__ __forceinline__ int64_t pk(int64_t i, int64_t j, int64_t m) { return j * m - j * (j - 1) / 2 + (i - j); }
__device__ __forceinline__ int pk32(int i, int j, int m) { return j * m - j * (j - 1) / 2 + (i - j); }   // LDS fronts

// L panel traffic (written by the factorization, read once by the backward substitution): the
// stores are non-temporal, so the solve's ~300 MB of L stream past the caches instead of evicting the
// next J+H build's inputs (in-step J+H 16.0-16.5 -> 13.2-14.5 us, solve -14 us; plain stores and
// loads: profiles/r05_ntl_lds_ab.txt). The backward launches' panel loads are non-temporal too (plain
// loads measured slower), except the folded landmarks' backward launch, which reads its L columns
// with plain loads (non-temporal there: solve +13 us, profiles/r05_fold_l_policy_ab.txt).
#define ST_L(p, i, v) __builtin_nontemporal_store((v), (p) + (i))
#define LD_L(p, i) __builtin_nontemporal_load((p) + (i))
#define ST_LF(p, i, v) ST_L(p, i, v)
#define LD_LF(p, i) ((p)[i])

// Hand-off data between fronts processed in one dataflow launch (update matrices, forward
// u-vectors, backward x rows) is written and read with relaxed agent-scope atomics (coherent sc1
// accesses) so no L2-wide release/acquire fence is needed per front; COH = false is plain access.
template <bool COH> __device__ __forceinline__ double ldc(const double* p) {
    if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool COH> __device__ __forceinline__ void stc(double* p, double v) {
    if constexpr (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// Tagged granules (cdna_hip_programming.md §6 Guideline 16, R2: the data is the flag). A double
// travels as two 8-byte granules {epoch, 32 bits of it}, each written by one relaxed agent-scope
// atomic store (sc1, write-through) and read by relaxed agent-scope atomic loads (sc1): a consumer
// that sees the step's epoch in both tags holds the value, with no flag, no drain of the producer's
// stores and no second load round trip. The epoch is the GN step's (never 0, bumped per step), so
// granules of earlier steps never match.
__device__ __forceinline__ void tag_pair(unsigned long long* g, double v, uint32_t epoch) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v), t = (unsigned long long)epoch << 32;
    __hip_atomic_store(g, t | (b & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, t | (b >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one read of a tagged pair: *ok &= both tags current; the value assembled from the halves
__device__ __forceinline__ double untag_pair(const unsigned long long* g, uint32_t epoch, bool& ok) {
    const unsigned long long lo = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ok = ok && (uint32_t)(lo >> 32) == epoch && (uint32_t)(hi >> 32) == epoch;
    return __longlong_as_double((long long)((hi << 32) | (lo & 0xffffffffull)));
}

struct MfArgs {
    const int32_t* level;        // supernode ids of this level
    int count;
    const int32_t* col0;
    const int32_t* k;
    const int32_t* r;
    const int64_t* L_off;
    const int64_t* U_off;
    const int64_t* u_off;
    const int64_t* scratch_off;  // -1 => LDS
    const int32_t* child_ptr;
    const int32_t* child;
    const int64_t* rmap_off;
    const int32_t* rmap;
    const int32_t* amap_ptr;
    const int32_t* amap_src;
    const int32_t* amap_dst;
    const int64_t* findex_off;
    const int32_t* findex;
    const double* A;             // CSR values of H (fp64)
    const float* A32;            // fp32 block array the fold reads instead of A (see mf_set_fold_source),
    int64_t pl_lo;               // and where its factored pose-landmark region starts; A32 null otherwise
    double* L;
    double* U;
    double* u;
    double* scratch;
    double* x;                   // rhs in, solution out (permuted order)
    int32_t* info;               // count of non-positive pivots
    const int32_t* fold_cnt;     // folded landmark children (Schur ordering, see plan.hpp)
    const int32_t* fold_cptr;
    const int32_t* fold_chunk;
    const int32_t* fold_rec;
    const int16_t* emap;            // extend-add positions: entry e of child c's packed update matrix goes to
    const int64_t* emap_off;        // packed position emap[emap_off[c] + e] of its parent's front (wave fronts)
    unsigned long long* stamps_f;   // diagnostics (mf_debug_set_stamps): factor / backward stamps, or null
    unsigned long long* stamps_b;
    // tagged hand-offs inside a dataflow launch (tag_pair / sweep): a flow front whose parent is in
    // the same flow publishes its update matrix and u-vector as tagged granules at Ug + ug_off[s]
    // (-1: plain U / u); every backward front publishes its solved x as tagged granules xg[2 dof]
    unsigned long long* Ug;
    const int64_t* ug_off;
    unsigned long long* xg;
    const int8_t* xtag;             // per supernode: its x is read by a backward flow front (write xg)
    const uint32_t* epoch;          // the GN step's epoch (device word, mf_epoch_ptr)
};

typedef double dbl4 __attribute__((ext_vector_type(4)));   // one lane's part of an f64 MFMA accumulator

// Assembly of H entries into a front by one wavefront (F[dst] = A[src], or += when the front
// already holds the folded landmarks' part), 4 entries per lane in flight: index loads, then value
// gathers, then LDS stores. Loads past the front's range are clamped to its last entry instead of
// predicated: a predicated load becomes a branch with the load's wait inside it, which serialises
// the four loads (one memory latency each instead of one for all four).
__device__ __forceinline__ void assemble_wave(const MfArgs& a, int q0_, int q1, double* F, int lane, bool add) {
    for (int q0 = q0_; q0 < q1; q0 += 256) {
        int src[4], dst[4];
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = min(q0 + 64 * u + lane, q1 - 1);
            src[u] = a.amap_src[q];
            dst[u] = a.amap_dst[q];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = a.A[src[u]];
        if (add) {   // (uniform) the four front entries read at once, as in extend_child
            double f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = F[dst[u]];
            asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] += f[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q0 + 64 * u + lane < q1) F[dst[u]] = v[u];
    }
}

// 1 / sqrt(d) for d > 0 in the normal range: hardware estimate refined by two Newton steps
// (quadratic convergence: full double precision, within an ulp or two of 1.0 / sqrt(d)).
__device__ __forceinline__ double rsqrt_nr(double d) {
    double y = __builtin_amdgcn_rsq(d);
    const double h = 0.5 * d;
    y = y * fma(-h * y, y, 1.5);
    y = y * fma(-h * y, y, 1.5);
    return y;
}

// phase stamp k of front s (lane 0; the product launches pass no stamp buffer)
__device__ __forceinline__ void fstamp(unsigned long long* stp, int s, int k) {
#ifdef BOS_MF_PIVOT_CYCLES
    if (stp && stp == g_pivot_bwd) return;   // the backward half holds the pivot-loop cycle stamps
#endif
    if (stp && (threadIdx.x & 63) == 0) stp[8 * (int64_t)s + k] = __builtin_amdgcn_s_memrealtime();
}
#ifdef BOS_MF_PIVOT_CYCLES
// Diagnostic build only (tools/pivot_cycles.py): core-clock stamps of every front in the backward
// half of the stamp buffer: [1] children ready, [2] their values loaded, [3] extend-added, [0] pivot
// loop start (rows in registers), [4..6] after two-pivot steps 1-3, [7] pivot loop end.
__device__ __forceinline__ void cstamp(unsigned long long* stpb, int s, int k) {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (stpb && (threadIdx.x & 63) == 0) stpb[8 * (int64_t)s + k] = t;
}
#endif

}  // namespace

}  // namespace dev
}  // namespace bos
