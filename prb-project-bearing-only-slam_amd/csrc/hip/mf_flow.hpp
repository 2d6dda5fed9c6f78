// The hand-off between fronts: the dataflow launches' ticket queue and bounded waits, and the children's
// extend-add inputs (plain from earlier launches, tagged granules inside a flow) that every wave-front
// kernel (mf_wave.hpp) and the backward flow (mf_backward.hpp) build on.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mf_device.hpp"
#include "multifrontal.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

// ---- dataflow (work-queue) kernels: one launch walks a whole tree range. A wavefront takes the
// next front from an atomic ticket (fronts listed in topological order), prepares what does not
// depend on other fronts (the fold and the assembly of H), waits for the fronts it depends on
// (children bottom-up, the parent top-down) by polling their tagged hand-off data (tag_pair /
// untag_pair: the data is the flag), processes the front and writes its own hand-off data tagged.
// A wave only ever waits for tickets already taken by running waves, so any grid size is
// deadlock-free. Every wait is bounded in time: a dependency that has not arrived within 50 ms marks
// the launch stalled (kStall in info), and from then on every wait of every wave returns at once, so
// a stalled launch drains in about one timeout and is reported as an error (bos_step returns
// BOS_ERR_SOLVER and the box-plus is skipped), never a hang.
// The ticket is reset by the launch itself: the last wave to leave zeroes it (and its exit
// counter), so no host-side reset is needed between launches and no error path can leave a
// partly consumed ticket behind (a launch that never started never took one).
struct Flow {
    const int32_t* order;   // fronts in processing order
    int n;
    int* ticket;            // zero at launch; zeroed again by the launch's last wave
    int* exits;             // waves that have left the launch (same life cycle)
    const uint32_t* epoch_src;   // device word: this step's epoch (bumped once per GN step by the
                                 // step_mark kernel before the first flow launch, mf_epoch_ptr)
    uint32_t epoch;              // *epoch_src, read by the launch itself (graph-replayable)
    const int8_t* fid;      // per supernode: the flow launch (id) that processes it, 0 = none; a front
                            // waits only for fronts of its own launch (the others finished earlier:
                            // per-level launches, the other program, or another rank's exchange)
    int id;
    unsigned long long* stamps;   // diagnostics (bos_debug_solver_stamps): 8 realtime stamps per front, or null
};

// Front-processing modes: per-level launch (no waits), dataflow launch (flags in global memory,
// coherent hand-off). (A third, the tree's top as one workgroup with flags in LDS, measured slower
// than the flows: DESIGN.md §4.)
constexpr int kModeLevel = 0, kModeFlow = 1;

constexpr int kStall = kMfStall;               // or-ed into info when a dependency wait times out
constexpr uint64_t kWaitTicks = 5000000;        // 50 ms of the 100 MHz realtime clock

__device__ __forceinline__ int next_ticket(int* ticket) {
    int t = 0;
    if (threadIdx.x == 0) t = atomicAdd(ticket, 1);
    return __builtin_amdgcn_readfirstlane(t);
}

// Memory ordering of the in-launch hand-off (the form cdna_hip_programming.md §6 Guideline 16 and
// MI355X_MICROARCH.md § visibility allow without an agent-scope acquire; gfx950 has 8 XCDs with
// private L2s and per-CU L1s that other CUs' stores never refresh): every handed-off double (update
// matrices and u-vectors of a child in the same flow, x of a backward front whose children wait for
// it) is written as a tagged pair by relaxed agent-scope atomic stores (global_store ... sc1,
// write-through to the memory-side coherence point) and read by relaxed agent-scope atomic loads
// (global_load ... sc1, which bypass the CU's L1 and the XCD's L2 copy); a consumer accepts a value
// only when both of its halves carry this step's epoch, so it can never take a stale or torn value,
// and no drain, flag or fence is needed on either side. Data from earlier launches (kernel boundary)
// is read with plain loads. Checked in the disassembly: the granule loads and stores are
// global_load/store_dwordx2 sc1, no flat_ access, no scalar load of handed-off data.
// Called by every wave once it has taken its last ticket.
__device__ __forceinline__ void leave_flow(const Flow& f) {
    if (threadIdx.x == 0 && atomicAdd(f.exits, 1) == (int)gridDim.x - 1) {
        __hip_atomic_store(f.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(f.exits, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A child's extend-add inputs: its r, row map entry (lane < rc) and where its update matrix and
// u-vector live, and the parent-front positions of the first 256 entries of its packed update
// matrix (4 per lane) — static structure, loaded before the child has finished — then its values:
// the u-vector entry and those 256 entries.
struct ChildPre {
    int rc, smap_v;
    double uval;
    double v[4];
    int pos[4];
    const double* Uc;
    const double* uc;
    const int16_t* ec;
    const unsigned long long* G;    // tagged update matrix + u-vector (a child in the same flow), or null
};

// (Every structure and value array is padded by kMfPad elements, so the clamped reads below stay in
// bounds even for an empty child range; see kMfPad.)
__device__ __forceinline__ void child_meta(const MfArgs& a, int c, int lane, ChildPre& p) {
    const int rc = a.r[c];   // rc < m <= MAXM
    const int roff = a.rmap_off[c];
    p.rc = rc;
    p.Uc = a.U + a.U_off[c];
    p.uc = a.u + a.u_off[c];
    p.ec = a.emap + a.emap_off[c];
    const int64_t go = a.ug_off[c];
    p.G = go >= 0 ? a.Ug + go : nullptr;
    const int sv = a.rmap[roff + min(lane, max(rc - 1, 0))];
    p.smap_v = lane < rc ? sv : 0;
    const int ne = rc * (rc + 1) / 2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = 64 * u + lane;
        const int pv = p.ec[min(e, max(ne - 1, 0))];
        p.pos[u] = e < ne ? pv : 0;
    }
}

template <bool COH>
__device__ __forceinline__ void child_vals(int lane, ChildPre& p) {
    const int rc = p.rc;
    const double uv = ldc<COH>(p.uc + min(lane, max(rc - 1, 0)));
    p.uval = lane < rc ? uv : 0.0;
    const int ne = rc * (rc + 1) / 2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = 64 * u + lane;
        const double v = ldc<COH>(p.Uc + min(e, max(ne - 1, 0)));
        p.v[u] = e < ne ? v : 0.0;
    }
}

// A child of the same flow (p.G): poll its tagged update matrix and u-vector until every granule
// carries this step's epoch (the data is the flag: no completion flag, no second load round trip),
// keeping the u-vector entry and the first 256 entries. Bounded (kWaitTicks): a stall marks info
// and returns (the launch then drains, the step fails).
// Waiting is done by ONE lane probing ONE granule (the child's last u-vector entry, its last store),
// the full sweep follows once it matches: a wave sweeping all its granules on every poll multiplied
// the polling traffic by ~600 loads per poll.
__device__ __forceinline__ bool probe_granule(const unsigned long long* g, uint32_t epoch, uint64_t t0, int32_t* info) {
    if (threadIdx.x % 64 == 0) {
        for (uint32_t it = 0;; ++it) {
            if ((uint32_t)(__hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32) == epoch) break;
            if ((it & 15) == 15) {
                const bool stalled = (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kMfStall) != 0;
                if (stalled || __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    __builtin_amdgcn_wave_barrier();
    return true;
}

__device__ __forceinline__ void child_sweep(ChildPre& p, uint32_t epoch, int lane, int32_t* info) {
    const int rc = p.rc, ne = rc * (rc + 1) / 2;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    probe_granule(p.G + 2 * (int64_t)(ne + max(rc - 1, 0)) + 1, epoch, t0, info);
    for (uint32_t it = 0;; ++it) {
        bool ok = true;
        const double uv = untag_pair(p.G + 2 * (int64_t)(ne + min(lane, max(rc - 1, 0))), epoch, ok);
        p.uval = lane < rc ? uv : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = 64 * u + lane;
            const double v = untag_pair(p.G + 2 * (int64_t)min(e, max(ne - 1, 0)), epoch, ok);
            p.v[u] = e < ne ? v : 0.0;
        }
        for (int e0 = 256; e0 < ne; e0 += 256)   // later entries: checked here, read in extend_child
#pragma unroll
            for (int u = 0; u < 4; ++u) (void)untag_pair(p.G + 2 * (int64_t)min(e0 + 64 * u + lane, ne - 1), epoch, ok);
        if (__builtin_amdgcn_ballot_w64(!ok) == 0) return;
        if ((it & 15) == 15) {
            const bool stalled = (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kMfStall) != 0;
            if (stalled || __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) {
                if (lane == 0) atomicOr(info, kMfStall);
                return;
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Extend-add of one child: every entry of its packed update matrix added at its precomputed position
// in the parent's packed front (positions of one child are distinct), then its u-vector.
template <bool COH>
__device__ __forceinline__ void extend_child(const MfArgs& a, const ChildPre& p, double* F, double* wv, int m, int lane,
                                             uint32_t epoch = 0) {
    const int rc = p.rc;
    const int ne = rc * (rc + 1) / 2;
    for (int e0 = 0; e0 < ne; e0 += 256) {
        double v[4];
        int pos[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = min(e0 + 64 * u + lane, ne - 1);   // clamped (see assemble_wave)
            bool ok = true;   // (tagged: child_sweep has seen every tag current)
            v[u] = e0 == 0 ? p.v[u] : p.G ? untag_pair(p.G + 2 * (int64_t)e, epoch, ok) : ldc<COH>(p.Uc + e);
            pos[u] = e0 == 0 ? p.pos[u] : p.ec[e];
        }
        // the four front entries read at once (positions of one child are distinct; a lane past the
        // child's entries reads a valid position and writes nothing), then added and written back: a
        // read-modify-write per entry under its own branch waited for each read separately
        double f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u] = F[pos[u]];
        asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + 64 * u + lane < ne) F[pos[u]] = f[u] + v[u];
    }
    if (lane < rc) wv[p.smap_v] += p.uval;
    wave_sync();
}

}  // namespace

}  // namespace dev
}  // namespace bos
