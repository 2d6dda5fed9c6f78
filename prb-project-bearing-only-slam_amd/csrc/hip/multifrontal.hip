// GPU supernodal multifrontal Cholesky for the GN normal system (replaces the reference's
// Eigen SimplicialLDLT, slam/solver.cpp:75-85; pattern analysed once like analyzePattern at
// :77-80 — here the symbolic analysis is host/plan.cpp build_multifrontal).
//
// P^T H_nf P = L L^T, H read from the J+H kernel's block array through the assembly map; fp64 and
// deterministic (no atomics on values). A front is
//   1. zeroed, then receives its entries of H (precomputed map) and the extend-add of its
//      children's update matrices (children sequentially, entries in parallel: deterministic),
//   2. partially factored (right-looking Cholesky of its k own columns),
//   3. written out: the m x k panel of L and the packed r x r update matrix for its parent.
// DESIGN.md §4 "Solver" and the route table in §5 are the authority on what runs where and why; this
// file is the host side and one translation unit over the device code in the headers it includes:
//   wave_util.hpp    readlane_d, wave_sync, stage_lds (shared with pair_cov.hip and node_cov.hip)
//   mf_device.hpp    MfArgs, packed indexing, the L panel cache policy, coherent and tagged accesses,
//                    assemble_wave, rsqrt_nr, the diagnostic stamps, kMfPad
//   mf_level.hpp     level fallback: mf_factor_level, mf_forward_level, mf_backward_level
//   mf_fold.hpp      wave fold of the folded landmark children: fold_children, fold_store
//   mf_blk.hpp       blocked fronts (65-128 rows): fold_children_wg, factor_front_blk, mf_factor_blk
//   mf_flow.hpp      Flow (ticket queue, bounded waits) and the children's hand-off: child_meta,
//                    child_vals, child_sweep, extend_child
//   mf_wave.hpp      wave fronts: factor_front_reg / mf_factor_reg (register pivot loop),
//                    factor_front_pan / mf_factor_pan (panel), mf_factor_mixb (mixed launch),
//                    mf_factor_flow
//   mf_backward.hpp  backward_front, mf_backward_wave, mf_backward_fold, mf_backward_flow
// Here: front_class / launch_class, Prog and build_prog (a program's launch lists), MfDevice and
// mf_create, and the launch sequences.
//
// mf_factor (fused with the forward substitution), levels below the factor flow, leaves first. A level
// with blocked fronts that fits the GPU in one round is ONE mixed launch (mf_factor_mixb). Any other
// level launches its classes side by side: class 64 (and a handful of class-16 fronts) on a side
// stream, the blocked fronts on a second side stream, classes 16 and 48 (which takes the 17-32 row
// fronts too) on the main stream, which then joins both; fronts above kMfBlkMaxM rows (fallback plans)
// take the level fallback last. The rest of the tree, its narrow top, is one dataflow launch
// (mf_factor_flow). mf_solve runs top-down: one dataflow launch (mf_backward_flow) over the top, then
// per level the wave fronts (mf_backward_wave) and the workgroup fronts (mf_backward_level), and the
// folded landmarks last (mf_backward_fold). Every launch site notes its route (bos_host.h BOS_ROUTE_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/bos_host.h"
#include "../host/plan.hpp"
#include "device_mem.hpp"
#include "mf_backward.hpp"
#include "mf_blk.hpp"
#include "mf_device.hpp"
#include "mf_flow.hpp"
#include "mf_level.hpp"
#include "mf_wave.hpp"
#include "multifrontal.hpp"
#include "selinv.hpp"

namespace bos {
namespace dev {

// front size classes: m <= 16, 32, 48, 64 (one wavefront, registers / LDS), m <= kBlkMaxM (workgroup,
// blocked, folds landmarks: mf_factor_blk) and larger (workgroup, global scratch: mf_factor_level)
constexpr int kClasses = 6;
inline int front_class(int m) { return m <= kMfWaveMaxM ? (m - 1) / 16 : m <= kBlkMaxM ? 4 : 5; }
// The launch a front goes to: fronts with 16 < m <= 32 run in the class-48 launch of their level (one
// launch packs the level's waves better than two in a row on one stream: solve 589 -> 564 us on
// config 3; moving the m <= 16 fronts too measured 570)
inline int launch_class(int m) {
    const int c = front_class(m);
    return c == 1 ? 2 : c;
}

// The fronts one launch sequence processes: every front on one GPU; a rank's own subtrees or the
// replicated top when sharded (plan.hpp Shard). Levels below flow_lev0 run per level (binned by
// front class), the rest of the factorization as one dataflow launch; the backward solve as one
// dataflow launch over levels >= solve_lev0 (top-down), then per level, then the folded landmarks.
struct Prog {
    int id = 0;                     // flow id (1: own / everything, 2: top)
    std::vector<int32_t> ptr;       // (level l, class c) = list[ptr[l * kClasses + c], ...)
    std::vector<int> lds_factor, lds_fwd, lds_bwd;   // per (level, class): dynamic LDS bytes
    std::vector<int> lds_blk;       // per level: mf_factor_blk's LDS for its class-4 fronts
    int32_t* list = nullptr;
    int flow_lev0 = 0, n_flow_factor = 0;
    bool first_waited = false;      // the factor flow's first front has its parent in the same flow
    int32_t* order_factor = nullptr;
    bool flow_solve = false;
    int solve_lev0 = 0, n_flow_solve = 0, lds_bwd_flow = 0;
    int32_t* order_bwd = nullptr;
    int32_t* fold_list = nullptr;   // folded landmarks whose parent is in this program
    int n_fold = 0;
    // per-level backward launches of the wave fronts (classes 0-3, one launch per level, the LDS of
    // the level's largest panel): level l's fronts are blist[bptr[l] .. bptr[l + 1]), blds[l] bytes each
    std::vector<int32_t> bptr;
    std::vector<int> blds;
    int32_t* blist = nullptr;
    // host copies of list / order_factor / order_bwd / fold_list / blist: what the launch sites note
    // into the route report (MfDevice::note)
    std::vector<int32_t> h_list, h_order_factor, h_order_bwd, h_fold_list, h_blist;
    const int32_t* hl(int lev, int c) const { return h_list.data() + ptr[lev * kClasses + c]; }
    int count(int lev, int c0, int c1) const { return ptr[lev * kClasses + c1] - ptr[lev * kClasses + c0]; }
    int count(int lev, int c) const { return count(lev, c, c + 1); }
    int lds_max(const std::vector<int>& v, int lev, int c0, int c1) const {
        int b = 0;
        for (int c = c0; c < c1; ++c) b = std::max(b, v[lev * kClasses + c]);
        return b;
    }
};

// Dataflow launch geometry (config 3, measured with tools/solver_stamps.py and variant builds): a
// wave waiting on a dependency polls its flag, and waiting waves slow the ones working, so the flows
// run few waves: 6 per CU for the factorization (solve 593 us at 6 against 599 at 8, 602 at 4, 682
// at 12) and 4 per CU for the backward substitution (582 us at 4, 617 at 6, 636 at 8, 706 at 16).
// The flows take only the narrow top of the tree; wide levels (independent fronts, throughput
// bound) run as per-level launches: the backward substitution of levels with >= kSolveWideLevel
// fronts before the flow reaches them (config 3: levels 0-5, solve 659 -> 582 us), the
// factorization of levels with >= kFactorWideLevel fronts before its flow starts (config 3: levels
// 0-2, 564 -> 556 us; also level 3: 567).
#ifndef BOS_MF_FLOW_WAVES_F   // (A/B builds may override the flow geometry)
#define BOS_MF_FLOW_WAVES_F 6
#endif
constexpr int kFlowWavesFactor = BOS_MF_FLOW_WAVES_F;
// The per-level backward launch of a level's wave fronts gives every wave the LDS of the level's
// largest panel (m k doubles): class-64 fronts (up to ~16 KB) then hold a level-0 launch to 8-10
// waves per CU; splitting the big panels into a launch of their own measured no faster.
#ifndef BOS_MF_FLOW_WAVES_B
#define BOS_MF_FLOW_WAVES_B 4
#endif
constexpr int kFlowWavesBackward = BOS_MF_FLOW_WAVES_B;
#ifndef BOS_MF_SOLVE_WIDE   // (A/B builds may override the two thresholds)
#define BOS_MF_SOLVE_WIDE 256
#endif
#ifndef BOS_MF_FACTOR_WIDE
#define BOS_MF_FACTOR_WIDE 2048
#endif
constexpr int kSolveWideLevel = BOS_MF_SOLVE_WIDE;
constexpr int kFactorWideLevel = BOS_MF_FACTOR_WIDE;
struct MfDevice {
    DeviceMem mem;                // every device array below, both programs' lists included
    int nlevels = 0, nsuper = 0, ncu = 256;
    bool mixb = false;            // mf_factor_mixb too (a level's blocked and wave fronts in one launch)
    bool blk = false;             // mf_factor_blk may take its (up to 132 KB of) dynamic LDS
    // a level's largest fronts (class 64: few, one latency-bound round) run on a side stream beside
    // the level's other classes
    hipStream_t side = nullptr, side2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;
    static constexpr int tiny16 = 256;   // class-16 launches of at most this many fronts go to the side stream too
    Prog prog[2];                 // [0]: own (or every front), [1]: the replicated top (sharded only)
    int8_t *fid_f = nullptr, *fid_b = nullptr;   // flow membership: factor, backward
    int32_t* parent = nullptr;
    int* tickets = nullptr;       // [2 * kMfTickets]: work-queue tickets, then the launches' exit counters
    uint32_t* epoch = nullptr;    // device word, 1 at creation (granule tags start at 0), bumped per GN step
    unsigned long long* stamps = nullptr;   // diagnostics: [2][nsuper][8] flow stamps (factor, backward), or null
    int32_t *fold_cnt = nullptr, *fold_cptr = nullptr, *fold_chunk = nullptr, *fold_rec = nullptr;
    int16_t* emap = nullptr;
    int64_t* emap_off = nullptr;
    int32_t *col0 = nullptr, *k = nullptr, *r = nullptr, *child_ptr = nullptr, *child = nullptr,
            *rmap = nullptr, *amap_ptr = nullptr, *amap_src = nullptr, *amap_dst = nullptr, *findex = nullptr,
            *info = nullptr;
    int64_t *L_off = nullptr, *U_off = nullptr, *u_off = nullptr, *scratch_off = nullptr, *rmap_off = nullptr,
            *findex_off = nullptr;
    double *L = nullptr, *U = nullptr, *u = nullptr, *scratch = nullptr;
    const float* A32 = nullptr;   // mf_set_fold_source
    int64_t pl_lo = 0;
    // tagged hand-offs (MfArgs): update-matrix granules of flow fronts whose parent is in the same
    // flow, their offsets, x granules per dof and the fronts whose x a backward flow reads
    unsigned long long *Ug = nullptr, *xg = nullptr;
    int64_t* ug_off = nullptr;
    int8_t* xtag = nullptr;
    SelInv* selinv = nullptr;     // selected inverse (hip/selinv.hip): built when marginals are first asked for
    // Route report (bos_debug_solver_routes): every launch site of mf_factor_t / mf_solve notes its
    // route (bos_host.h BOS_ROUTE_*) for the fronts of the list it launches, the first time a program's
    // sequence is enqueued; a front's folded children (the fold_cnt the kernels read) go with it.
    std::vector<int8_t> route_f, route_b;
    std::vector<int32_t> h_child_ptr, h_child, h_fold_cnt;
    bool noted_f[2] = {false, false}, noted_b[2] = {false, false};
    void note_f(int which, int route, const int32_t* fronts, int n) {
        if (noted_f[which]) return;
        for (int i = 0; i < n; ++i) {
            const int s = fronts[i];
            route_f[s] = (int8_t)route;
            if (!h_fold_cnt.empty())
                for (int ci = h_child_ptr[s]; ci < h_child_ptr[s] + h_fold_cnt[s]; ++ci)
                    route_f[h_child[ci]] = (int8_t)BOS_ROUTE_F_FOLDED;
        }
    }
    void note_b(int which, int route, const int32_t* fronts, int n) {
        if (noted_b[which]) return;
        for (int i = 0; i < n; ++i) route_b[fronts[i]] = (int8_t)route;
    }

    MfArgs args(const Prog& P, int lev, int c, const double* A, double* x) const {
        MfArgs g;
        g.level = P.list + (P.ptr.empty() ? 0 : P.ptr[lev * kClasses + c]);
        g.count = P.ptr.empty() ? 0 : P.count(lev, c);
        g.col0 = col0; g.k = k; g.r = r; g.L_off = L_off; g.U_off = U_off; g.u_off = u_off;
        g.scratch_off = scratch_off; g.child_ptr = child_ptr; g.child = child; g.rmap_off = rmap_off; g.rmap = rmap;
        g.amap_ptr = amap_ptr; g.amap_src = amap_src; g.amap_dst = amap_dst; g.findex_off = findex_off;
        g.findex = findex; g.A = A; g.A32 = A32; g.pl_lo = pl_lo; g.L = L; g.U = U; g.u = u; g.scratch = scratch; g.x = x; g.info = info;
        g.fold_cnt = fold_cnt; g.fold_cptr = fold_cptr; g.fold_chunk = fold_chunk; g.fold_rec = fold_rec;
        g.emap = emap; g.emap_off = emap_off;
        g.Ug = Ug; g.ug_off = ug_off; g.xg = xg; g.xtag = xtag; g.epoch = epoch;
        g.stamps_f = stamps;
        g.stamps_b = stamps ? stamps + 8 * (int64_t)nsuper : nullptr;
        return g;
    }
};

namespace {

int build_prog(DeviceMem& mem, const Multifrontal& F, const std::vector<int8_t>& sel, int id, Prog& P, std::vector<int8_t>& fid_f,
               std::vector<int8_t>& fid_b, std::string& err) {
    P.id = id;
    const int L = F.nlevels;
    P.lds_factor.assign(L * kClasses, 0); P.lds_fwd.assign(L * kClasses, 0); P.lds_bwd.assign(L * kClasses, 0);
    P.ptr.assign(L * kClasses + 1, 0);
    P.lds_blk.assign(L, 0);
    auto mine = [&](int s) { return sel[s] == id; };
    std::vector<int32_t> lst;
    for (int l = 0; l < L; ++l)
        for (int c = 0; c < kClasses; ++c) {
            const int lc = l * kClasses + c;
            for (int q = F.level_ptr[l]; q < F.level_ptr[l + 1]; ++q) {
                const int s = F.level[q], k = F.k[s], m = k + F.r[s];
                if (!mine(s) || launch_class(m) != c) continue;
                lst.push_back(s);
                if (c < 4) {
                    P.lds_fwd[lc] = std::max(P.lds_fwd[lc], (m + m * k) * 8);
                    P.lds_bwd[lc] = std::max(P.lds_bwd[lc], (2 * k + (m - k) + m * k) * 8);
                } else {
                    if (m <= kLdsCapM) P.lds_factor[lc] = std::max(P.lds_factor[lc], m * m * 8);
                    if (c == 4) P.lds_blk[l] = std::max(P.lds_blk[l], blk_lds_bytes(m));
                    P.lds_fwd[lc] = std::max(P.lds_fwd[lc], m * 8);
                    P.lds_bwd[lc] = std::max(P.lds_bwd[lc], (2 * k + (k <= 64 ? k * (k + 1) : 0)) * 8);
                }
            }
            // longest fronts first (estimated by flops plus folded rows): the launch's tail is
            // then made of short fronts
            auto cost = [&](int s2) {
                const double k = F.k[s2], r = F.r[s2];
                double cc = k * k * k / 3 + k * k * r + k * r * r;
                if (!F.fold_cnt.empty())
                    for (int ci = F.child_ptr[s2]; ci < F.child_ptr[s2] + F.fold_cnt[s2]; ++ci)
                        cc += 4.0 * F.r[F.child[ci]] * F.r[F.child[ci]];
                return cc;
            };
            std::stable_sort(lst.begin() + P.ptr[lc], lst.end(), [&](int x, int y) { return cost(x) > cost(y); });
            P.ptr[lc + 1] = (int32_t)lst.size();
        }
    auto mine_in_level = [&](int l) {
        int c = 0;
        for (int q = F.level_ptr[l]; q < F.level_ptr[l + 1]; ++q) c += mine(F.level[q]);
        return c;
    };
    std::vector<int32_t> blst;
    P.bptr.assign(L + 1, 0);
    P.blds.assign(L, 0);
    for (int l = 0; l < L; ++l) {
        // the level's wave fronts (classes 0-3, in list order: longest first)
        const int q0 = P.ptr[l * kClasses], q1 = P.ptr[l * kClasses + 4];
        for (int q = q0; q < q1; ++q) {
            const int s2 = lst[q], k = F.k[s2], m = k + F.r[s2];
            P.blds[l] = std::max(P.blds[l], (2 * k + (m - k) + m * k) * 8);
            blst.push_back(s2);
        }
        P.bptr[l + 1] = (int32_t)blst.size();
    }
    // dataflow ranges: the factor flow starts at the lowest level (>= 2) from which every front is
    // <= kFlowMaxM, and above the wide levels. Both decided on the whole tree, not on this program's
    // fronts: a front is then factored by the same kernel (per-level or flow) whatever the partition,
    // and the per-level class-48 kernel (mf_factor_pan: trailing update on MFMA) and the flow's
    // rounding differ, so a sharded step equals the one-GPU step bit for bit only this way.
    P.flow_lev0 = L;
    while (P.flow_lev0 > 2) {
        bool small = true;
        for (int q = F.level_ptr[P.flow_lev0 - 1]; q < F.level_ptr[P.flow_lev0] && small; ++q)
            small = F.k[F.level[q]] + F.r[F.level[q]] <= kFlowMaxM;
        if (!small) break;
        --P.flow_lev0;
    }
    {
        int wide = std::min(2, L);
        while (wide < L && F.level_ptr[wide + 1] - F.level_ptr[wide] >= kFactorWideLevel) ++wide;
        P.flow_lev0 = std::max(P.flow_lev0, wide);
    }
    std::vector<int32_t> ofac, ofwd;
    for (int q = F.level_ptr[std::min(P.flow_lev0, L)]; q < F.level_ptr[L]; ++q) {
        const int s = F.level[q];
        if (!mine(s)) continue;
        ofac.push_back(s);
        fid_f[s] = (int8_t)id;
    }
    P.n_flow_factor = (int)ofac.size();
    P.first_waited = !ofac.empty() && F.parent[ofac[0]] >= 0 && fid_f[F.parent[ofac[0]]] == id;
    P.solve_lev0 = std::min(2, L);
    while (P.solve_lev0 < L && mine_in_level(P.solve_lev0) >= kSolveWideLevel) ++P.solve_lev0;
    for (int q = F.level_ptr[P.solve_lev0]; q < F.level_ptr[L]; ++q) {
        const int s = F.level[q], k = F.k[s], m = k + F.r[s];
        if (!mine(s)) continue;
        ofwd.push_back(s);
        P.lds_bwd_flow = std::max(P.lds_bwd_flow, (2 * k + (m - k) + m * k) * 8);
    }
    std::vector<int32_t> obwd(ofwd.rbegin(), ofwd.rend());
    P.n_flow_solve = (int)ofwd.size();
    P.flow_solve = P.n_flow_solve > 0 && P.lds_bwd_flow <= 48 * 1024;
    if (!P.flow_solve) P.solve_lev0 = L;
    else
        for (int s : obwd) fid_b[s] = (int8_t)id;
    std::vector<int32_t> folds;
    for (int s : F.fold_list)
        if (mine(F.parent[s])) folds.push_back(s);
    P.n_fold = (int)folds.size();
    if (!(mem.upload(&P.list, lst, kMfPad) && mem.upload(&P.order_factor, ofac, kMfPad) && mem.upload(&P.order_bwd, obwd, kMfPad) &&
          mem.upload(&P.fold_list, folds, kMfPad) && mem.upload(&P.blist, blst, kMfPad))) {
        err = "device allocation or upload failed (multifrontal)";
        return -2;
    }
    P.h_list = lst; P.h_order_factor = ofac; P.h_order_bwd = obwd; P.h_fold_list = folds; P.h_blist = blst;
    return 0;
}

}  // namespace

int mf_create(const Multifrontal& F, const int8_t* owner, int rank, MfDevice** out, std::string& err) {
    MfDevice* d = new MfDevice();
    *out = d;
    d->nlevels = F.nlevels;
    d->nsuper = F.nsuper;
    d->route_f.assign(F.nsuper, (int8_t)BOS_ROUTE_NONE);
    d->route_b.assign(F.nsuper, (int8_t)BOS_ROUTE_NONE);
    d->h_child_ptr = F.child_ptr; d->h_child = F.child; d->h_fold_cnt = F.fold_cnt;
    std::vector<int64_t> scr(F.nsuper, -1);
    int64_t scratch_size = 0;
    for (int s = 0; s < F.nsuper; ++s) {
        const int m = F.k[s] + F.r[s];
        if (m > kLdsCapM) { scr[s] = scratch_size; scratch_size += (int64_t)m * m; }
    }
    {
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
            d->ncu = ncu;
        // a front of kBlkMaxM rows takes 129 KB of LDS (160 KB per CU on gfx950)
        const int blk_lds = blk_lds_bytes(kBlkMaxM);
        d->blk = hipFuncSetAttribute((const void*)mf_factor_blk<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     blk_lds) == hipSuccess &&
                 hipFuncSetAttribute((const void*)mf_factor_blk<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     blk_lds) == hipSuccess;
        d->mixb = d->blk &&
                  hipFuncSetAttribute((const void*)mf_factor_mixb<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      blk_lds) == hipSuccess &&
                  hipFuncSetAttribute((const void*)mf_factor_mixb<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      blk_lds) == hipSuccess;
        (void)hipGetLastError();
        if (!d->blk) {
            // the plan folds landmarks into fronts of up to kMfBlkMaxM rows, which only mf_factor_blk eliminates
            for (int s = 0; s < F.nsuper; ++s)
                if (F.k[s] + F.r[s] > kMfWaveMaxM && !F.fold_cnt.empty() && F.fold_cnt[s] > 0) {
                    err = "multifrontal: the blocked front kernel cannot get its LDS (needed by this plan's folds)";
                    return -2;
                }
        }
    }
    // program of every supernode: 1 = own (everything on one GPU), 2 = top, 0 = another rank's
    std::vector<int8_t> sel(F.nsuper, 1), fid_f(F.nsuper, 0), fid_b(F.nsuper, 0);
    if (owner)
        for (int s = 0; s < F.nsuper; ++s) sel[s] = owner[s] == rank ? 1 : owner[s] == -1 ? 2 : 0;
    int rc;
    if ((rc = build_prog(d->mem, F, sel, 1, d->prog[0], fid_f, fid_b, err)) ||
        (owner && (rc = build_prog(d->mem, F, sel, 2, d->prog[1], fid_f, fid_b, err))))
        return rc;
    // every structure array with its kMfPad tail; every buffer zeroed
    DeviceMem& mem = d->mem;
    auto up = [&](auto** p, const auto& v) { return mem.upload(p, v, kMfPad); };
    auto bad = [&] { err = "device allocation or upload failed (multifrontal)"; return -2; };
    if (!(up(&d->fid_f, fid_f) && up(&d->fid_b, fid_b) && up(&d->parent, F.parent))) return bad();
    {   // tagged hand-offs: a flow front whose parent is in the same flow publishes its update matrix
        // and u-vector as granule pairs; every ancestor of a backward-flow front publishes its x so
        std::vector<int64_t> ugo(F.nsuper, -1);
        int64_t ug_size = 0, ndof = 0;
        for (int c = 0; c < F.nsuper; ++c) {
            ndof = std::max<int64_t>(ndof, (int64_t)F.col0[c] + F.k[c]);
            const int p = F.parent[c];
            if (p < 0 || fid_f[c] == 0 || fid_f[p] != fid_f[c]) continue;
            const int64_t rc2 = F.r[c];
            ugo[c] = ug_size;
            ug_size += 2 * (rc2 * (rc2 + 1) / 2 + rc2);
        }
        std::vector<int8_t> xt(F.nsuper, 0);
        for (int c = 0; c < F.nsuper; ++c)
            if (fid_b[c] != 0)
                for (int q = c; q >= 0 && !xt[q]; q = F.parent[q]) xt[q] = 1;
        if (!(up(&d->ug_off, ugo) && up(&d->xtag, xt) && mem.alloc(&d->Ug, std::max<int64_t>(ug_size, 1), true, 2 * kMfPad) &&
              mem.alloc(&d->xg, std::max<int64_t>(2 * ndof, 1), true, 2 * kMfPad)))
            return bad();
    }
    if (!(mem.alloc(&d->tickets, 2 * kMfTickets, true) && mem.upload(&d->epoch, std::vector<uint32_t>{1}))) return bad();
    {   // extend-add positions of every child whose parent is a wave or blocked front (m <= kBlkMaxM)
        std::vector<int64_t> eoff(F.nsuper, 0);
        std::vector<int16_t> em;
        for (int c = 0; c < F.nsuper; ++c) {
            const int p = F.parent[c];
            if (p < 0) continue;
            const int mp = F.k[p] + F.r[p], rc = F.r[c];
            if (mp > kBlkMaxM || rc == 0) continue;
            bool folded = false;
            for (int ci = F.child_ptr[p]; ci < F.child_ptr[p] + (F.fold_cnt.empty() ? 0 : F.fold_cnt[p]); ++ci)
                folded = folded || F.child[ci] == c;
            if (folded) continue;
            eoff[c] = (int64_t)em.size();
            const int32_t* rm = F.rmap.data() + F.rmap_off[c];
            for (int j = 0; j < rc; ++j)
                for (int i = j; i < rc; ++i) {
                    const int I = rm[i], J = rm[j];
                    if (I < J || I >= mp) { err = "multifrontal: child row map not increasing"; return -1; }
                    // wave fronts: packed lower column-major; blocked fronts: full m x m column-major
                    em.push_back((int16_t)(mp <= kMfWaveMaxM ? J * mp - J * (J - 1) / 2 + (I - J) : I + J * mp));
                }
        }
        if (!(up(&d->emap, em) && up(&d->emap_off, eoff))) return bad();
    }
    if (!(up(&d->col0, F.col0) && up(&d->k, F.k) && up(&d->r, F.r) && up(&d->child_ptr, F.child_ptr) && up(&d->child, F.child) &&
          up(&d->rmap, F.rmap) && up(&d->amap_ptr, F.amap_ptr) && up(&d->amap_src, F.amap_src) && up(&d->amap_dst, F.amap_dst) &&
          up(&d->findex, F.findex) && up(&d->L_off, F.L_off) && up(&d->U_off, F.U_off) && up(&d->u_off, F.u_off) &&
          up(&d->scratch_off, scr) && up(&d->rmap_off, F.rmap_off) && up(&d->findex_off, F.findex_off) &&
          up(&d->fold_cnt, F.fold_cnt) && up(&d->fold_cptr, F.fold_cptr) && up(&d->fold_chunk, F.fold_chunk) &&
          up(&d->fold_rec, F.fold_rec)))
        return bad();
    if (hipStreamCreateWithFlags(&d->side, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&d->side2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_join2, hipEventDisableTiming) != hipSuccess) {
        err = "side stream creation failed (multifrontal)";
        return -2;
    }
    auto alloc = [&](double** p, int64_t n) {   // + kMfPad: clamped reads
        return mem.alloc(p, std::max<int64_t>(n, 1), true, kMfPad);
    };
    if (!(alloc(&d->L, F.L_size) && alloc(&d->U, F.U_size) && alloc(&d->u, F.u_size) && alloc(&d->scratch, scratch_size) &&
          mem.alloc(&d->info, 1, true)))
        return bad();
    return 0;
}

void mf_destroy(MfDevice* d) {
    if (!d) return;
    selinv_destroy(d->selinv);
    if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
    if (d->ev_join) (void)hipEventDestroy(d->ev_join);
    if (d->ev_join2) (void)hipEventDestroy(d->ev_join2);
    if (d->side) (void)hipStreamDestroy(d->side);
    if (d->side2) (void)hipStreamDestroy(d->side2);
    delete d;
}

// info is zero on entry: zeroed at creation and, after every iteration, by the end-of-step
// reduce_stats launch (mf_info_ptr). The work-queue tickets reset themselves (leave_flow). Every
// launch argument is fixed (the flows read the step's epoch from the device), so the sequence can be
// captured once into a hipGraph and replayed.
template <bool F32>
hipError_t mf_factor_t(MfDevice* d, int which, const double* A, double* x, hipStream_t s) {
    hipError_t e;
    const Prog& P = d->prog[which];
    if (P.ptr.empty()) return hipSuccess;
    // Each launch of a level is written once here; an empty list launches nothing.
    // wave class c of level l (0: register pivot loop; 2, 3: panel kernel) on stream st
    auto wave_class = [&](int l, int c, hipStream_t st, int route) {
        const int n = P.count(l, c);
        if (!n) return;
        const MfArgs g = d->args(P, l, c, A, x);
        if (c == 0) hipLaunchKernelGGL((mf_factor_reg<16, F32>), dim3(n), dim3(64), 0, st, g);
        else if (c == 2) hipLaunchKernelGGL((mf_factor_pan<48, kPanelKP, F32>), dim3(n), dim3(64), 0, st, g);
        else hipLaunchKernelGGL((mf_factor_pan<64, kPanelKP, F32>), dim3(n), dim3(64), 0, st, g);
        d->note_f(which, route, P.hl(l, c), n);
    };
    // the blocked fronts (class 4) of level l on stream st
    auto blocked = [&](int l, hipStream_t st, int route) {
        const int n = P.count(l, 4);
        hipLaunchKernelGGL((mf_factor_blk<F32>), dim3(n), dim3(kMfBlock), P.lds_blk[l], st, d->args(P, l, 4, A, x));
        d->note_f(which, route, P.hl(l, 4), n);
    };
    // class c (4 or 5) of level l on the unblocked workgroup kernel in global scratch, and its forward step
    auto level_pair = [&](int l, int c) {
        const int n = P.count(l, c);
        if (!n) return;
        const MfArgs g = d->args(P, l, c, A, x);
        hipLaunchKernelGGL(mf_factor_level, dim3(n), dim3(kMfBlock), P.lds_factor[l * kClasses + c], s, g);
        hipLaunchKernelGGL(mf_forward_level, dim3(n), dim3(kMfBlock), P.lds_fwd[l * kClasses + c], s, g);
        d->note_f(which, BOS_ROUTE_F_LEVEL, P.hl(l, c), n);
    };
    for (int l = 0; l < std::min(P.flow_lev0, d->nlevels); ++l) {
        // a level with blocked fronts and few fronts in all (config 2): one launch for all of them
#ifdef BOS_DIAG_PAIR
        const int n4 = P.count(l, 4), nwf = P.count(l, 0, 4) - P.count(l, 2) + (P.count(l, 2) + 1) / 2;
#else
        const int n4 = P.count(l, 4), nwf = P.count(l, 0, 4);
#endif
        if (d->mixb && n4 > 0 && n4 + nwf <= d->ncu) {
            const int4 nw = make_int4(P.count(l, 0), P.count(l, 1), P.count(l, 2), P.count(l, 3));
            const int4 ow = make_int4(0, P.count(l, 0), P.count(l, 0, 2), P.count(l, 0, 3));
            hipLaunchKernelGGL((mf_factor_mixb<F32>), dim3(n4 + nwf), dim3(kMfBlock), std::max(P.lds_blk[l], kMixbWaveLds),
                               s, d->args(P, l, 0, A, x), d->args(P, l, 4, A, x).level, n4, nw, ow);
            d->note_f(which, BOS_ROUTE_F_MIXB_BLK, P.hl(l, 4), n4);
            d->note_f(which, BOS_ROUTE_F_MIXB_WAVE, P.hl(l, 0), P.count(l, 0, 4));
            level_pair(l, 5);   // fronts above kBlkMaxM rows (fallback plans)
            if ((e = hipGetLastError()) != hipSuccess) return e;
            continue;
        }
        const bool fork = d->side && P.count(l, 3) > 0;
        // the level's blocked fronts (config 2's separators: a few workgroups, each one latency-bound
        // front) on a second side stream, beside the wave fronts instead of after them
        const bool fork2 = d->side2 && d->blk && P.count(l, 4) > 0;
        // a handful of class-16 fronts (one latency-bound round, negligible load) follow them there
        const bool tiny16 = fork && P.count(l, 0) <= d->tiny16;
        if (fork || fork2) {
            if ((e = hipEventRecord(d->ev_fork, s)) != hipSuccess) return e;
        }
        if (fork2) {
            if ((e = hipStreamWaitEvent(d->side2, d->ev_fork, 0)) != hipSuccess) return e;
            blocked(l, d->side2, BOS_ROUTE_F_BLK_SIDE2);
            if ((e = hipEventRecord(d->ev_join2, d->side2)) != hipSuccess) return e;
        }
        if (fork) {
            if ((e = hipStreamWaitEvent(d->side, d->ev_fork, 0)) != hipSuccess) return e;
            wave_class(l, 3, d->side, BOS_ROUTE_F_PAN64_SIDE);
            if (tiny16) wave_class(l, 0, d->side, BOS_ROUTE_F_REG16_SIDE);
            if ((e = hipEventRecord(d->ev_join, d->side)) != hipSuccess) return e;
        }
        if (!tiny16) wave_class(l, 0, s, BOS_ROUTE_F_REG16);
        // (class 1 has no list of its own: launch_class() sends its fronts to the class-48 launch)
        wave_class(l, 2, s, BOS_ROUTE_F_PAN48);
        if (!fork) wave_class(l, 3, s, BOS_ROUTE_F_PAN64);
        if (fork && (e = hipStreamWaitEvent(s, d->ev_join, 0)) != hipSuccess) return e;
        if (fork2 && (e = hipStreamWaitEvent(s, d->ev_join2, 0)) != hipSuccess) return e;
        // larger fronts: up to kBlkMaxM rows the blocked workgroup kernel (MFMA; folds; forward step fused),
        // above it (fallback plans) the unblocked workgroup kernel in global scratch and its forward step
        if (!fork2) {
            if (d->blk && P.count(l, 4)) blocked(l, s, BOS_ROUTE_F_BLK);
            else level_pair(l, 4);
        }
        level_pair(l, 5);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (P.n_flow_factor > 0) {
        const Flow f{P.order_factor, P.n_flow_factor, d->tickets, d->tickets + kMfTickets, d->epoch, 0u,
                     d->fid_f, P.id, d->stamps};
        const int grid = std::min(P.n_flow_factor, d->ncu * kFlowWavesFactor);
        hipLaunchKernelGGL((mf_factor_flow<F32>), dim3(grid), dim3(64), 0, s, d->args(P, 0, 0, A, x), f);
        d->note_f(which, BOS_ROUTE_F_FLOW, P.h_order_factor.data(), P.n_flow_factor);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    d->noted_f[which] = true;
    return hipSuccess;
}

hipError_t mf_factor(MfDevice* d, int which, const double* A, double* x, hipStream_t s) {
    return d->A32 ? mf_factor_t<true>(d, which, A, x, s) : mf_factor_t<false>(d, which, A, x, s);
}

void mf_set_fold_source(MfDevice* d, const float* A32, int64_t pl_lo) {
    d->A32 = A32;
    d->pl_lo = pl_lo;
}

hipError_t mf_solve(MfDevice* d, int which, double* x, hipStream_t s) {
    // backward substitution (the forward one ran inside mf_factor): one flow launch over the levels
    // >= solve_lev0 (top-down), then per-level launches below it
    hipError_t e;
    const Prog& P = d->prog[which];
    if (P.ptr.empty()) return hipSuccess;
    if (P.flow_solve) {
        const Flow fb{P.order_bwd, P.n_flow_solve, d->tickets + 1, d->tickets + kMfTickets + 1,
                      d->epoch, 0u, d->fid_b, P.id, d->stamps ? d->stamps + 8 * (int64_t)d->nsuper : nullptr};
        const int grid = std::min(P.n_flow_solve, d->ncu * kFlowWavesBackward);
        hipLaunchKernelGGL(mf_backward_flow, dim3(grid), dim3(64), P.lds_bwd_flow, s, d->args(P, 0, 0, nullptr, x), fb,
                           (const int32_t*)d->parent);
        d->note_b(which, BOS_ROUTE_B_FLOW, P.h_order_bwd.data(), P.n_flow_solve);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int l = std::min(P.solve_lev0, d->nlevels) - 1; l >= 0; --l) {
        int n;
        if (P.bptr[l + 1] > P.bptr[l]) {
            MfArgs g = d->args(P, l, 0, nullptr, x);
            g.level = P.blist + P.bptr[l];
            g.count = P.bptr[l + 1] - P.bptr[l];
            hipLaunchKernelGGL(mf_backward_wave, dim3(g.count), dim3(64), P.blds[l], s, g);
            d->note_b(which, BOS_ROUTE_B_WAVE, P.h_blist.data() + P.bptr[l], g.count);
        }
        if ((n = P.count(l, 4, kClasses))) {   // the workgroup fronts (classes 4 and 5, one list)
            MfArgs g = d->args(P, l, 4, nullptr, x);
            g.count = n;
            hipLaunchKernelGGL(mf_backward_level, dim3(n), dim3(kMfBlock), P.lds_max(P.lds_bwd, l, 4, kClasses), s, g);
            d->note_b(which, BOS_ROUTE_B_LEVEL, P.hl(l, 4), n);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (P.n_fold > 0) {   // folded landmarks last: their rows are poses, final by now
        MfArgs g = d->args(P, 0, 0, nullptr, x);
        g.level = P.fold_list;
        g.count = P.n_fold;
        hipLaunchKernelGGL(mf_backward_fold, dim3(((int64_t)P.n_fold * kFoldLanes + kMfBlock - 1) / kMfBlock), dim3(kMfBlock), 0, s, g);
        d->note_b(which, BOS_ROUTE_B_FOLD, P.h_fold_list.data(), P.n_fold);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    d->noted_b[which] = true;
    return hipSuccess;
}

int mf_debug_routes(const MfDevice* d, int8_t* factor, int8_t* backward) {
    for (int w = 0; w < 2; ++w)
        if (!d->prog[w].ptr.empty() && (!d->noted_f[w] || !d->noted_b[w])) return -1;
    std::copy(d->route_f.begin(), d->route_f.end(), factor);
    std::copy(d->route_b.begin(), d->route_b.end(), backward);
    return 0;
}

MfView mf_view(const MfDevice* d) { return MfView{d->k, d->r, d->parent, d->rmap, d->L_off, d->rmap_off, d->L}; }
SelInv** mf_selinv_slot(MfDevice* d) { return &d->selinv; }
int32_t* mf_info_ptr(const MfDevice* d) { return d->info; }
uint32_t* mf_epoch_ptr(const MfDevice* d) { return d->epoch; }
void mf_debug_set_stamps(MfDevice* d, unsigned long long* stamps) {
    d->stamps = stamps;
#ifdef BOS_MF_PIVOT_CYCLES
    unsigned long long* b = stamps ? stamps + 8 * (int64_t)d->nsuper : nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_pivot_bwd), &b, sizeof(b));
#endif
}
int32_t* mf_tickets_ptr(const MfDevice* d) { return d->tickets; }
double* mf_update_ptr(const MfDevice* d) { return d->U; }
double* mf_uvec_ptr(const MfDevice* d) { return d->u; }

hipError_t mf_debug_skip_next_front(MfDevice* d, hipStream_t s) {
    // only where a front of the same launch waits for the skipped one (otherwise nothing would notice
    // the skip and the step would use the front's previous outputs)
    if (d->prog[0].n_flow_factor == 0 || !d->prog[0].first_waited) return hipErrorInvalidValue;
    static const int one = 1;
    return hipMemcpyAsync(d->tickets, &one, sizeof(int), hipMemcpyHostToDevice, s);
}

}  // namespace dev
}  // namespace bos
