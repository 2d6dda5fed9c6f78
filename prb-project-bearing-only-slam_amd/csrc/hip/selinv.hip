// Selected inverse (Takahashi recursion) of the multifrontal Cholesky factor: the diagonal blocks of
// (P^T H_nf P)^-1 that belong to whole nodes, from the finished L panels of hip/multifrontal.hip.
//
// Supernode s with k own dofs J and r update rows R, panel L = [L11; L21], parent p:
//   G     = Sigma_RR, entry (i, j) at the parent's Sigma front position (rmap[i], rmap[j])
//   Li    = L11^-1 (lower triangle of L11 only)
//   Z     = L21 Li
//   S_RJ  = -G Z
//   S_JJ  = Li^T Li - Z^T S_RJ   (lower triangle, mirrored)
// A supernode that has children (folded landmarks count) stores its Sigma front [[S_JJ, .], [S_RJ, G]]
// (full m x m column-major) for them. One workgroup per front; one launch per tree level and front
// class, top-down, then one for the folded landmarks. A front reads only its parent's Sigma front,
// which an earlier launch finished: plain stream order, no flags, no waits, no atomics.
//
// Working set of a front: Li (k k), Z (r k), S_RJ (r k), G (r r) = m m doubles. It lives in LDS for
// fronts of up to kMfBlkMaxM rows (one wavefront for m <= kMfWaveMaxM, else 256 threads and up to
// 128 KiB, requested as mf_factor_blk does); larger fronts, or 65-128-row fronts when that LDS is not
// granted, keep Li, Z and S_RJ in a global workspace and read G from the parent's front in place.
//
// Edge covariances: the cross block of an edge's two nodes is a piece of S_RJ (or of S_JJ when both
// nodes share the supernode) of the front that owns the node eliminated first. The X = true
// instantiation of the kernel writes those pieces, through the plan's cross records, into the pair
// buffer, in all three front classes (S_RJ sits in LDS or in the workspace behind the same pointer);
// the X = false instantiation is the marginals' kernel, unchanged.
#include "selinv.hpp"

#include <algorithm>
#include <memory>
#include <vector>

#include "../../../include/bos_host.h"
#include "../host/plan.hpp"
#include "device_mem.hpp"
#include "edge_cov.hpp"
#include "multifrontal.hpp"

namespace bos {
namespace dev {

namespace {

struct SelArgs {
    const int32_t* list;      // the launch's supernodes
    const int32_t *k, *r, *parent, *rmap, *out_ptr, *out_rec;
    const int64_t *L_off, *rmap_off, *S_off, *ws_off;
    const double* L;
    double *S, *ws, *out;
    int64_t lm_base;          // the landmark blocks' offset in out (9 NP)
    const int32_t *cr_ptr, *cr_rec;   // cross records (plan.hpp CrossRecords), read by selinv_front<T, true> only
    double* pairs;                    // [9 n_pairs]
};

constexpr int kWaveThreads = 64, kBlkThreads = 256;
constexpr int kDefaultLds = 64 * 1024;
typedef double dbl4 __attribute__((ext_vector_type(4)));

template <int T, bool X> __global__ __launch_bounds__(T) void selinv_front(const SelArgs a) {
    extern __shared__ double sel_lds[];
    const int s = a.list[blockIdx.x], t = threadIdx.x;
    const int k = a.k[s], r = a.r[s], m = k + r;
    const double* Ls = a.L + a.L_off[s];
    const bool in_lds = a.ws_off[s] < 0;
    double* w = in_lds ? sel_lds : a.ws + a.ws_off[s];
    double *Li = w, *Z = Li + k * k, *SR = Z + r * k, *Gs = SR + r * k;
    const int32_t* rm = a.rmap + a.rmap_off[s];
    const double* Sp = nullptr;
    int mp = 0;
    if (r > 0) {
        const int p = a.parent[s];
        mp = a.k[p] + a.r[p];
        Sp = a.S + a.S_off[p];
    }
    auto G = [&](int i, int l) { return in_lds ? Gs[i + l * r] : Sp[rm[i] + (int64_t)rm[l] * mp]; };

    if (in_lds)
        for (int idx = t; idx < r * r; idx += T) Gs[idx] = Sp[rm[idx % r] + (int64_t)rm[idx / r] * mp];
    // The panel is read from global memory once, coalesced: L11's lower triangle into Li's place and
    // L21 into Z's; both are then overwritten in place.
    for (int idx = t; idx < k * k; idx += T)
        if (idx % k >= idx / k) Li[idx] = Ls[idx % k + (int64_t)(idx / k) * m];
    for (int idx = t; idx < r * k; idx += T) Z[idx] = Ls[(k + idx % r) + (int64_t)(idx / r) * m];
    __syncthreads();
    // Li = L11^-1 row by row, a column per thread: X[i][j] = ((i == j) - sum_{j <= l < i} L[i][l] X[l][j])
    // / L[i][i]. Rows above i already hold X; row i holds L until every thread has read it, so the new
    // row waits in the unused upper triangle (at its transposed place) for the barrier.
    for (int i = 0; i < k; ++i) {
        const double d = Li[i + i * k];
        for (int j = t; j < i; j += T) {
            double acc = 0.0;
            for (int l = j; l < i; ++l) acc -= Li[i + l * k] * Li[l + j * k];
            Li[j + i * k] = acc / d;
        }
        __syncthreads();
        for (int j = t; j <= i; j += T) Li[i + j * k] = j < i ? Li[j + i * k] : 1.0 / d;
        __syncthreads();
    }
    // Z = L21 Li, a row per thread, columns ascending: Z[i][j] = sum_{l >= j} L21[i][l] Li[l][j] needs
    // only the columns l >= j of row i of L21, so each entry is overwritten as soon as it is formed
    for (int i = t; i < r; i += T)
        for (int j = 0; j < k; ++j) {
            double acc = 0.0;
            for (int l = j; l < k; ++l) acc += Z[i + l * r] * Li[l + j * k];
            Z[i + j * r] = acc;
        }
    __syncthreads();
    bool tiled = false;
    if constexpr (T == kBlkThreads) tiled = in_lds;
    if (tiled) {
        // G Z in 16 x 16 tiles on the f64 MFMA (16 x 16 x 4), the tiles dealt to the four waves. Lane l
        // feeds A = G[16 bi + (l & 15)][4 st + (l >> 4)] and B = Z[4 st + (l >> 4)][16 bj + (l & 15)];
        // it receives rows 16 bi + (l >> 4) + 4 v (v = 0..3) of column 16 bj + (l & 15). Entries past
        // r or k are fed as zeros.
        const int lane = t & 63, c16 = lane & 15, q4 = lane >> 4, ntr = (r + 15) >> 4, ntc = (k + 15) >> 4;
        for (int tile = t >> 6; tile < ntr * ntc; tile += T / 64) {
            const int bi = tile % ntr, bj = tile / ntr, row = 16 * bi + c16, col = 16 * bj + c16;
            dbl4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int l0 = 0; l0 < r; l0 += 4) {
                const int l = l0 + q4;
                const double av = row < r && l < r ? Gs[row + l * r] : 0.0;
                const double bv = col < k && l < r ? Z[l + col * r] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 16 * bi + q4 + 4 * v;
                if (i < r && col < k) SR[i + col * r] = -acc[v];
            }
        }
    } else {
        for (int idx = t; idx < r * k; idx += T) {
            const int i = idx % r, j = idx / r;
            double acc = 0.0;
            for (int l = 0; l < r; ++l) acc += G(i, l) * Z[l + j * r];
            SR[idx] = -acc;
        }
    }
    __syncthreads();
    auto sjj = [&](int x, int y) {   // entry (x, y) of S_JJ, evaluated as its lower-triangle twin
        const int hi = max(x, y), lo = min(x, y);
        double acc = 0.0;
        for (int l = hi; l < k; ++l) acc += Li[l + hi * k] * Li[l + lo * k];
        for (int i = 0; i < r; ++i) acc -= Z[i + hi * r] * SR[i + lo * r];
        return acc;
    };
    if (a.S_off[s] >= 0) {   // the Sigma front, for the children
        double* Sf = a.S + a.S_off[s];
        for (int idx = t; idx < k * k; idx += T) {
            const int x = idx % k, y = idx / k;
            if (x < y) continue;
            const double v = sjj(x, y);
            Sf[x + (int64_t)y * m] = v;
            Sf[y + (int64_t)x * m] = v;
        }
        for (int idx = t; idx < r * k; idx += T) {
            const int i = idx % r, j = idx / r;
            const double v = SR[idx];
            Sf[(k + i) + (int64_t)j * m] = v;
            Sf[j + (int64_t)(k + i) * m] = v;
        }
        for (int idx = t; idx < r * r; idx += T) Sf[(k + idx % r) + (int64_t)(k + idx / r) * m] = G(idx % r, idx / r);
    }
    const int q0 = a.out_ptr[s], nq = a.out_ptr[s + 1] - q0;
    for (int e = t; e < nq * 9; e += T) {   // the whole nodes' diagonal blocks
        const int32_t* rec = a.out_rec + 3 * (int64_t)(q0 + e / 9);
        const int loc = rec[0], sz = rec[2], xy = e % 9;
        if (xy >= sz * sz) continue;
        const int x = xy / sz, y = xy % sz;
        a.out[(sz == 3 ? 0 : a.lm_base) + rec[1] + xy] = sjj(loc + x, loc + y);
    }
    if constexpr (X) {   // the edges' cross blocks: entry xy of the pair's block, canonical orientation
        const int c0 = a.cr_ptr[s], nc = a.cr_ptr[s + 1] - c0;
        for (int e = t; e < nc * 9; e += T) {
            const int32_t* rec = a.cr_rec + kCrossRec * (int64_t)(c0 + e / 9);
            const int pos = rec[0], loc = rec[1], rows = rec[2], cols = rec[3], xy = e % 9;
            if (xy >= rows * cols) continue;
            const int i = rec[5] ? xy % rows : xy / cols, j = rec[5] ? xy / rows : xy % cols;
            a.pairs[9 * (int64_t)rec[4] + xy] = pos >= k ? SR[(pos - k + i) + (loc + j) * r] : sjj(pos + i, loc + j);
        }
    }
}

struct Launch {
    int first, count, threads, lds;
};

}  // namespace

// the feature's state (mf_edge_cov_build): index arrays, pair buffer and per-edge outputs in one arena
struct EdgeCovDev {
    DeviceMem mem;           // the arena alone
    char* arena = nullptr;   // null until built
    int64_t n_pairs = 0;
    int Mb = 0, Mo = 0;
    int32_t *cr_ptr = nullptr, *cr_rec = nullptr, *edge_slot = nullptr, *edge_tr = nullptr;
    int32_t *b_pose = nullptr, *b_lm = nullptr, *o_src = nullptr, *o_dst = nullptr;
    double *pairs = nullptr, *bearing_cross = nullptr, *odom_cross = nullptr, *bearing_var = nullptr, *odom_cov = nullptr;
    CrossRecords h_cr;   // the host's copy of what was uploaded (mf_selinv_report)
};

struct SelInv {
    DeviceMem mem;   // every device array below (the edge arena: ec.mem)
    EdgeCovDev ec;
    std::vector<Launch> launches;
    // the report (mf_selinv_report): per supernode the class and the launch selinv_build's add gave it,
    // and the host's copies of the diagonal-block records and the Sigma fronts' offsets
    std::vector<int8_t> cls;
    std::vector<int32_t> launch_of, h_out_ptr, h_out_rec;
    std::vector<int64_t> h_S_off;
    int32_t *list = nullptr, *out_ptr = nullptr, *out_rec = nullptr;
    int64_t *S_off = nullptr, *ws_off = nullptr;
    double *S = nullptr, *ws = nullptr, *out = nullptr;
    int64_t sigma_bytes = 0, out_count = 0, lm_base = 0;
};

void selinv_destroy(SelInv* p) { delete p; }

namespace {

int selinv_build(const Plan& P, SelInv** out, std::string& err) {
    const Multifrontal& F = P.mf;
    std::vector<int32_t> out_ptr, out_rec;
    if (!selinv_records(P, out_ptr, out_rec)) { err = "marginals: a node's dofs are split between two supernodes"; return -1; }
    for (int s = 0; s < F.nsuper; ++s) {   // everything the kernels index with, checked once
        const int k = F.k[s], r = F.r[s], p = F.parent[s];
        if (k <= 0 || r < 0 || (r > 0 && p < 0)) { err = "marginals: malformed supernode"; return -1; }
        for (int i = 0; i < r; ++i) {
            const int32_t v = F.rmap[F.rmap_off[s] + i];
            if (v < 0 || v >= F.k[p] + F.r[p]) { err = "marginals: update row outside the parent's front"; return -1; }
        }
        for (int q = out_ptr[s]; q < out_ptr[s + 1]; ++q)
            if (out_rec[3 * q] < 0 || out_rec[3 * q] + out_rec[3 * q + 2] > k) { err = "marginals: node outside its supernode"; return -1; }
    }
    // 65-128-row fronts keep their m m doubles in LDS when the workgroup kernel may take them
    const int blk_lds = kMfBlkMaxM * kMfBlkMaxM * (int)sizeof(double);
    const bool big_lds = hipFuncSetAttribute((const void*)selinv_front<kBlkThreads, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             blk_lds) == hipSuccess &&
                         hipFuncSetAttribute((const void*)selinv_front<kBlkThreads, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             blk_lds) == hipSuccess;
    (void)hipGetLastError();
    const int lds_cap = big_lds ? blk_lds : kDefaultLds;

    std::unique_ptr<SelInv> si(new SelInv());   // dropped with its allocations on every failure below
    si->cls.assign(F.nsuper, (int8_t)-1);
    si->launch_of.assign(F.nsuper, -1);
    std::vector<int32_t> list;
    std::vector<int64_t> S_off(F.nsuper, -1), ws_off(F.nsuper, -1);
    int64_t S_size = 0, ws_size = 0;
    for (int s = 0; s < F.nsuper; ++s)
        if (F.child_ptr[s + 1] > F.child_ptr[s]) {
            const int64_t m = F.k[s] + F.r[s];
            S_off[s] = S_size;
            S_size += m * m;
        }
    for (int s = 0; s < F.nsuper; ++s)
        if (F.r[s] > 0 && S_off[F.parent[s]] < 0) {
            err = "marginals: a supernode is missing from its parent's child list";
            return -1;
        }
    auto add = [&](const std::vector<int32_t>& fr, int threads) {
        if (fr.empty()) return;
        Launch ln{(int)list.size(), (int)fr.size(), threads, 0};
        int64_t ws = 0;
        for (int s : fr) {
            const int64_t k = F.k[s], r = F.r[s], m = k + r, bytes = m * m * (int64_t)sizeof(double);
            if (bytes <= (threads == kWaveThreads ? kDefaultLds : lds_cap)) {
                ln.lds = std::max<int>(ln.lds, (int)bytes);
                si->cls[s] = threads == kWaveThreads ? BOS_SELINV_WAVE_LDS : BOS_SELINV_BLK_LDS_MFMA;
            } else {
                ws_off[s] = ws;   // launches follow each other on one stream: they share the workspace
                ws += k * k + 2 * r * k;
                si->cls[s] = BOS_SELINV_BLK_WORKSPACE;
            }
            si->launch_of[s] = (int32_t)si->launches.size();
            list.push_back(s);
        }
        ws_size = std::max(ws_size, ws);
        si->launches.push_back(ln);
    };
    std::vector<int32_t> wave, blk;
    for (int lv = F.nlevels - 1; lv >= 0; --lv) {
        wave.clear();
        blk.clear();
        for (int q = F.level_ptr[lv]; q < F.level_ptr[lv + 1]; ++q) {
            const int s = F.level[q];
            (F.k[s] + F.r[s] <= kMfWaveMaxM ? wave : blk).push_back(s);
        }
        add(wave, kWaveThreads);
        add(blk, kBlkThreads);
    }
    wave.clear();
    blk.clear();
    for (int s : F.fold_list) (F.k[s] + F.r[s] <= kMfWaveMaxM ? wave : blk).push_back(s);
    add(wave, kWaveThreads);
    add(blk, kBlkThreads);

    si->lm_base = 9 * (int64_t)P.NP;
    si->out_count = 9 * (int64_t)P.NP + 4 * (int64_t)P.NL;
    si->sigma_bytes = std::max<int64_t>(S_size, 1) * (int64_t)sizeof(double);
    DeviceMem& mem = si->mem;
    if (!(mem.upload(&si->list, list, 0, true) && mem.upload(&si->out_ptr, out_ptr, 0, true) &&
          mem.upload(&si->out_rec, out_rec, 0, true) && mem.upload(&si->S_off, S_off, 0, true) &&
          mem.upload(&si->ws_off, ws_off, 0, true) && mem.alloc(&si->S, std::max<int64_t>(S_size, 1), false) &&
          mem.alloc(&si->ws, std::max<int64_t>(ws_size, 1), false) && mem.alloc(&si->out, std::max<int64_t>(si->out_count, 1), false))) {
        err = "marginals: a device allocation failed after " + std::to_string(mem.bytes()) +
              " bytes (Sigma-front buffer: " + std::to_string(si->sigma_bytes) + " bytes)";
        return -2;
    }
    si->h_out_ptr.swap(out_ptr);
    si->h_out_rec.swap(out_rec);
    si->h_S_off.swap(S_off);
    *out = si.release();
    return 0;
}

}  // namespace

int mf_selected_inverse(MfDevice* d, const Plan& P, const double** out_dev, hipStream_t s, std::string& err, bool emit_cross) {
    SelInv** slot = mf_selinv_slot(d);
    if (!*slot) {
        const int rc = selinv_build(P, slot, err);
        if (rc) { *slot = nullptr; return rc; }
    }
    SelInv* si = *slot;
    if (emit_cross && !si->ec.arena) { err = "edge covariances: the cross records are not built"; return -1; }
    const MfView v = mf_view(d);
    SelArgs a;
    a.cr_ptr = emit_cross ? si->ec.cr_ptr : nullptr; a.cr_rec = emit_cross ? si->ec.cr_rec : nullptr;
    a.pairs = emit_cross ? si->ec.pairs : nullptr;
    a.k = v.k; a.r = v.r; a.parent = v.parent; a.rmap = v.rmap; a.L_off = v.L_off; a.rmap_off = v.rmap_off; a.L = v.L;
    a.out_ptr = si->out_ptr; a.out_rec = si->out_rec; a.S_off = si->S_off; a.ws_off = si->ws_off;
    a.S = si->S; a.ws = si->ws; a.out = si->out; a.lm_base = si->lm_base;
    hipError_t e = hipMemsetAsync(si->out, 0, std::max<int64_t>(si->out_count, 1) * sizeof(double), s);
    for (size_t i = 0; i < si->launches.size() && e == hipSuccess; ++i) {
        const Launch& ln = si->launches[i];
        a.list = si->list + ln.first;
        if (ln.threads == kWaveThreads) {
            if (emit_cross) selinv_front<kWaveThreads, true><<<ln.count, kWaveThreads, ln.lds, s>>>(a);
            else selinv_front<kWaveThreads, false><<<ln.count, kWaveThreads, ln.lds, s>>>(a);
        } else {
            if (emit_cross) selinv_front<kBlkThreads, true><<<ln.count, kBlkThreads, ln.lds, s>>>(a);
            else selinv_front<kBlkThreads, false><<<ln.count, kBlkThreads, ln.lds, s>>>(a);
        }
        e = hipGetLastError();
    }
    if (e != hipSuccess) { err = std::string("marginals: selected-inverse launch: ") + hipGetErrorString(e); return -2; }
    *out_dev = si->out;
    return 0;
}

bool mf_edge_cov_built(const MfDevice* d) {
    SelInv* const* slot = mf_selinv_slot(const_cast<MfDevice*>(d));
    return *slot && (*slot)->ec.arena;
}

int64_t mf_edge_cov_bytes(const MfDevice* d) {
    SelInv* const* slot = mf_selinv_slot(const_cast<MfDevice*>(d));
    return *slot ? (int64_t)(*slot)->ec.mem.bytes() : 0;
}

int mf_edge_cov_build(MfDevice* d, const Plan& P, const EdgeList& E, std::string& err) {
    SelInv** slot = mf_selinv_slot(d);
    if (!*slot) {
        const int rc = selinv_build(P, slot, err);
        if (rc) { *slot = nullptr; return rc; }
    }
    EdgeCovDev& ec = (*slot)->ec;
    if (ec.arena) return 0;
    const Multifrontal& F = P.mf;
    CrossRecords cr;
    if (!selinv_cross_records(P, E.Mb, E.Mo, E.b_pose, E.b_lm, E.o_src, E.o_dst, cr)) {
        err = "bos_edge_covariances: an edge's cross block is not inside one front";
        return -1;
    }
    // everything the kernels index with, checked once (the edges' endpoints: selinv_cross_records)
    const int64_t edges = (int64_t)E.Mb + E.Mo, nrec = cr.ptr[F.nsuper];
    bool good = nrec == cr.n_pairs && (int64_t)cr.rec.size() == kCrossRec * nrec && (int64_t)cr.edge_slot.size() == edges &&
                (int64_t)cr.edge_tr.size() == edges;
    for (int s = 0; s < F.nsuper && good; ++s)
        for (int q = cr.ptr[s]; q < cr.ptr[s + 1] && good; ++q) {
            const int32_t* rec = cr.rec.data() + (size_t)kCrossRec * q;
            const bool pose_pair = rec[2] == 3 && rec[3] == 3;
            good = rec[0] >= 0 && rec[0] + rec[2] <= F.k[s] + F.r[s] && rec[1] >= 0 && rec[1] + rec[3] <= F.k[s] &&
                   (pose_pair || rec[2] * rec[3] == 6) && rec[4] >= 0 && rec[4] < cr.n_pairs && (rec[5] == 0 || rec[5] == 1);
        }
    for (int64_t e = 0; e < edges && good; ++e) good = cr.edge_slot[e] >= -1 && cr.edge_slot[e] < cr.n_pairs;
    if (!good) { err = "bos_edge_covariances: malformed cross records"; return -1; }

    // one arena: [index arrays | pair buffer | per-edge outputs], every part aligned to 256 bytes (an
    // empty one keeps an element's room). Built aside: a failure leaves ec as it was.
    Arena ar(true);
    ar.add(&ec.cr_ptr, cr.ptr); ar.add(&ec.cr_rec, cr.rec); ar.add(&ec.edge_slot, cr.edge_slot); ar.add(&ec.edge_tr, cr.edge_tr);
    ar.add(&ec.b_pose, E.b_pose, (size_t)E.Mb); ar.add(&ec.b_lm, E.b_lm, (size_t)E.Mb);
    ar.add(&ec.o_src, E.o_src, (size_t)E.Mo); ar.add(&ec.o_dst, E.o_dst, (size_t)E.Mo);
    ar.reserve(&ec.pairs, 9 * (size_t)cr.n_pairs);
    ar.reserve(&ec.bearing_cross, 6 * (size_t)E.Mb); ar.reserve(&ec.odom_cross, 9 * (size_t)E.Mo);
    ar.reserve(&ec.bearing_var, (size_t)E.Mb); ar.reserve(&ec.odom_cov, 9 * (size_t)E.Mo);
    DeviceMem mem;
    if (!ar.commit(mem, &ec.arena)) {
        err = "bos_edge_covariances: device allocation or upload of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    ec.mem = std::move(mem);
    ec.n_pairs = cr.n_pairs;
    ec.Mb = E.Mb; ec.Mo = E.Mo;
    ec.h_cr = std::move(cr);
    return 0;
}

int mf_selinv_report(const MfDevice* d, const Plan& P, int32_t* fronts, int32_t* node_front, int32_t* edge_front) {
    SelInv* const* slot = mf_selinv_slot(const_cast<MfDevice*>(d));
    if (!*slot) return -1;
    const SelInv* si = *slot;
    const Multifrontal& F = P.mf;
    const bool cross = si->ec.arena != nullptr;
    const CrossRecords& cr = si->ec.h_cr;
    std::vector<char> folded(F.nsuper, 0);
    for (int s : F.fold_list) folded[s] = 1;
    if (node_front) std::fill(node_front, node_front + P.NP + P.NL, -1);
    std::vector<int32_t> slot_front(cross ? cr.n_pairs : 0, -1);
    for (int s = 0; s < F.nsuper; ++s) {
        int32_t* o = fronts + (size_t)BOS_SELINV_COLS * s;
        o[0] = si->cls[s]; o[1] = si->launch_of[s]; o[2] = F.k[s]; o[3] = F.r[s]; o[4] = folded[s];
        o[5] = si->h_S_off[s] >= 0;
        o[6] = si->h_out_ptr[s + 1] - si->h_out_ptr[s];
        o[7] = o[8] = o[9] = cross ? 0 : -1;
        if (node_front)
            for (int q = si->h_out_ptr[s]; q < si->h_out_ptr[s + 1]; ++q) {
                const int32_t* rec = si->h_out_rec.data() + 3 * (size_t)q;
                node_front[rec[2] == 3 ? rec[1] / 9 : P.NP + rec[1] / 4] = s;
            }
        for (int q = cross ? cr.ptr[s] : 0; cross && q < cr.ptr[s + 1]; ++q) {
            const int32_t* rec = cr.rec.data() + (size_t)kCrossRec * q;
            ++o[rec[0] >= F.k[s] ? 7 : 8];
            o[9] += rec[5];
            slot_front[rec[4]] = s;
        }
    }
    if (edge_front)
        for (int64_t e = 0; e < (int64_t)P.Mb + P.Mo; ++e)
            edge_front[e] = cross && cr.edge_slot[e] >= 0 ? slot_front[cr.edge_slot[e]] : -1;
    return 0;
}

int mf_edge_project(MfDevice* d, const double* pose, const double* lm, const bool want[4], EdgeCovResult* res, hipStream_t s,
                    std::string& err) {
    SelInv** slot = mf_selinv_slot(d);
    if (!*slot || !(*slot)->ec.arena) { err = "edge covariances: the cross records are not built"; return -1; }
    const SelInv* si = *slot;
    const EdgeCovDev& ec = si->ec;
    EdgeCovIn in;
    in.Mb = ec.Mb; in.Mo = ec.Mo;
    in.pose = pose; in.lm = lm;
    in.pose_cov = si->out; in.lm_cov = si->out + si->lm_base;
    in.pairs = ec.pairs;
    in.b_pose = ec.b_pose; in.b_lm = ec.b_lm; in.o_src = ec.o_src; in.o_dst = ec.o_dst;
    in.edge_slot = ec.edge_slot; in.edge_tr = ec.edge_tr;
    EdgeCovOut o;
    o.bearing_cross = want[0] ? ec.bearing_cross : nullptr;
    o.odom_cross = want[1] ? ec.odom_cross : nullptr;
    o.bearing_var = want[2] ? ec.bearing_var : nullptr;
    o.odom_cov = want[3] ? ec.odom_cov : nullptr;
    const hipError_t e = launch_edge_project(in, o, s);
    if (e != hipSuccess) { err = std::string("edge covariances: projection launch: ") + hipGetErrorString(e); return -2; }
    res->bearing_cross = o.bearing_cross; res->odom_cross = o.odom_cross; res->bearing_var = o.bearing_var; res->odom_cov = o.odom_cov;
    return 0;
}

int64_t mf_selinv_sigma_bytes(const MfDevice* d) {
    SelInv* const* slot = mf_selinv_slot(const_cast<MfDevice*>(d));
    return *slot ? (*slot)->sigma_bytes : 0;
}

}  // namespace dev
}  // namespace bos
