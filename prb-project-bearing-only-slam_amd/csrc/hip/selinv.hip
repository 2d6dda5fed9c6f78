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
#include "selinv.hpp"

#include <algorithm>
#include <vector>

#include "../host/plan.hpp"
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
};

constexpr int kWaveThreads = 64, kBlkThreads = 256;
constexpr int kDefaultLds = 64 * 1024;
typedef double dbl4 __attribute__((ext_vector_type(4)));

template <int T> __global__ __launch_bounds__(T) void selinv_front(const SelArgs a) {
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
}

struct Launch {
    int first, count, threads, lds;
};

template <typename X> bool put(X** p, const std::vector<X>& v, int64_t& bytes) {
    *p = nullptr;
    bytes = (int64_t)std::max<size_t>(v.size(), 1) * sizeof(X);
    if (hipMalloc((void**)p, bytes) != hipSuccess) { *p = nullptr; return false; }
    return v.empty() || hipMemcpy(*p, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice) == hipSuccess;
}

}  // namespace

struct SelInv {
    std::vector<Launch> launches;
    int32_t *list = nullptr, *out_ptr = nullptr, *out_rec = nullptr;
    int64_t *S_off = nullptr, *ws_off = nullptr;
    double *S = nullptr, *ws = nullptr, *out = nullptr;
    int64_t sigma_bytes = 0, out_count = 0, lm_base = 0;
};

void selinv_destroy(SelInv* p) {
    if (!p) return;
    void* bufs[] = {p->list, p->out_ptr, p->out_rec, p->S_off, p->ws_off, p->S, p->ws, p->out};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete p;
}

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
    const bool big_lds = hipFuncSetAttribute((const void*)selinv_front<kBlkThreads>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             blk_lds) == hipSuccess;
    (void)hipGetLastError();
    const int lds_cap = big_lds ? blk_lds : kDefaultLds;

    SelInv* si = new SelInv();
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
            delete si;
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
            } else {
                ws_off[s] = ws;   // launches follow each other on one stream: they share the workspace
                ws += k * k + 2 * r * k;
            }
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
    int64_t bytes = 0;
    bool ok = put(&si->list, list, bytes) && put(&si->out_ptr, out_ptr, bytes) && put(&si->out_rec, out_rec, bytes) &&
              put(&si->S_off, S_off, bytes) && put(&si->ws_off, ws_off, bytes);
    if (ok) { bytes = si->sigma_bytes; ok = hipMalloc((void**)&si->S, bytes) == hipSuccess; if (!ok) si->S = nullptr; }
    if (ok) { bytes = std::max<int64_t>(ws_size, 1) * (int64_t)sizeof(double); ok = hipMalloc((void**)&si->ws, bytes) == hipSuccess; if (!ok) si->ws = nullptr; }
    if (ok) { bytes = std::max<int64_t>(si->out_count, 1) * (int64_t)sizeof(double); ok = hipMalloc((void**)&si->out, bytes) == hipSuccess; if (!ok) si->out = nullptr; }
    if (!ok) {
        (void)hipGetLastError();
        err = "marginals: device allocation of " + std::to_string(bytes) + " bytes failed (Sigma-front buffer: " +
              std::to_string(si->sigma_bytes) + " bytes)";
        selinv_destroy(si);
        return -2;
    }
    *out = si;
    return 0;
}

}  // namespace

int mf_selected_inverse(MfDevice* d, const Plan& P, const double** out_dev, hipStream_t s, std::string& err) {
    SelInv** slot = mf_selinv_slot(d);
    if (!*slot) {
        const int rc = selinv_build(P, slot, err);
        if (rc) { *slot = nullptr; return rc; }
    }
    SelInv* si = *slot;
    const MfView v = mf_view(d);
    SelArgs a;
    a.k = v.k; a.r = v.r; a.parent = v.parent; a.rmap = v.rmap; a.L_off = v.L_off; a.rmap_off = v.rmap_off; a.L = v.L;
    a.out_ptr = si->out_ptr; a.out_rec = si->out_rec; a.S_off = si->S_off; a.ws_off = si->ws_off;
    a.S = si->S; a.ws = si->ws; a.out = si->out; a.lm_base = si->lm_base;
    hipError_t e = hipMemsetAsync(si->out, 0, std::max<int64_t>(si->out_count, 1) * sizeof(double), s);
    for (size_t i = 0; i < si->launches.size() && e == hipSuccess; ++i) {
        const Launch& ln = si->launches[i];
        a.list = si->list + ln.first;
        if (ln.threads == kWaveThreads) selinv_front<kWaveThreads><<<ln.count, kWaveThreads, ln.lds, s>>>(a);
        else selinv_front<kBlkThreads><<<ln.count, kBlkThreads, ln.lds, s>>>(a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { err = std::string("marginals: selected-inverse launch: ") + hipGetErrorString(e); return -2; }
    *out_dev = si->out;
    return 0;
}

int64_t mf_selinv_sigma_bytes(const MfDevice* d) {
    SelInv* const* slot = mf_selinv_slot(const_cast<MfDevice*>(d));
    return *slot ? (*slot)->sigma_bytes : 0;
}

}  // namespace dev
}  // namespace bos
