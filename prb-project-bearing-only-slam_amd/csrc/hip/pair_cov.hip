// Pair covariances: Sigma_ab = (L^-1 E_a)^T (L^-1 E_b) from the finished L panels of hip/multifrontal.hip
// (host/pair_cov.hpp). All arithmetic is fp64; every wave works alone: no flags, waits, tickets or atomics.
//
// pair_path_kernel: one wavefront (one workgroup) per distinct node, d = 3 or 2 right-hand sides, walking
// from the node's supernode to the root. Between fronts w (m rows x d) lives in one of two LDS buffers:
// the front's update rows are scattered through rmap into the other, zeroed, buffer, which becomes the
// parent's w. Two front classes:
//   m <= 64: one row per lane in registers, the pivot's y broadcast by v_readlane. The panel's addresses
//            do not depend on w, so eight columns are loaded (coalesced, lane = row) before the eight
//            dependent pivot steps that use them; the lane on the diagonal holds L(j, j) in the same load.
//   m > 64:  w stays in LDS, rows strided over the lanes. Four columns are loaded for a block of up to
//            384 rows, then the four pivots are applied; the first row block holds the pivot rows
//            themselves and fixes the four y (kept in registers for the remaining row blocks).
// Every row sees its pivots in ascending order in both classes, as the host twin's loop does.
// pair_product_kernel: one wavefront per block; a lane sums its rows t = lane, lane + 64, ... in order,
// then the wave reduces by xor-butterfly (a fixed order). Diagonal blocks are the pair (a, a) over the
// whole path, lower triangle evaluated and mirrored.
// pair_project_kernel: one thread per query (host/pair_cov.hpp pair_cov_query).
#include "pair_cov.hpp"
#include "device_mem.hpp"
#include "wave_util.hpp"

#include <algorithm>

namespace bos {
namespace dev {

namespace {

constexpr int kWave = 64;
constexpr int kRegCols = 8;              // m <= 64: panel columns loaded ahead of their pivots
constexpr int kLdsCols = 4, kLdsSlots = 6;   // m > 64: columns per chunk, rows per lane and row block
constexpr int kProdBlock = 256, kProjBlock = 256;

struct PathArgs {
    const int32_t *k, *r, *parent, *rmap;
    const int64_t *L_off, *rmap_off;
    const double* L;
    const int32_t *n_sn, *n_loc, *n_d;
    const int64_t* y_off;
    double* Y;
    int buf;   // doubles of one w buffer
};

template <int D> __device__ void path_solve(const PathArgs& a, int node, double* wl, double* wn) {
    const int lane = threadIdx.x;
    int s = a.n_sn[node], j0 = a.n_loc[node];
    double* Y = a.Y + a.y_off[node];
    {   // the unit columns at the node's dofs
        const int m = a.k[s] + a.r[s];
        for (int idx = lane; idx < m * D; idx += kWave) wl[idx] = 0.0;
        __syncthreads();
        if (lane < D) wl[(j0 + lane) * D + lane] = 1.0;
        __syncthreads();
    }
    int64_t base = 0;
    for (;;) {
        const int k = a.k[s], r = a.r[s], m = k + r;
        const double* Ls = a.L + a.L_off[s];
        const int p = r > 0 ? a.parent[s] : -1;
        const int mp = p >= 0 ? a.k[p] + a.r[p] : 0;
        const int32_t* rm = a.rmap + a.rmap_off[s];
        if (m <= kWave) {
            double w[D];
#pragma unroll
            for (int c = 0; c < D; ++c) w[c] = lane < m ? wl[lane * D + c] : 0.0;
            for (int jb = j0; jb < k; jb += kRegCols) {
                double col[kRegCols];
#pragma unroll
                for (int u = 0; u < kRegCols; ++u) {
                    const int j = jb + u;
                    col[u] = j < k && lane >= j && lane < m ? Ls[lane + (int64_t)j * m] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kRegCols; ++u) {
                    const int j = jb + u;
                    if (j < k) {
                        const double dg = readlane_d(col[u], j);
#pragma unroll
                        for (int c = 0; c < D; ++c) {
                            const double y = readlane_d(w[c], j) / dg;
                            w[c] = lane == j ? y : (lane > j ? w[c] - col[u] * y : w[c]);
                        }
                    }
                }
            }
            if (lane < k) {
#pragma unroll
                for (int c = 0; c < D; ++c) Y[(base + lane) * D + c] = w[c];
            }
            if (p < 0) break;
            for (int idx = lane; idx < mp * D; idx += kWave) wn[idx] = 0.0;
            __syncthreads();
            if (lane >= k && lane < m) {
                const int dst = rm[lane - k];
#pragma unroll
                for (int c = 0; c < D; ++c) wn[dst * D + c] = w[c];
            }
        } else {
            for (int jb = j0; jb < k; jb += kLdsCols) {
                double y[kLdsCols][D];
                for (int rb = jb; rb < m; rb += kWave * kLdsSlots) {
                    const bool first = rb == jb;   // the row block that holds the chunk's pivot rows
                    double col[kLdsCols][kLdsSlots];
#pragma unroll
                    for (int u = 0; u < kLdsCols; ++u)
#pragma unroll
                        for (int sl = 0; sl < kLdsSlots; ++sl) {
                            const int j = jb + u, i = rb + lane + kWave * sl;
                            col[u][sl] = j < k && i < m && i >= j ? Ls[i + (int64_t)j * m] : 0.0;
                        }
#pragma unroll
                    for (int u = 0; u < kLdsCols; ++u) {
                        const int j = jb + u;
                        if (j < k) {
                            if (first) {
                                const double dg = readlane_d(col[u][0], u);   // lane u, slot 0: row jb + u = j
#pragma unroll
                                for (int c = 0; c < D; ++c) y[u][c] = wl[j * D + c] / dg;
                            }
#pragma unroll
                            for (int sl = 0; sl < kLdsSlots; ++sl) {
                                const int i = rb + lane + kWave * sl;
                                if (i < m && i >= j) {
#pragma unroll
                                    for (int c = 0; c < D; ++c) wl[i * D + c] = i == j ? y[u][c] : wl[i * D + c] - col[u][sl] * y[u][c];
                                }
                            }
                            if (first) __syncthreads();   // the next pivot's row is in this block
                        }
                    }
                }
                __syncthreads();   // the next chunk deals the rows to other lanes
            }
            for (int idx = lane; idx < k * D; idx += kWave) Y[base * D + idx] = wl[idx];
            if (p < 0) break;
            for (int idx = lane; idx < mp * D; idx += kWave) wn[idx] = 0.0;
            __syncthreads();
            for (int t = lane; t < r; t += kWave) {
                const int dst = rm[t];
#pragma unroll
                for (int c = 0; c < D; ++c) wn[dst * D + c] = wl[(k + t) * D + c];
            }
        }
        __syncthreads();
        double* sw = wl;
        wl = wn;
        wn = sw;
        base += k;
        s = p;
        j0 = 0;
    }
}

// one wavefront per workgroup: the barriers above are the wave's own (trip counts differ between nodes)
__global__ __launch_bounds__(kWave) void pair_path_kernel(const PathArgs a) {
    extern __shared__ double pair_lds[];
    const int node = blockIdx.x;
    if (a.n_d[node] == 3) path_solve<3>(a, node, pair_lds, pair_lds + a.buf);
    else path_solve<2>(a, node, pair_lds, pair_lds + a.buf);
}

struct ProdArgs {
    int n_diag, NP;          // diagonal-block tasks (one per distinct node, or 0), then the queries' cross blocks
    int64_t n_cross;
    const int64_t* y_off;
    const int32_t *n_d, *n_len;
    const int32_t *q_a, *q_b, *q_slot_a, *q_slot_b, *q_off_a, *q_off_b, *q_c;
    const double* Y;
    double *diag, *cross;
};

__global__ __launch_bounds__(kProdBlock) void pair_product_kernel(const ProdArgs a) {
    const int64_t task = (int64_t)blockIdx.x * (kProdBlock / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (task >= a.n_diag + a.n_cross) return;
    const double *Ya, *Yb;
    double* dst;
    int da, db, c;
    int64_t oa, ob;
    const bool lower = task < a.n_diag;
    if (lower) {
        Ya = Yb = a.Y + a.y_off[task];
        da = db = a.n_d[task];
        c = a.n_len[task];
        oa = ob = 0;
        dst = a.diag + 9 * task;
    } else {
        const int64_t q = task - a.n_diag;
        const int sa = a.q_slot_a[q], sb = a.q_slot_b[q];
        da = a.q_a[q] < a.NP ? 3 : 2;
        db = a.q_b[q] < a.NP ? 3 : 2;
        c = sa >= 0 && sb >= 0 ? a.q_c[q] : 0;
        Ya = a.Y + (c > 0 ? a.y_off[sa] : 0);
        Yb = a.Y + (c > 0 ? a.y_off[sb] : 0);
        oa = a.q_off_a[q];
        ob = a.q_off_b[q];
        dst = a.cross + 9 * q;
    }
    double acc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = 0.0;
    for (int t = lane; t < c; t += kWave) {
        double ya[3], yb[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            ya[i] = i < da ? Ya[(oa + t) * da + i] : 0.0;
            yb[i] = i < db ? Yb[(ob + t) * db + i] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (!lower || j <= i) acc[i][j] = fma(ya[i], yb[j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            for (int o = 32; o > 0; o >>= 1) acc[i][j] += __shfl_xor(acc[i][j], o);
    if (lane == 0) {
        double out[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) out[e] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (i < da && j < db) out[i * db + j] = lower && j > i ? acc[j][i] : acc[i][j];
#pragma unroll
        for (int e = 0; e < 9; ++e) dst[e] = out[e];
    }
}

__global__ __launch_bounds__(kProjBlock) void pair_project_kernel(const PairQueryIn in, const PairQueryOut out, int64_t n) {
    const int64_t q = (int64_t)blockIdx.x * kProjBlock + threadIdx.x;
    if (q < n) pair_cov_query(in, out, q);
}

}  // namespace

struct PairCov {
    DeviceMem mem;           // the arena alone
    char* arena = nullptr;
    // the uploaded batch
    int32_t n_nodes = 0;
    int64_t n_queries = 0;
    bool want[4] = {false, false, false, false};
    int64_t* y_off = nullptr;
    int32_t *n_sn = nullptr, *n_loc = nullptr, *n_d = nullptr, *n_len = nullptr;
    int32_t *q_a = nullptr, *q_b = nullptr, *q_slot_a = nullptr, *q_slot_b = nullptr, *q_off_a = nullptr, *q_off_b = nullptr, *q_c = nullptr;
    double *Y = nullptr, *diag = nullptr, *cross = nullptr, *out[4] = {};
};

PairCov* pair_cov_create() { return new PairCov(); }

void pair_cov_destroy(PairCov* p) { delete p; }

int64_t pair_cov_bytes(const PairCov* p) { return p ? (int64_t)p->mem.bytes() : 0; }

namespace {
int upload_batch(PairCov* p, const PairCovBatch& b, const bool want[4], bool need_diag, bool need_cross, std::string& err) {
    // one arena: [index arrays | Y | diagonal blocks | cross blocks | outputs], every part aligned to 256 bytes
    // (an empty one keeps an element's room); it only grows
    const size_t nn = (size_t)b.n_nodes, nq = (size_t)b.n_queries;
    Arena ar(true);
    ar.add(&p->y_off, b.y_off, nn);
    ar.add(&p->n_sn, b.n_sn, nn); ar.add(&p->n_loc, b.n_loc, nn); ar.add(&p->n_d, b.n_d, nn); ar.add(&p->n_len, b.n_len, nn);
    ar.add(&p->q_a, b.q_a, nq); ar.add(&p->q_b, b.q_b, nq); ar.add(&p->q_slot_a, b.q_slot_a, nq); ar.add(&p->q_slot_b, b.q_slot_b, nq);
    ar.add(&p->q_off_a, b.q_off_a, nq); ar.add(&p->q_off_b, b.q_off_b, nq); ar.add(&p->q_c, b.q_c, nq);
    ar.reserve(&p->Y, (size_t)b.y_count);
    ar.reserve(&p->diag, need_diag ? 9 * nn : 0);
    ar.reserve(&p->cross, need_cross ? 9 * nq : 0);
    for (int i = 0; i < 4; ++i) ar.reserve(&p->out[i], want[i] ? 9 * nq : 0);
    bool ok;
    if (ar.bytes() > p->mem.bytes()) {
        p->mem.release(p->arena);
        ok = ar.commit(p->mem, &p->arena);
    } else {
        ok = ar.place(p->arena);
    }
    if (!ok) {
        err = "bos_pair_covariances: device allocation or upload of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    p->n_nodes = b.n_nodes;
    p->n_queries = b.n_queries;
    for (int i = 0; i < 4; ++i) {
        p->want[i] = want[i];
        if (!want[i]) p->out[i] = nullptr;
    }
    if (!need_diag) p->diag = nullptr;
    if (!need_cross) p->cross = nullptr;
    return 0;
}
}  // namespace

int pair_cov_upload(PairCov* p, const PairCovBatch& b, const bool want[4], std::string& err) {
    return upload_batch(p, b, want, want[1] || want[2] || want[3], want[0] || want[1], err);
}

int pair_cov_upload_blocks(PairCov* p, const PairCovBatch& b, std::string& err) {
    const bool none[4] = {false, false, false, false};
    return upload_batch(p, b, none, true, true, err);
}

hipError_t pair_path_enqueue(const MfView& v, int max_m, int n_nodes, const int32_t* n_sn, const int32_t* n_loc, const int32_t* n_d,
                             const int64_t* y_off, double* Y, hipStream_t s) {
    if (n_nodes <= 0) return hipSuccess;
    PathArgs a;
    a.k = v.k; a.r = v.r; a.parent = v.parent; a.rmap = v.rmap; a.L_off = v.L_off; a.rmap_off = v.rmap_off; a.L = v.L;
    a.n_sn = n_sn; a.n_loc = n_loc; a.n_d = n_d; a.y_off = y_off; a.Y = Y;
    a.buf = max_m * 3;
    pair_path_kernel<<<n_nodes, kWave, 2 * (size_t)a.buf * sizeof(double), s>>>(a);
    return hipGetLastError();
}

namespace {
// the path solve and the products of the uploaded batch
hipError_t enqueue_blocks(PairCov* p, const MfView& v, int max_m, int NP, hipStream_t s, hipEvent_t after_solve) {
    hipError_t e = pair_path_enqueue(v, max_m, p->n_nodes, p->n_sn, p->n_loc, p->n_d, p->y_off, p->Y, s);
    if (e == hipSuccess && after_solve) e = hipEventRecord(after_solve, s);
    ProdArgs g;
    g.n_diag = p->diag ? p->n_nodes : 0;
    g.n_cross = p->cross ? p->n_queries : 0;
    g.NP = NP;
    g.y_off = p->y_off; g.n_d = p->n_d; g.n_len = p->n_len;
    g.q_a = p->q_a; g.q_b = p->q_b; g.q_slot_a = p->q_slot_a; g.q_slot_b = p->q_slot_b; g.q_off_a = p->q_off_a; g.q_off_b = p->q_off_b;
    g.q_c = p->q_c;
    g.Y = p->Y; g.diag = p->diag; g.cross = p->cross;
    const int64_t tasks = g.n_diag + g.n_cross, per = kProdBlock / kWave;
    if (e == hipSuccess && tasks > 0) {
        pair_product_kernel<<<(unsigned)((tasks + per - 1) / per), kProdBlock, 0, s>>>(g);
        e = hipGetLastError();
    }
    return e;
}

int enqueue_checks(const PairCov* p, int max_m, std::string& err) {
    if (!p->arena) { err = "bos_pair_covariances: no batch uploaded"; return -1; }
    if (max_m > kPairMaxM) { err = "bos_pair_covariances: a front of " + std::to_string(max_m) + " rows exceeds the path solve's LDS"; return -1; }
    return 0;
}
}  // namespace

int pair_cov_enqueue_blocks(PairCov* p, const MfView& v, int max_m, int NP, hipStream_t s, hipEvent_t after_solve, const double** diag,
                            const double** cross, std::string& err) {
    if (enqueue_checks(p, max_m, err)) return -1;
    const hipError_t e = enqueue_blocks(p, v, max_m, NP, s, after_solve);
    if (e != hipSuccess) { err = std::string("bos_pair_covariances: launch: ") + hipGetErrorString(e); return -2; }
    *diag = p->diag;
    *cross = p->cross;
    return 0;
}

int pair_cov_enqueue(PairCov* p, const MfView& v, int max_m, int NP, const double* pose, const double* lm, hipStream_t s,
                     hipEvent_t after_solve, PairCovOut* out, std::string& err) {
    if (enqueue_checks(p, max_m, err)) return -1;
    hipError_t e = enqueue_blocks(p, v, max_m, NP, s, after_solve);
    if (e == hipSuccess && p->n_queries > 0) {
        PairQueryIn in;
        in.NP = NP; in.pose = pose; in.lm = lm;
        in.node_a = p->q_a; in.node_b = p->q_b; in.slot_a = p->q_slot_a; in.slot_b = p->q_slot_b;
        in.crossbuf = p->cross; in.diag = p->diag;
        PairQueryOut o;
        o.cross = p->out[0]; o.projected = p->out[1]; o.cov_a = p->out[2]; o.cov_b = p->out[3];
        pair_project_kernel<<<(unsigned)((p->n_queries + kProjBlock - 1) / kProjBlock), kProjBlock, 0, s>>>(in, o, p->n_queries);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { err = std::string("bos_pair_covariances: launch: ") + hipGetErrorString(e); return -2; }
    out->cross = p->out[0]; out->projected = p->out[1]; out->cov_a = p->out[2]; out->cov_b = p->out[3];
    return 0;
}

}  // namespace dev
}  // namespace bos
