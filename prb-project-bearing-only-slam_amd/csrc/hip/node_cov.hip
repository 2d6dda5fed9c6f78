// Node covariances: the block column Sigma(:, a) = L^-T (L^-1 E_a) from the finished L panels of
// hip/multifrontal.hip (host/node_cov.hpp). All arithmetic is fp64; a front is swept by one workgroup (a
// folded landmark by one thread) that works alone: no flags, waits, tickets or atomics, a launch depends on
// the one before through stream order.
//
// node_scatter_kernel: one workgroup walks a's root path and copies the path solve's rows into the zeroed X.
// node_sweep_wave_kernel (m <= 64): one wavefront (one workgroup) per front. Lane i holds x of the front's
//   row i in registers (d doubles). A pivot lane j subtracts L(i, j) x_i for the rows below it, from the
//   last row up: x_i is broadcast by v_readlane, L(i, j) is the lane's own column of the panel, so no sum
//   crosses lanes. The panel's addresses do not depend on x: eight rows are loaded before the eight
//   dependent steps that use them, in the separator rows and in the pivot chain alike.
// node_sweep_block_kernel (64 < m <= kPairMaxM): one workgroup of four waves per front, x (m x d) in LDS.
//   The pivots are taken in blocks of 64 from the last: every wave takes columns j of the block and forms
//   t_j = y_j - sum over the rows i below the block of L(i, j) x_i, a lane summing its rows i = lane,
//   lane + 64, ... in order and the wave reducing by xor-butterfly (a fixed order); then the first wave
//   solves the block's 64 x 64 triangle in registers as the wave class does.
// node_sweep_leaf_kernel (the folded landmarks: k = 2, leaves, m <= 64): one thread per front, the wave
//   class's operations in its order. Config 3 has 200 000 of them: one wavefront each took 204 us of the
//   sweep's 420, one thread each shares no LDS, barrier or cross-lane step with its neighbours.
// node_gather_kernel: one thread per target node (host/node_cov.hpp node_cov_target).
#include "node_cov.hpp"
#include "device_mem.hpp"
#include "wave_util.hpp"

#include <algorithm>
#include <vector>

namespace bos {
namespace dev {

namespace {

constexpr int kWave = 64;
constexpr int kAhead = 8;            // panel rows loaded ahead of the steps that use them
constexpr int kBlockThreads = 256;   // the block class: four waves
constexpr int kGatherBlock = 256, kScatterBlock = 256, kLeafBlock = 256;

struct SweepArgs {
    const int32_t *k, *r, *col0, *findex, *order;
    const int64_t *L_off, *findex_off;
    const double* L;
    double* X;
    int first;   // the launch's fronts: order[first + blockIdx.x]
};

// The pivots b0 .. b0 + nb - 1 (nb <= 64) of a front, everything below them already subtracted: lane l < nb
// holds t of pivot b0 + l in acc and leaves with its x. From the last pivot up; lane l's panel entries are
// L(b0 + jl, b0 + l), its own column.
template <int D> __device__ __forceinline__ void tri_solve(const double* Ls, int m, int b0, int nb, int lane, double (&acc)[D]) {
    const double* colp = Ls + (int64_t)(b0 + lane) * m;
    const double dg_own = lane < nb ? colp[b0 + lane] : 1.0;
    for (int jb = nb - 1; jb >= 0; jb -= kAhead) {
        double row[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int jl = jb - u;
            row[u] = jl >= 0 && lane < jl ? colp[b0 + jl] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int jl = jb - u;
            if (jl >= 0) {
                const double dg = readlane_d(dg_own, jl);
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const double x = readlane_d(acc[c], jl) / dg;
                    acc[c] = lane == jl ? x : (lane < jl ? acc[c] - row[u] * x : acc[c]);
                }
            }
        }
    }
}

template <int D> __device__ void sweep_wave(const SweepArgs& a, int s) {
    const int lane = threadIdx.x;
    const int k = a.k[s], m = k + a.r[s];
    const double* Ls = a.L + a.L_off[s];
    const int32_t* fi = a.findex + a.findex_off[s];
    const int64_t at = lane < m ? fi[lane] : 0;
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = lane < m ? a.X[at * D + c] : 0.0;
    const double* colp = Ls + (int64_t)lane * m;   // a pivot lane's column
    for (int ib = m - 1; ib >= k; ib -= kAhead) {
        double e[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int i = ib - u;
            e[u] = i >= k && lane < k ? colp[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int i = ib - u;
            if (i >= k) {
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const double xi = readlane_d(x[c], i);
                    x[c] = lane < k ? x[c] - e[u] * xi : x[c];
                }
            }
        }
    }
    tri_solve<D>(Ls, m, 0, k, lane, x);
    if (lane < k) {
#pragma unroll
        for (int c = 0; c < D; ++c) a.X[at * D + c] = x[c];
    }
}

// one wavefront per workgroup, one front per wavefront
__global__ __launch_bounds__(kWave) void node_sweep_wave_kernel(const SweepArgs a, int d) {
    const int s = a.order[a.first + blockIdx.x];
    if (d == 3) sweep_wave<3>(a, s);
    else sweep_wave<2>(a, s);
}

template <int D> __device__ void sweep_block(const SweepArgs& a, int s, double* xs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k[s], m = k + a.r[s];
    const double* Ls = a.L + a.L_off[s];
    const int32_t* fi = a.findex + a.findex_off[s];
    for (int i = tid; i < m; i += kBlockThreads) {
        const int64_t at = fi[i];
#pragma unroll
        for (int c = 0; c < D; ++c) xs[i * D + c] = a.X[at * D + c];
    }
    __syncthreads();
    for (int b1 = k; b1 > 0; b1 -= kWave) {
        const int b0 = b1 > kWave ? b1 - kWave : 0, nb = b1 - b0;
        for (int jl = wave; jl < nb; jl += kBlockThreads / kWave) {
            const int j = b0 + jl;
            const double* cj = Ls + (int64_t)j * m;
            double sum[D];
#pragma unroll
            for (int c = 0; c < D; ++c) sum[c] = 0.0;
            for (int i = b1 + lane; i < m; i += kWave) {
                const double l = cj[i];
#pragma unroll
                for (int c = 0; c < D; ++c) sum[c] = fma(l, xs[i * D + c], sum[c]);
            }
#pragma unroll
            for (int c = 0; c < D; ++c)
                for (int o = 32; o > 0; o >>= 1) sum[c] += __shfl_xor(sum[c], o);
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < D; ++c) xs[j * D + c] -= sum[c];
            }
        }
        __syncthreads();
        if (wave == 0) {
            double acc[D];
#pragma unroll
            for (int c = 0; c < D; ++c) acc[c] = lane < nb ? xs[(b0 + lane) * D + c] : 0.0;
            tri_solve<D>(Ls, m, b0, nb, lane, acc);
            if (lane < nb) {
#pragma unroll
                for (int c = 0; c < D; ++c) xs[(b0 + lane) * D + c] = acc[c];
            }
        }
        __syncthreads();
    }
    double* Xs = a.X + (int64_t)a.col0[s] * D;   // the pivots' rows are consecutive
    for (int idx = tid; idx < k * D; idx += kBlockThreads) Xs[idx] = xs[idx];
}

__global__ __launch_bounds__(kBlockThreads) void node_sweep_block_kernel(const SweepArgs a, int d) {
    extern __shared__ double node_lds[];
    const int s = a.order[a.first + blockIdx.x];
    if (d == 3) sweep_block<3>(a, s, node_lds);
    else sweep_block<2>(a, s, node_lds);
}

// A folded landmark (k = 2, a leaf, m <= 64): one thread, the wave class's operations in the wave class's order
template <int D> __device__ void sweep_leaf(const SweepArgs& a, int s) {
    const int m = 2 + a.r[s];
    const double* Ls = a.L + a.L_off[s];
    const int32_t* fi = a.findex + a.findex_off[s];
    double* Xs = a.X + (int64_t)a.col0[s] * D;
    double x0[D], x1[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        x0[c] = Xs[c];
        x1[c] = Xs[D + c];
    }
    for (int i = m - 1; i >= 2; --i) {
        const double l0 = Ls[i], l1 = Ls[m + i];
        const int64_t at = fi[i];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const double xi = a.X[at * D + c];
            x0[c] -= l0 * xi;
            x1[c] -= l1 * xi;
        }
    }
    const double d0 = Ls[0], l10 = Ls[1], d1 = Ls[m + 1];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        x1[c] = x1[c] / d1;
        x0[c] = (x0[c] - l10 * x1[c]) / d0;
        Xs[c] = x0[c];
        Xs[D + c] = x1[c];
    }
}

// one thread per front; the threads share nothing
__global__ __launch_bounds__(kLeafBlock) void node_sweep_leaf_kernel(const SweepArgs a, int d, int count) {
    const int t = blockIdx.x * kLeafBlock + threadIdx.x;
    if (t >= count) return;
    const int s = a.order[a.first + t];
    if (d == 3) sweep_leaf<3>(a, s);
    else sweep_leaf<2>(a, s);
}

// one workgroup: the rows of Y (the path solve's slice, path order) to the dofs of the path's supernodes
__global__ __launch_bounds__(kScatterBlock) void node_scatter_kernel(const int32_t* k, const int32_t* r, const int32_t* parent,
                                                                       const int32_t* col0, const int32_t* start, const double* Y,
                                                                       double* X, int d) {
    int64_t base = 0;
    for (int s = *start; s >= 0; s = r[s] > 0 ? parent[s] : -1) {
        const int ks = k[s];
        double* dst = X + (int64_t)col0[s] * d;
        for (int idx = threadIdx.x; idx < ks * d; idx += kScatterBlock) dst[idx] = Y[base * d + idx];
        base += ks;
    }
}

__global__ __launch_bounds__(kGatherBlock) void node_gather_kernel(const NodeCovIn in, const NodeCovOut out) {
    const int u = blockIdx.x * kGatherBlock + threadIdx.x;
    if (u < in.NP + in.NL) node_cov_target(in, out, u);
}

}  // namespace

struct NodeCov {
    DeviceMem mem;   // the arena alone
    char* arena = nullptr;
    int NP = 0, NL = 0, max_m = 0;
    int64_t n = 0;
    std::vector<NodeCovPlan::Launch> launch;
    // per supernode, per front row, the sweep's order; per node: supernode, first dof inside it, dofs, first dof
    int32_t *col0 = nullptr, *findex = nullptr, *order = nullptr, *node_sn = nullptr, *node_loc = nullptr, *node_d = nullptr,
            *node_dof = nullptr;
    int64_t *findex_off = nullptr, *zero = nullptr;   // zero: the one Y slice's offset
    double *Y = nullptr, *X = nullptr, *out[4] = {};
};

NodeCov* node_cov_create() { return new NodeCov(); }

void node_cov_destroy(NodeCov* p) { delete p; }

int64_t node_cov_bytes(const NodeCov* p) { return p ? (int64_t)p->mem.bytes() : 0; }

bool node_cov_built(const NodeCov* p) { return p && p->arena; }

int node_cov_build(NodeCov* p, const Plan& P, const PairPaths& pp, const NodeCovPlan& np, std::string& err) {
    // one arena: [index arrays | Y | X | one node's output blocks], every part aligned to 256 bytes
    const Multifrontal& F = P.mf;
    const size_t NP = (size_t)P.NP, NL = (size_t)P.NL;
    std::vector<int32_t> nd(NP + NL);
    for (size_t u = 0; u < NP + NL; ++u) nd[u] = u < NP ? 3 : 2;
    const std::vector<int64_t> zero(1, 0);
    Arena ar(true);
    ar.add(&p->col0, F.col0);
    ar.add(&p->findex, F.findex);
    ar.add(&p->findex_off, F.findex_off);
    ar.add(&p->order, np.order);
    ar.add(&p->node_sn, pp.node_sn);
    ar.add(&p->node_loc, pp.node_loc);
    ar.add(&p->node_d, nd);
    ar.add(&p->node_dof, P.node_dof);
    ar.add(&p->zero, zero);
    ar.reserve(&p->Y, 3 * (size_t)np.max_path);
    ar.reserve(&p->X, 3 * (size_t)P.n);
    const size_t count[4] = {9 * NP, 6 * NL, 9 * NP, 4 * NL};
    for (int i = 0; i < 4; ++i) ar.reserve(&p->out[i], count[i]);
    if (!ar.commit(p->mem, &p->arena)) {
        err = "bos_node_covariances: device allocation or upload of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    p->NP = P.NP; p->NL = P.NL; p->n = P.n; p->max_m = np.max_m;
    p->launch = np.launch;
    return 0;
}

int node_cov_enqueue(NodeCov* p, const MfView& v, int a, bool fixed, const bool want[4], const double* sig, const double* pose, const double* lm,
                     hipStream_t s, hipEvent_t after_solve, NodeCovDev* out, std::string& err) {
    if (!p->arena) { err = "bos_node_covariances: the arena is not built"; return -1; }
    if (p->max_m > kPairMaxM) { err = "bos_node_covariances: a front of " + std::to_string(p->max_m) + " rows exceeds the sweep's LDS"; return -1; }
    if (a < 0 || a >= p->NP + p->NL) { err = "bos_node_covariances: bad node"; return -1; }
    const int d = a < p->NP ? 3 : 2;
    hipError_t e = hipSuccess;
    const bool any_cross = want[0] || want[1] || want[2] || want[3];
    if (!fixed && any_cross) {   // the fixed pose has no supernode: its column is zero and nothing is solved
        e = pair_path_enqueue(v, p->max_m, 1, p->node_sn + a, p->node_loc + a, p->node_d + a, p->zero, p->Y, s);
        if (e == hipSuccess) e = hipMemsetAsync(p->X, 0, (size_t)p->n * d * sizeof(double), s);
        if (e == hipSuccess) {
            node_scatter_kernel<<<1, kScatterBlock, 0, s>>>(v.k, v.r, v.parent, p->col0, p->node_sn + a, p->Y, p->X, d);
            e = hipGetLastError();
        }
        SweepArgs g;
        g.k = v.k; g.r = v.r; g.col0 = p->col0; g.findex = p->findex; g.order = p->order; g.L_off = v.L_off; g.findex_off = p->findex_off;
        g.L = v.L; g.X = p->X;
        for (size_t i = 0; i < p->launch.size() && e == hipSuccess; ++i) {
            const NodeCovPlan::Launch& L = p->launch[i];
            g.first = L.first;
            if (L.cls == kNodeCovBlock) node_sweep_block_kernel<<<L.count, kBlockThreads, (size_t)p->max_m * 3 * sizeof(double), s>>>(g, d);
            else if (L.cls == kNodeCovLeaf) node_sweep_leaf_kernel<<<(L.count + kLeafBlock - 1) / kLeafBlock, kLeafBlock, 0, s>>>(g, d, L.count);
            else node_sweep_wave_kernel<<<L.count, kWave, 0, s>>>(g, d);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && after_solve) e = hipEventRecord(after_solve, s);
    if (e == hipSuccess && any_cross) {
        NodeCovIn in;
        in.NP = p->NP; in.NL = p->NL; in.a = a; in.d = d; in.n = p->n;
        in.pose = pose; in.lm = lm; in.X = fixed ? nullptr : p->X; in.node_dof = p->node_dof; in.sig = sig;
        NodeCovOut o;
        o.cross_pose = want[0] ? p->out[0] : nullptr; o.cross_landmark = want[1] ? p->out[1] : nullptr;
        o.projected_pose = want[2] ? p->out[2] : nullptr; o.projected_landmark = want[3] ? p->out[3] : nullptr;
        const int nodes = p->NP + p->NL;
        node_gather_kernel<<<(nodes + kGatherBlock - 1) / kGatherBlock, kGatherBlock, 0, s>>>(in, o);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { err = std::string("bos_node_covariances: launch: ") + hipGetErrorString(e); return -2; }
    out->cross_pose = want[0] ? p->out[0] : nullptr; out->cross_landmark = want[1] ? p->out[1] : nullptr;
    out->projected_pose = want[2] ? p->out[2] : nullptr; out->projected_landmark = want[3] ? p->out[3] : nullptr;
    return 0;
}

}  // namespace dev
}  // namespace bos
