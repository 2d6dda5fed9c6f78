// Node covariances (bos_node_covariances): one node's covariance against every node, the block column
// Sigma(:, a) = H_nf^-1 E_a.
//
// With H = L L^T the column is L^-T (L^-1 E_a). L^-1 E_a is non-zero only on a's root path and is the pair
// feature's path solve (pair_cov.hpp); its rows are scattered into X (n x d doubles, row-major, permuted dof
// order, d = a's dofs), zero elsewhere. The backward substitution then visits every front once, the levels
// from the root's down and the folded landmarks after them: for front s with panel L (m x k),
//   x_j = (X[col0 + j] - sum over j < i < m of L(i, j) x_i) / L(j, j),  j = k - 1 ... 0,
// x_i for i >= k read from X at findex[i]; all d columns together. Row u's dofs of X then hold Sigma(u, a).
//
// This header holds what the device path (hip/node_cov.hip) and the host twin
// (bos_plan_mf_node_covariances) share: the sweep's launch order with the checks of everything a kernel
// indexes with, the per-target gather and projection (__host__ __device__, through edge_cov.hpp), and the
// literal host form of the sweep.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "edge_cov.hpp"
#include "pair_cov.hpp"
#include "plan.hpp"

namespace bos {

constexpr int kNodeCovWaveM = 64;   // rows of the largest front one wavefront sweeps in registers

// ---- per-target gather and projection, one thread per target node on the device ------------------------
struct NodeCovIn {
    int NP = 0, NL = 0;
    int a = 0, d = 3;                              // the query node and its dofs
    int64_t n = 0;                                 // the system's dofs: node_dof == n marks the fixed pose
    const double *pose = nullptr, *lm = nullptr;   // master state: [3 NP], [2 NL]
    const double* X = nullptr;                     // [n * d] the column; null: a is the fixed pose
    const int32_t* node_dof = nullptr;             // [NP + NL] first permuted dof
    const double* sig = nullptr;                   // [9 NP | 4 NL] the selected inverse's blocks; null without projection
};
struct NodeCovOut {   // one query's slices: [9 NP], [6 NL], [9 NP], [4 NL]; any may be null
    double *cross_pose = nullptr, *cross_landmark = nullptr, *projected_pose = nullptr, *projected_landmark = nullptr;
};

// query node of D dofs against target u of DU dofs
template <int D, int DU> BOS_HD void node_cov_target_t(const NodeCovIn& in, const NodeCovOut& o, int u) {
    const int64_t dof = in.node_dof[u];
    const bool zero = !in.X || dof >= in.n;   // the query or the target is the fixed pose
    double C[D * DU];                         // Sigma(a, u): rows a's dofs (below, an index past it is clamped where
                                              // the unrolled loop's guard already excludes the entry)
BOS_UNROLL
    for (int i = 0; i < D; ++i)
BOS_UNROLL
        for (int j = 0; j < DU; ++j) C[i * DU + j] = zero ? 0.0 : in.X[(dof + j) * D + i];
    double* co = DU == 3 ? (o.cross_pose ? o.cross_pose + 9 * (int64_t)u : nullptr)
                         : (o.cross_landmark ? o.cross_landmark + 6 * (int64_t)(u - in.NP) : nullptr);
    if (co) {
BOS_UNROLL
        for (int i = 0; i < (DU == 3 ? 9 : 6); ++i) co[i] = i < D * DU ? C[i < D * DU ? i : 0] : 0.0;
    }
    double* po = DU == 3 ? (o.projected_pose ? o.projected_pose + 9 * (int64_t)u : nullptr)
                         : (o.projected_landmark ? o.projected_landmark + 4 * (int64_t)(u - in.NP) : nullptr);
    if (!po || !in.sig) return;
    const double* sa = D == 3 ? in.sig + 9 * (int64_t)in.a : in.sig + 9 * (int64_t)in.NP + 4 * (int64_t)(in.a - in.NP);
    const double* su = DU == 3 ? in.sig + 9 * (int64_t)u : in.sig + 9 * (int64_t)in.NP + 4 * (int64_t)(u - in.NP);
    double Saa[D * D], Suu[DU * DU], out[DU == 3 ? 9 : 4];
BOS_UNROLL
    for (int i = 0; i < D * D; ++i) Saa[i] = sa[i];
BOS_UNROLL
    for (int i = 0; i < DU * DU; ++i) Suu[i] = su[i];
BOS_UNROLL
    for (int i = 0; i < (DU == 3 ? 9 : 4); ++i) out[i] = 0.0;
    if constexpr (D == DU) if (u == in.a) {   // the self-loop rule of bos_edge_covariances: all four blocks are the marginals' S_aa
BOS_UNROLL
        for (int i = 0; i < D * DU; ++i) C[i] = Saa[i < D * D ? i : 0];
    }
    if constexpr (D == 3 && DU == 3) {   // the odometry prediction a -> u
        double J[18], err[3];
        const int a = in.a;
        const double ths = in.pose[3 * a + 2];
        odometry_error_jacobian<double>(in.pose[3 * a], in.pose[3 * a + 1], ths, cos(ths), sin(ths), in.pose[3 * u], in.pose[3 * u + 1],
                                        in.pose[3 * u + 2], 0.0, 0.0, 0.0, err, J);
        edge_odom_cov(Saa, Suu, C, J, out);
    } else if constexpr (D == 3) {       // the predicted bearing of landmark u from pose a
        double J[5];
        const int a = in.a, l = u - in.NP;
        const double th = in.pose[3 * a + 2];
        (void)bearing_error_jacobian<double>(in.pose[3 * a], in.pose[3 * a + 1], cos(th), sin(th), in.lm[2 * l], in.lm[2 * l + 1], 0.0, J);
        out[0] = edge_bearing_var(Saa, Suu, C, J);
    } else if constexpr (DU == 3) {      // the predicted bearing of landmark a from pose u: Sigma(u, a) = C^T
        double J[5], Ct[6];
        const int l = in.a - in.NP;
BOS_UNROLL
        for (int i = 0; i < 3; ++i)
BOS_UNROLL
            for (int j = 0; j < 2; ++j) Ct[2 * i + j] = C[(j * DU + i) < D * DU ? j * DU + i : 0];
        const double th = in.pose[3 * u + 2];
        (void)bearing_error_jacobian<double>(in.pose[3 * u], in.pose[3 * u + 1], cos(th), sin(th), in.lm[2 * l], in.lm[2 * l + 1], 0.0, J);
        out[0] = edge_bearing_var(Suu, Saa, Ct, J);
    } else {                             // l_a - l_u
        edge_landmark_diff_cov(Saa, Suu, C, out);
    }
BOS_UNROLL
    for (int i = 0; i < (DU == 3 ? 9 : 4); ++i) po[i] = out[i];
}

BOS_HD void node_cov_target(const NodeCovIn& in, const NodeCovOut& o, int u) {
    if (in.d == 3) {
        if (u < in.NP) node_cov_target_t<3, 3>(in, o, u);
        else node_cov_target_t<3, 2>(in, o, u);
    } else {
        if (u < in.NP) node_cov_target_t<2, 3>(in, o, u);
        else node_cov_target_t<2, 2>(in, o, u);
    }
}

// ---- the sweep's launch order --------------------------------------------------------------------------
// order: every supernode once, the levels from the root's down and the folded landmarks last, inside a
// level (or the folds) class by class. launch: one entry per non-empty class of a level, in stream order.
// Classes: a front of at most kNodeCovWaveM rows is swept by one wavefront, a larger one by one workgroup;
// a folded landmark (k = 2, a leaf) of at most kNodeCovWaveM rows by one thread.
constexpr int kNodeCovWave = 0, kNodeCovBlock = 1, kNodeCovLeaf = 2;
struct NodeCovPlan {
    struct Launch { int32_t first = 0, count = 0, cls = 0; };
    std::vector<int32_t> order;
    std::vector<Launch> launch;
    int max_m = 0;       // the largest front
    int max_path = 0;    // dofs of the longest root path
};

// Builds the order and checks everything the sweep's kernels index with: findex against n, the panels
// against the factor's size (pair_paths_build has run: pp), every supernode in exactly one list, a parent
// above its child, the folded landmarks' parents. False with err.
inline bool node_cov_plan_build(const Plan& P, const PairPaths& pp, NodeCovPlan& np, std::string& err) {
    const Multifrontal& F = P.mf;
    const int ns = F.nsuper;
    const char* bad = nullptr;
    std::vector<int32_t> lev(ns, -1);   // tree level; nlevels: a folded landmark
    np = NodeCovPlan();
    np.max_m = pp.max_m;
    if ((int)F.level_ptr.size() != F.nlevels + 1 || (int)F.findex_off.size() < ns || (int)F.col0.size() < ns) bad = "malformed level lists";
    for (int l = 0; l < F.nlevels && !bad; ++l)
        for (int q = F.level_ptr[l]; q < F.level_ptr[l + 1] && !bad; ++q) {
            const int s = q >= 0 && q < (int)F.level.size() ? F.level[q] : -1;
            if (s < 0 || s >= ns || lev[s] >= 0) bad = "a supernode outside the level lists or in two of them";
            else lev[s] = l;
        }
    for (size_t q = 0; q < F.fold_list.size() && !bad; ++q) {
        const int s = F.fold_list[q];
        if (s < 0 || s >= ns || lev[s] >= 0) bad = "a folded landmark in a level list or listed twice";
        else if (F.r[s] <= 0 || F.parent[s] < 0 || F.parent[s] >= ns || lev[F.parent[s]] < 0 || lev[F.parent[s]] >= F.nlevels)
            bad = "a folded landmark without a parent in the level lists";
        else if (F.child_ptr[s + 1] != F.child_ptr[s]) bad = "a folded landmark with children";
        else lev[s] = F.nlevels;
    }
    for (int s = 0; s < ns && !bad; ++s) {
        const int k = F.k[s], m = k + F.r[s];
        const int64_t fo = F.findex_off[s];
        if (lev[s] < 0) bad = "a supernode in no list";
        else if (F.r[s] > 0 && lev[s] < F.nlevels && lev[F.parent[s]] <= lev[s]) bad = "a parent not above its child";
        else if (fo < 0 || fo + m > (int64_t)F.findex.size() || F.col0[s] < 0 || (int64_t)F.col0[s] + k > P.n) bad = "front rows outside the system";
        for (int i = 0; i < m && !bad; ++i) {
            const int32_t v = F.findex[fo + i];
            if (v < 0 || v >= P.n || (i < k && v != F.col0[s] + i)) bad = "front rows outside the system";
        }
    }
    if ((int64_t)P.node_dof.size() != (int64_t)P.NP + P.NL) bad = "malformed node layout";
    for (int u = 0; u < P.NP + P.NL && !bad; ++u) {
        const int d = u < P.NP ? 3 : 2;
        if (u == P.fixed ? P.node_dof[u] != P.n : (P.node_dof[u] < 0 || (int64_t)P.node_dof[u] + d > P.n || pp.node_sn[u] < 0))
            bad = "a node outside the system";
    }
    if (bad) { err = std::string("bos_node_covariances: ") + bad; return false; }
    auto add = [&](const std::vector<int32_t>& list, bool folds) {
        auto cls_of = [&](int32_t s) {
            const int m = F.k[s] + F.r[s];
            return m > kNodeCovWaveM ? kNodeCovBlock : (folds && F.k[s] == 2 ? kNodeCovLeaf : kNodeCovWave);
        };
        for (int cls = 0; cls < 3; ++cls) {
            NodeCovPlan::Launch L;
            L.first = (int32_t)np.order.size();
            L.cls = cls;
            for (int32_t s : list)
                if (cls_of(s) == cls) np.order.push_back(s);
            L.count = (int32_t)np.order.size() - L.first;
            if (L.count > 0) np.launch.push_back(L);
        }
    };
    std::vector<int32_t> list;
    for (int l = F.nlevels - 1; l >= 0; --l) {
        list.assign(F.level.begin() + F.level_ptr[l], F.level.begin() + F.level_ptr[l + 1]);
        add(list, false);
    }
    add(F.fold_list, true);
    int64_t longest = 0;
    for (int s = 0; s < ns; ++s) longest = std::max(longest, pp.path_dofs[s]);
    np.max_path = (int)longest;
    return true;
}

inline bool node_ids_valid(int NP, int NL, int64_t n, const int32_t* nodes) {
    for (int64_t q = 0; q < n; ++q)
        if (nodes[q] < 0 || nodes[q] >= NP + NL) return false;
    return true;
}

// ---- the literal host form -----------------------------------------------------------------------------
// X (n x d, row-major) <- L^-T X over the order of np; a pivot's sum runs from the front's last row up, the
// order of the device's wave class
inline void node_cov_backward_host(const Multifrontal& F, const NodeCovPlan& np, const double* L, int d, double* X) {
    for (int32_t s : np.order) {
        const int k = F.k[s], m = k + F.r[s];
        const double* Ls = L + F.L_off[s];
        const int32_t* fi = F.findex.data() + F.findex_off[s];
        for (int j = k - 1; j >= 0; --j)
            for (int c = 0; c < d; ++c) {
                double acc = X[(size_t)fi[j] * d + c];
                for (int i = m - 1; i > j; --i) acc -= Ls[i + (size_t)j * m] * X[(size_t)fi[i] * d + c];
                X[(size_t)fi[j] * d + c] = acc / Ls[j + (size_t)j * m];
            }
    }
}

// X <- 0, then the path solve's rows (Y: pair_path_solve_host from supernode s0) at their dofs
inline void node_cov_scatter_host(const Multifrontal& F, const PairPaths& pp, int64_t n, int s0, int d, const double* Y, double* X) {
    std::fill(X, X + (size_t)n * d, 0.0);
    int64_t base = 0;
    for (int s = s0; s >= 0; s = pp.up[s]) {
        std::copy(Y + base * d, Y + (base + F.k[s]) * d, X + (size_t)F.col0[s] * d);
        base += F.k[s];
    }
}

}  // namespace bos
