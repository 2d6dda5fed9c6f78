// Pair covariances (bos_pair_covariances): the joint covariance of two arbitrary nodes, edge or no edge.
//
// With H = L L^T, Sigma_ab = (L^-1 E_a)^T (L^-1 E_b). L^-1 E_a is non-zero only on the supernodes of the
// path from a's supernode to the root of the assembly tree, so a node needs one sparse forward solve
// along its root path (its Y slice: path_dofs rows, d = 3 or 2 columns, row-major) and a pair the dot
// products of the two slices over the dofs the paths share: the tail from the lowest common ancestor up.
//
// This header holds what the device path (hip/pair_cov.hip), its host preparation and the host twin
// (bos_plan_mf_pair_covariances) share: the static per-plan path data with the checks of everything a
// kernel indexes with, the per-query projection (__host__ __device__, through edge_cov.hpp), and the
// literal host form of the path solve and the product.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "edge_cov.hpp"
#include "plan.hpp"

namespace bos {

// ---- per-query projection, one thread per query on the device ------------------------------------------
// Blocks are row-major in the first rows * cols of a query's (or a distinct node's) nine doubles.
struct PairQueryIn {
    int NP = 0;
    const double *pose = nullptr, *lm = nullptr;          // master state: [3 NP], [2 NL]
    const int32_t *node_a = nullptr, *node_b = nullptr;   // [n] node ids (pose u: u, landmark l: NP + l)
    const int32_t *slot_a = nullptr, *slot_b = nullptr;   // [n] the node's diagonal block in diag; -1: the fixed pose
    const double* crossbuf = nullptr;                     // [9 n] Sigma(a, b); may be null when no output needs it
    const double* diag = nullptr;                         // [9 distinct nodes] Sigma(a, a); null as crossbuf
};
struct PairQueryOut {   // [9 n] each; any may be null
    double *cross = nullptr, *projected = nullptr, *cov_a = nullptr, *cov_b = nullptr;
};

BOS_HD void pair_cov_query(const PairQueryIn& in, const PairQueryOut& o, int64_t q) {
    const int a = in.node_a[q], b = in.node_b[q], sa = in.slot_a[q], sb = in.slot_b[q];
    const int da = a < in.NP ? 3 : 2, db = b < in.NP ? 3 : 2;
    const bool need_c = (o.cross || o.projected) && in.crossbuf;
    double C[9], Saa[9], Sbb[9];
BOS_UNROLL
    for (int i = 0; i < 9; ++i) {
        C[i] = need_c && i < da * db ? in.crossbuf[9 * q + i] : 0.0;
        Saa[i] = in.diag && sa >= 0 && i < da * da ? in.diag[9 * (int64_t)sa + i] : 0.0;
        Sbb[i] = in.diag && sb >= 0 && i < db * db ? in.diag[9 * (int64_t)sb + i] : 0.0;
    }
    if (o.cross) {
BOS_UNROLL
        for (int i = 0; i < 9; ++i) o.cross[9 * q + i] = C[i];
    }
    if (o.cov_a) {
BOS_UNROLL
        for (int i = 0; i < 9; ++i) o.cov_a[9 * q + i] = Saa[i];
    }
    if (o.cov_b) {
BOS_UNROLL
        for (int i = 0; i < 9; ++i) o.cov_b[9 * q + i] = Sbb[i];
    }
    if (!o.projected) return;
    double out[9];
BOS_UNROLL
    for (int i = 0; i < 9; ++i) out[i] = 0.0;
    if (da == 3 && db == 3) {   // the odometry prediction a -> b
        double J[18], err[3];
        const double ths = in.pose[3 * a + 2];
        odometry_error_jacobian<double>(in.pose[3 * a], in.pose[3 * a + 1], ths, cos(ths), sin(ths), in.pose[3 * b], in.pose[3 * b + 1],
                                        in.pose[3 * b + 2], 0.0, 0.0, 0.0, err, J);
        edge_odom_cov(Saa, Sbb, C, J, out);
    } else if (da == 3) {       // the predicted bearing of landmark b from pose a
        double J[5];
        const int l = b - in.NP;
        const double th = in.pose[3 * a + 2];
        (void)bearing_error_jacobian<double>(in.pose[3 * a], in.pose[3 * a + 1], cos(th), sin(th), in.lm[2 * l], in.lm[2 * l + 1], 0.0, J);
        out[0] = edge_bearing_var(Saa, Sbb, C, J);
    } else {                    // l_a - l_b
        double D[4];
        edge_landmark_diff_cov(Saa, Sbb, C, D);
BOS_UNROLL
        for (int i = 0; i < 4; ++i) out[i] = D[i];
    }
BOS_UNROLL
    for (int i = 0; i < 9; ++i) o.projected[9 * q + i] = out[i];
}

// ---- static per-plan path data -------------------------------------------------------------------------
struct PairPaths {
    std::vector<int32_t> node_sn, node_loc;   // [NP + NL] supernode and first dof inside its k own dofs; -1: the fixed pose
    std::vector<int32_t> up;                  // [nsuper] the supernode a path continues in: parent when r > 0, else -1
    std::vector<int32_t> depth;               // [nsuper] ancestors on the path
    std::vector<int64_t> path_dofs;           // [nsuper] sum of k over the supernode and its ancestors
    int max_m = 0;                            // the largest front, folded landmarks included
};

// Builds the path data and checks everything the kernels index with (as selinv_build does). False with
// err when a node's dofs straddle two supernodes or the tree is malformed.
inline bool pair_paths_build(const Plan& P, PairPaths& pp, std::string& err) {
    const Multifrontal& F = P.mf;
    const int ns = F.nsuper, nodes = P.NP + P.NL;
    std::vector<int32_t> out_ptr, out_rec;
    if (!selinv_records(P, out_ptr, out_rec)) { err = "bos_pair_covariances: a node's dofs are split between two supernodes"; return false; }
    pp.node_sn.assign(nodes, -1);
    pp.node_loc.assign(nodes, -1);
    pp.up.assign(ns, -1);
    pp.max_m = 0;
    std::vector<int32_t> mark;
    for (int s = 0; s < ns; ++s) {
        const int k = F.k[s], r = F.r[s], p = F.parent[s], m = k + r;
        if (k <= 0 || r < 0 || (r > 0 && (p < 0 || p >= ns || p == s)) || F.L_off[s] < 0 || F.L_off[s] + (int64_t)m * k > F.L_size) {
            err = "bos_pair_covariances: malformed supernode";
            return false;
        }
        pp.max_m = std::max(pp.max_m, m);
        if (r > 0) {
            const int mp = F.k[p] + F.r[p];
            mark.assign(mp, 0);
            for (int i = 0; i < r; ++i) {
                const int32_t v = F.rmap[F.rmap_off[s] + i];
                if (v < 0 || v >= mp || mark[v]++) { err = "bos_pair_covariances: update row outside the parent's front"; return false; }
            }
            pp.up[s] = p;
        }
        for (int q = out_ptr[s]; q < out_ptr[s + 1]; ++q) {
            const int loc = out_rec[3 * q], sz = out_rec[3 * q + 2];
            if (loc < 0 || loc + sz > k) { err = "bos_pair_covariances: node outside its supernode"; return false; }
            const int u = sz == 3 ? out_rec[3 * q + 1] / 9 : P.NP + out_rec[3 * q + 1] / 4;
            pp.node_sn[u] = s;
            pp.node_loc[u] = loc;
        }
    }
    pp.depth.assign(ns, -1);
    pp.path_dofs.assign(ns, 0);
    std::vector<int32_t> chain;
    for (int s = 0; s < ns; ++s) {
        chain.clear();
        int t = s;
        while (t >= 0 && pp.depth[t] < 0) {
            chain.push_back(t);
            t = pp.up[t];
            if ((int)chain.size() > ns) { err = "bos_pair_covariances: the assembly tree has a cycle"; return false; }
        }
        for (int i = (int)chain.size() - 1; i >= 0; --i) {
            const int c = chain[i], u = pp.up[c];
            pp.depth[c] = u < 0 ? 0 : pp.depth[u] + 1;
            pp.path_dofs[c] = (u < 0 ? 0 : pp.path_dofs[u]) + F.k[c];
        }
    }
    return true;
}

// lowest common ancestor of two supernodes (either may be the other's ancestor); -1 across two roots
inline int pair_lca(const PairPaths& pp, int a, int b) {
    while (a >= 0 && b >= 0 && pp.depth[a] > pp.depth[b]) a = pp.up[a];
    while (a >= 0 && b >= 0 && pp.depth[b] > pp.depth[a]) b = pp.up[b];
    while (a >= 0 && b >= 0 && a != b) { a = pp.up[a]; b = pp.up[b]; }
    return a >= 0 && b >= 0 ? a : -1;
}

// ids in [0, NP + NL); a mixed pair as (pose, landmark)
inline bool pair_ids_valid(int NP, int NL, int64_t n, const int32_t* node_a, const int32_t* node_b) {
    for (int64_t q = 0; q < n; ++q) {
        const int a = node_a[q], b = node_b[q];
        if (a < 0 || a >= NP + NL || b < 0 || b >= NP + NL || (a >= NP && b < NP)) return false;
    }
    return true;
}

// ---- host preparation of one batch ---------------------------------------------------------------------
// The queries [q0, q0 + nq) of a call reduced to their distinct free nodes (slot order: first use), each
// with a Y slice of len * d doubles, and per query the two slots (-1: the fixed pose), the first rows of
// the common tail in the two slices and its length c = path_dofs[LCA] (0 with the fixed pose or across
// two roots).
struct PairBatchHost {
    int64_t q0 = 0, nq = 0, y_count = 0;
    std::vector<int64_t> y_off;
    std::vector<int32_t> n_node, n_sn, n_loc, n_d, n_len;
    std::vector<int32_t> q_slot_a, q_slot_b, q_off_a, q_off_b, q_c;
};

// Takes queries from q0 on until the next one would bring the batch past max_nodes distinct nodes, max_y
// doubles of Y or max_q queries (a batch always takes at least one query). slot_of: [NP + NL] scratch, all
// -1 on entry and on return. The ids have been checked (pair_ids_valid).
inline void pair_batch_build(const Plan& P, const PairPaths& pp, int64_t n, const int32_t* node_a, const int32_t* node_b, int64_t q0,
                             int64_t max_nodes, int64_t max_y, int64_t max_q, std::vector<int32_t>& slot_of, PairBatchHost& B) {
    B = PairBatchHost();
    B.q0 = q0;
    auto cost = [&](int u) { return u == P.fixed || slot_of[u] >= 0 ? (int64_t)0 : pp.path_dofs[pp.node_sn[u]] * (u < P.NP ? 3 : 2); };
    auto slot = [&](int u) {
        if (u == P.fixed) return (int32_t)-1;
        if (slot_of[u] < 0) {
            const int s = pp.node_sn[u], d = u < P.NP ? 3 : 2;
            slot_of[u] = (int32_t)B.n_node.size();
            B.n_node.push_back(u);
            B.n_sn.push_back(s);
            B.n_loc.push_back(pp.node_loc[u]);
            B.n_d.push_back(d);
            B.n_len.push_back((int32_t)pp.path_dofs[s]);
            B.y_off.push_back(B.y_count);
            B.y_count += pp.path_dofs[s] * d;
        }
        return slot_of[u];
    };
    for (int64_t q = q0; q < n; ++q) {
        const int a = node_a[q], b = node_b[q];
        if (B.nq > 0) {
            const int64_t ya = cost(a), yb = a == b ? 0 : cost(b);
            const int64_t fresh = (ya > 0) + (yb > 0);
            if (B.nq >= max_q || (int64_t)B.n_node.size() + fresh > max_nodes || B.y_count + ya + yb > max_y) break;
        }
        const int32_t sa = slot(a), sb = slot(b);
        int32_t c = 0, oa = 0, ob = 0;
        if (sa >= 0 && sb >= 0) {
            const int l = pair_lca(pp, pp.node_sn[a], pp.node_sn[b]);
            if (l >= 0) {
                c = (int32_t)pp.path_dofs[l];
                oa = (int32_t)pp.path_dofs[pp.node_sn[a]] - c;
                ob = (int32_t)pp.path_dofs[pp.node_sn[b]] - c;
            }
        }
        B.q_slot_a.push_back(sa); B.q_slot_b.push_back(sb);
        B.q_off_a.push_back(oa); B.q_off_b.push_back(ob); B.q_c.push_back(c);
        ++B.nq;
    }
    for (int32_t u : B.n_node) slot_of[u] = -1;
}

// ---- the literal host form -----------------------------------------------------------------------------
// Y [path_dofs[s0] * d]: row t holds (L^-1 E)[dof t of the path], E the d unit columns at dofs loc .. loc +
// d - 1 of supernode s0. L: the factor's panels (Multifrontal::L_off, m x k column-major).
inline void pair_path_solve_host(const Multifrontal& F, const PairPaths& pp, const double* L, int s0, int loc, int d, double* Y) {
    std::vector<double> w((size_t)(F.k[s0] + F.r[s0]) * d, 0.0), next;
    for (int c = 0; c < d; ++c) w[(size_t)(loc + c) * d + c] = 1.0;
    int64_t base = 0;
    for (int s = s0, j0 = loc; s >= 0; j0 = 0) {
        const int k = F.k[s], r = F.r[s], m = k + r;
        const double* Ls = L + F.L_off[s];
        for (int j = j0; j < k; ++j)
            for (int c = 0; c < d; ++c) {
                const double y = w[(size_t)j * d + c] / Ls[j + (size_t)j * m];
                w[(size_t)j * d + c] = y;
                for (int i = j + 1; i < m; ++i) w[(size_t)i * d + c] -= Ls[i + (size_t)j * m] * y;
            }
        for (int i = 0; i < k * d; ++i) Y[base * d + i] = w[i];
        base += k;
        const int p = pp.up[s];
        if (p < 0) break;
        next.assign((size_t)(F.k[p] + F.r[p]) * d, 0.0);
        const int32_t* map = F.rmap.data() + F.rmap_off[s];
        for (int t = 0; t < r; ++t)
            for (int c = 0; c < d; ++c) next[(size_t)map[t] * d + c] = w[(size_t)(k + t) * d + c];
        w.swap(next);
        s = p;
    }
}

// out (row-major da x db in its first entries) = sum over t < c of Ya[offa + t][i] Yb[offb + t][j]; with
// lower (a diagonal block: Ya == Yb) only i >= j is evaluated and mirrored
inline void pair_product_host(const double* Ya, int64_t offa, int da, const double* Yb, int64_t offb, int db, int64_t c, bool lower,
                              double out[9]) {
    for (int i = 0; i < 9; ++i) out[i] = 0.0;
    for (int i = 0; i < da; ++i)
        for (int j = 0; j < (lower ? i + 1 : db); ++j) {
            double acc = 0.0;
            for (int64_t t = 0; t < c; ++t) acc += Ya[(offa + t) * da + i] * Yb[(offb + t) * db + j];
            out[i * db + j] = acc;
            if (lower) out[j * db + i] = acc;
        }
}

}  // namespace bos
