// Joint compatibility (bos_joint_compatibility): the joint NIS of a hypothesis of m <= kJointMaxM pairings
// (bearing z_i taken from pose p_i, assigned to landmark l_i, information omega_i),
//   d2 = e^T S^-1 e,  S = J Sigma J^T + R  over the stacked innovation (Neira & Tardos' joint compatibility).
//
// e_i: bearing_error at the fp64 master state, fp64 cos / sin (the association's assoc_innovation; z is not
//      wrapped first).  J_i: the 1 x 5 bearing Jacobian over [pose dofs | landmark dofs], z passed as zero.
// S_ii = edge_bearing_var(Sigma_pp, Sigma_ll, Sigma_pl, J_i) + 1.0 / omega_i: the pair call's projected[0]
//      for (p_i, NP + l_i) plus 1.0 / omega_i, bit for bit (joint_S_diag).
// S_ij (i > j) = J_i C_ij J_j^T (joint_S_offdiag), C_ij the 5 x 5 matrix of the four blocks Sigma(p_i, p_j),
//      Sigma(p_i, l_j), Sigma(l_i, p_j), Sigma(l_i, l_j), each the pair call's block of that node pair (read
//      transposed where the pair call has the opposite order; exactly zero with the fixed pose; a node with
//      itself: its cov_a). Order: t_r = sum over c = 0 .. 4 ascending of C[r][c] * J_j[c], starting from the
//      first product; then sum over r = 0 .. 4 ascending of J_i[r] * t_r, likewise. No FP contraction.
//      S_ji is the same value.
// LDL^T and the prefix NIS, right-looking, one IEEE operation at a time (joint_l, joint_sub, joint_prefix; no
// FP contraction), A the working copy of S and y of e. For k = 0 .. m - 1:
//      D_k = A_kk;  for i > k: l_ik = A_ik / D_k;  for i > k and k < j <= i: A_ij = A_ij - l_ik * A_jk (A_jk
//      unscaled);  for i > k: y_i = y_i - l_ik * y_k;  prefix_k = prefix_{k-1} + (y_k * y_k) / D_k.
//      From the first D_k that is not finite and positive on, every prefix is NaN.
// A caller reproduces every bit of the prefixes from the returned e and S.
//
// This header holds what the device kernel (hip/joint.hip), its host preparation and the host twin
// (bos_plan_mf_joint_compatibility) share: the argument rules, the expressions above, the serial recurrence
// and the batch builder that reduces a batch of hypotheses to distinct nodes, distinct node pairs and a table
// from every lower entry (i, j) of a hypothesis to the slots of its blocks.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "associate.hpp"
#include "pair_cov.hpp"

namespace bos {

constexpr int kJointMaxM = 32;   // BOS_JOINT_MAX_M
constexpr int kJointLd = 33;     // row stride of the working copy of S (the kernel's LDS padding)
constexpr int kJointDenseNodes = 512;   // a batch of at most this many nodes marks its pairs in a dense table

// ---- block references ----------------------------------------------------------------------------------
// A table entry names one block: -1 the zero block; otherwise 4 * slot + 2 * diagonal + transposed, slot an
// index into the batch's diagonal blocks (one per distinct node) or cross blocks (one per distinct pair).
constexpr int32_t kJointZero = -1;
BOS_HD int32_t joint_ref(int32_t slot, bool diag, bool tr) { return 4 * slot + (diag ? 2 : 0) + (tr ? 1 : 0); }

// out (rows x cols, row-major) = the referenced block, read transposed when the reference says so (the
// stored block is then cols x rows)
template <int ROWS, int COLS> BOS_HD void joint_gather(int32_t ref, const double* diag, const double* cross, double* out) {
    const double* src = ref < 0 ? nullptr : ((ref & 2) ? diag : cross) + 9 * (int64_t)(ref >> 2);
    const bool tr = ref >= 0 && (ref & 1);
BOS_UNROLL
    for (int r = 0; r < ROWS; ++r)
BOS_UNROLL
        for (int c = 0; c < COLS; ++c) out[r * COLS + c] = src ? (tr ? src[c * ROWS + r] : src[r * COLS + c]) : 0.0;
}

// ---- the expressions -----------------------------------------------------------------------------------
BOS_HD double joint_S_diag(const double Spp[9], const double Sll[4], const double Cpl[6], const double J[5], double omega) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double var = edge_bearing_var(Spp, Sll, Cpl, J);
    return var + 1.0 / omega;
}

// J_i C J_j^T, C = [[Cpp (3 x 3), Cpl (3 x 2)], [Clp (2 x 3), Cll (2 x 2)]] row-major blocks
BOS_HD double joint_S_offdiag(const double Cpp[9], const double Cpl[6], const double Clp[6], const double Cll[4], const double Ji[5],
                              const double Jj[5]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double t[5];
BOS_UNROLL
    for (int r = 0; r < 3; ++r) {
        double acc = Cpp[3 * r] * Jj[0];
        acc = acc + Cpp[3 * r + 1] * Jj[1];
        acc = acc + Cpp[3 * r + 2] * Jj[2];
        acc = acc + Cpl[2 * r] * Jj[3];
        acc = acc + Cpl[2 * r + 1] * Jj[4];
        t[r] = acc;
    }
BOS_UNROLL
    for (int r = 0; r < 2; ++r) {
        double acc = Clp[3 * r] * Jj[0];
        acc = acc + Clp[3 * r + 1] * Jj[1];
        acc = acc + Clp[3 * r + 2] * Jj[2];
        acc = acc + Cll[2 * r] * Jj[3];
        acc = acc + Cll[2 * r + 1] * Jj[4];
        t[3 + r] = acc;
    }
    double s = Ji[0] * t[0];
    s = s + Ji[1] * t[1];
    s = s + Ji[2] * t[2];
    s = s + Ji[3] * t[3];
    s = s + Ji[4] * t[4];
    return s;
}

// e and J of one pairing at the master state
BOS_HD double joint_innovation(const double* pose, const double* lm, int p, int l, double z, double J[5]) {
    const AssocFrame f = assoc_frame(pose, p);
    (void)bearing_error_jacobian<double>(f.px, f.py, f.c, f.s, lm[2 * l], lm[2 * l + 1], 0.0, J);
    return assoc_innovation(f, lm[2 * l], lm[2 * l + 1], z);
}

// What an S entry reads: the master state, the batch's blocks and one hypothesis's pairings and table
struct JointEntryIn {
    const double *pose = nullptr, *lm = nullptr;      // master state
    const double *diag = nullptr, *cross = nullptr;   // [9 distinct nodes], [9 distinct pairs]
    const int32_t* tab = nullptr;                     // the hypothesis's table: 4 references per lower entry, row by row
    const double* J = nullptr;                        // [5 m] the hypothesis's Jacobians
    const double* omega = nullptr;                    // [m]
};

// lower entry (i, j), j <= i, of S. Table entry i (i + 1) / 2 + j: for i > j the blocks (p_i, p_j), (p_i, l_j),
// (l_i, p_j), (l_i, l_j); for i == j the blocks (p_i, p_i), (p_i, l_i), unused, (l_i, l_i).
BOS_HD double joint_S_entry(const JointEntryIn& in, int i, int j) {
    const int32_t* ref = in.tab + 4 * (i * (i + 1) / 2 + j);
    double Cpp[9], Cpl[6], Clp[6], Cll[4];
    joint_gather<3, 3>(ref[0], in.diag, in.cross, Cpp);
    joint_gather<3, 2>(ref[1], in.diag, in.cross, Cpl);
    joint_gather<2, 2>(ref[3], in.diag, in.cross, Cll);
    if (i == j) return joint_S_diag(Cpp, Cll, Cpl, in.J + 5 * i, in.omega[i]);
    joint_gather<2, 3>(ref[2], in.diag, in.cross, Clp);
    return joint_S_offdiag(Cpp, Cpl, Clp, Cll, in.J + 5 * i, in.J + 5 * j);
}

// ---- the recurrence's operations -----------------------------------------------------------------------
BOS_HD bool joint_pivot_ok(double D) { return std::fabs(D) <= 1.7976931348623157e308 && D > 0.0; }
BOS_HD double joint_nan() { return __builtin_nan(""); }
BOS_HD double joint_l(double a_ik, double D) { return a_ik / D; }
BOS_HD double joint_sub(double a, double l, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a - l * b;
}
BOS_HD double joint_prefix(double prev, double y, double D) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return prev + (y * y) / D;
}

// The serial form: A [m x ld] (lower triangle read and overwritten), y [m] (overwritten), prefix [m]
inline void joint_ldl_prefix(int m, double* A, int ld, double* y, double* prefix) {
    double prev = 0.0;
    int k = 0;
    for (; k < m; ++k) {
        const double D = A[k * ld + k];
        if (!joint_pivot_ok(D)) break;
        for (int i = k + 1; i < m; ++i) {
            const double l = joint_l(A[i * ld + k], D);
            for (int j = k + 1; j <= i; ++j) A[i * ld + j] = joint_sub(A[i * ld + j], l, A[j * ld + k]);
            y[i] = joint_sub(y[i], l, y[k]);
        }
        prev = joint_prefix(prev, y[k], D);
        prefix[k] = prev;
    }
    for (; k < m; ++k) prefix[k] = joint_nan();
}

// ---- argument rules ------------------------------------------------------------------------------------
// null, or what is wrong (omega may be null: 1 for every pairing)
inline const char* joint_bad_argument(int NP, int NL, int32_t n_hyp, const int32_t* hyp_start, const int32_t* pose,
                                      const int32_t* landmark, const double* z, const double* omega) {
    if (n_hyp < 0 || (n_hyp > 0 && !hyp_start)) return "bad argument";
    if (n_hyp == 0) return nullptr;
    if (hyp_start[0] != 0) return "hyp_start[0] is not 0";
    for (int32_t h = 0; h < n_hyp; ++h) {
        if (hyp_start[h + 1] < hyp_start[h]) return "hyp_start decreases";
        if (hyp_start[h + 1] - hyp_start[h] > kJointMaxM) return "a hypothesis of more than BOS_JOINT_MAX_M pairings";
    }
    const int32_t n = hyp_start[n_hyp];
    if (n > 0 && (!pose || !landmark || !z)) return "bad argument";
    for (int32_t q = 0; q < n; ++q) {
        if (pose[q] < 0 || pose[q] >= NP) return "a pose outside [0, NP)";
        if (landmark[q] < 0 || landmark[q] >= NL) return "a landmark outside [0, NL)";
        if (!std::isfinite(z[q])) return "a bearing that is not finite";
        if (omega && !(std::isfinite(omega[q]) && omega[q] > 0.0)) return "an information that is not finite and positive";
    }
    return nullptr;
}

// ---- host preparation of one batch ---------------------------------------------------------------------
// The hypotheses [h0, h0 + nh) of a call: `pairs` reduces their node pairs to the distinct ones (a pair is
// (min node, max node), so a mixed one is (pose, landmark) as the pair call wants it; pairs with the fixed
// pose and of a node with itself are not listed, except a pairing's own (pose, landmark), which is always
// there so that every node of the batch is met), built by pair_batch_build, which also reduces them to the
// distinct free nodes. tab_off[h - h0]: the first table entry of h (entries, 4 references each); s_off: the
// first double of its m x m block in the batch's innovation_cov.
struct JointBatchHost {
    int32_t h0 = 0, nh = 0;
    int64_t n_entries = 0, s_count = 0;
    std::vector<int32_t> pair_a, pair_b;
    PairBatchHost pairs;
    std::vector<int64_t> tab_off, s_off;
    std::vector<int32_t> tab;
};

// Takes whole hypotheses from h0 on until the next one would bring the batch past max_y doubles of Y, max_hyp
// hypotheses or max_pairs node pairs before the reduction (m (2 m - 1) + m per hypothesis; a batch always takes
// at least one). slot_of: [NP + NL] scratch, all -1 on entry and on return. dense_nodes: the largest batch (in nodes)
// that marks its pairs in a dense table; both ways give the same batch. The arguments have been checked (joint_bad_argument).
inline void joint_batch_build(const Plan& P, const PairPaths& pp, int32_t n_hyp, const int32_t* hyp_start, const int32_t* pose,
                              const int32_t* landmark, int32_t h0, int64_t max_y, int64_t max_hyp, int64_t max_pairs,
                              std::vector<int32_t>& slot_of, JointBatchHost& B, int64_t dense_nodes = kJointDenseNodes) {
    B = JointBatchHost();
    B.h0 = h0;
    // 1. the hypotheses; slot_of numbers the nodes met (the fixed pose too): -2 - local id
    std::vector<int32_t> met;
    int64_t y = 0, raw_pairs = 0;
    for (int32_t h = h0; h < n_hyp; ++h) {
        const int32_t q0 = hyp_start[h], m = hyp_start[h + 1] - q0;
        const size_t met0 = met.size();
        int64_t add = 0;
        for (int32_t q = q0; q < q0 + m; ++q)
            for (int u : {(int)pose[q], P.NP + (int)landmark[q]})
                if (slot_of[u] == -1) {
                    slot_of[u] = -2 - (int32_t)met.size();
                    met.push_back(u);
                    if (u != P.fixed) add += pp.path_dofs[pp.node_sn[u]] * (u < P.NP ? 3 : 2);
                }
        const int64_t hp = (int64_t)m * (2 * m - 1) + m;
        if (B.nh > 0 && (B.nh >= max_hyp || y + add > max_y || raw_pairs + hp > max_pairs)) {
            for (size_t i = met0; i < met.size(); ++i) slot_of[met[i]] = -1;
            met.resize(met0);
            break;
        }
        y += add;
        raw_pairs += hp;
        ++B.nh;
    }
    const int32_t p_lo = hyp_start[h0], n_pairings = hyp_start[h0 + B.nh] - p_lo;
    const int64_t nl = (int64_t)met.size();
    std::vector<int32_t> lp((size_t)n_pairings), ll((size_t)n_pairings);   // a pairing's local pose and landmark
    for (int32_t q = 0; q < n_pairings; ++q) {
        lp[q] = -2 - slot_of[pose[p_lo + q]];
        ll[q] = -2 - slot_of[P.NP + landmark[p_lo + q]];
    }
    // 2. the distinct node pairs: sort-unique on (min node << 32 | max node). With few nodes (JCBB branches
    // share most of their pairs) a pair is listed once: ps[local(min) * nl + local(max)] marks it, then
    // holds its slot.
    const bool dense = nl <= dense_nodes;
    std::vector<int32_t> ps;
    if (dense) ps.assign((size_t)(nl * nl), -1);
    std::vector<uint64_t> keys;
    auto key = [](int a, int b) { return ((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b); };
    auto listed = [&](int a, int b) { return a != b && a != P.fixed && b != P.fixed; };
    auto note = [&](int a, int la, int b, int lb) {
        if (dense) {
            int32_t& slot = a < b ? ps[(size_t)(la * nl + lb)] : ps[(size_t)(lb * nl + la)];
            if (slot != -1) return;
            slot = 0;
        }
        keys.push_back(key(a, b));
    };
    for (int32_t h = h0; h < h0 + B.nh; ++h) {
        const int32_t q0 = hyp_start[h], m = hyp_start[h + 1] - q0, r0 = q0 - p_lo;
        for (int32_t i = 0; i < m; ++i) {
            const int pi = pose[q0 + i], li = P.NP + landmark[q0 + i], lpi = lp[r0 + i], lli = ll[r0 + i];
            note(pi, lpi, li, lli);
            for (int32_t j = 0; j < i; ++j) {
                const int pj = pose[q0 + j], lj = P.NP + landmark[q0 + j], lpj = lp[r0 + j], llj = ll[r0 + j];
                if (listed(pi, pj)) note(pi, lpi, pj, lpj);
                if (listed(pi, lj)) note(pi, lpi, lj, llj);
                if (listed(li, pj)) note(li, lli, pj, lpj);
                if (listed(li, lj)) note(li, lli, lj, llj);
            }
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    B.pair_a.resize(keys.size());
    B.pair_b.resize(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
        B.pair_a[i] = (int32_t)(keys[i] >> 32);
        B.pair_b[i] = (int32_t)(keys[i] & 0xffffffffu);
        if (dense) ps[(size_t)((-2 - slot_of[B.pair_a[i]]) * nl + (-2 - slot_of[B.pair_b[i]]))] = (int32_t)i;
    }
    // 3. the distinct nodes, their Y slices and the pairs' common tails
    for (int32_t u : met) slot_of[u] = -1;
    pair_batch_build(P, pp, (int64_t)keys.size(), B.pair_a.data(), B.pair_b.data(), 0, INT64_MAX, INT64_MAX, INT64_MAX, slot_of, B.pairs);
    std::vector<int32_t> dslot((size_t)nl, -1);   // a local node's diagonal block
    for (int64_t i = 0; i < nl; ++i) slot_of[met[i]] = (int32_t)i;
    for (size_t i = 0; i < B.pairs.n_node.size(); ++i) dslot[slot_of[B.pairs.n_node[i]]] = (int32_t)i;
    for (int32_t u : met) slot_of[u] = -1;
    // 4. the tables
    auto block = [&](int a, int la, int b, int lb) {   // Sigma(a, b)
        if (a == P.fixed || b == P.fixed) return kJointZero;
        if (a == b) return joint_ref(dslot[la], true, false);
        const int32_t slot = dense ? (a < b ? ps[(size_t)(la * nl + lb)] : ps[(size_t)(lb * nl + la)])
                                   : (int32_t)(std::lower_bound(keys.begin(), keys.end(), key(a, b)) - keys.begin());
        return joint_ref(slot, false, a > b);
    };
    B.tab.reserve(2 * (size_t)raw_pairs);
    for (int32_t h = h0; h < h0 + B.nh; ++h) {
        const int32_t q0 = hyp_start[h], m = hyp_start[h + 1] - q0, r0 = q0 - p_lo;
        B.tab_off.push_back(B.n_entries);
        B.s_off.push_back(B.s_count);
        B.n_entries += (int64_t)m * (m + 1) / 2;
        B.s_count += (int64_t)m * m;
        for (int32_t i = 0; i < m; ++i) {
            const int pi = pose[q0 + i], li = P.NP + landmark[q0 + i], lpi = lp[r0 + i], lli = ll[r0 + i];
            for (int32_t j = 0; j <= i; ++j) {
                const int pj = pose[q0 + j], lj = P.NP + landmark[q0 + j], lpj = lp[r0 + j], llj = ll[r0 + j];
                if (i == j) {
                    // the pairing's own blocks: a fixed pose's cross block is the pair call's zero block
                    B.tab.push_back(block(pi, lpi, pi, lpi));
                    B.tab.push_back(block(pi, lpi, li, lli));
                    B.tab.push_back(kJointZero);
                    B.tab.push_back(block(li, lli, li, lli));
                } else {
                    B.tab.push_back(block(pi, lpi, pj, lpj));
                    B.tab.push_back(block(pi, lpi, lj, llj));
                    B.tab.push_back(block(li, lli, pj, lpj));
                    B.tab.push_back(block(li, lli, lj, llj));
                }
            }
        }
    }
}

}  // namespace bos
