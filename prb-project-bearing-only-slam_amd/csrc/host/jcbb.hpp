// Joint-compatibility branch and bound (bos_jcbb): Neira & Tardos' search over the interpretation tree of
// one frame of m <= kJcbbMaxBearings bearings, on the all-pairings system of host/joint.hpp.
//
// Frame: bearing b has the candidates cand_landmark[cand_start[b] .. cand_start[b + 1]) in the caller's order;
// the frame's pairings are all (bearing, candidate) pairs in (bearing, list position) order, P <= kJointMaxM
// of them. e_all [P] and S_all [P x P] are the innovation and innovation_cov of the hypothesis made of those
// pairings (joint.hpp: same preparation, same joint_S_entry).
// Hypothesis: per bearing one of its candidates or nothing, no landmark twice. Its pairings in bearing order
// select a principal submatrix of S_all and a subvector of e_all; its prefix NIS values are those of the
// recurrence of joint.hpp on that submatrix, bit for bit. It is admissible iff every prefix j = 1 .. n is
// finite and <= gate[j - 1] (every pivot finite and positive); the empty hypothesis is admissible.
// Result: the admissible hypothesis with the most pairings; among those the smallest joint NIS (last prefix);
// among those the lexicographically smallest choice vector (a bearing's choice is its list position, nothing
// ranks after every position). A total order: the result does not depend on the order of the search.
//
// The recurrence row by row ("up-looking"): the search keeps, for the pairings chosen so far (positions
// 0 .. n - 1), the unscaled rows A_t[0 .. t], the pivots D_t = A_tt and y_t. A new pairing is row n:
//   a_j = S_all[q][q_j] (a_n = S_all[q][q]); for j = 0 .. n, for k = 0 .. j - 1 ascending:
//   a_j = a_j - (a_k / D_k) * A_jk  (A_nk = a_k, the row's own unscaled value); y = e_q, for k ascending:
//   y = y - (a_k / D_k) * y_k; D_n = a_n; prefix_n = prefix_{n-1} + (y * y) / D_n.
// For a fixed entry these are the right-looking form's operations in its order (joint_l, joint_sub,
// joint_prefix), so the bits are joint_ldl_prefix's.
// Prunings, both sound: prefix NIS never decreases in floating point (a term (y y) / D with D > 0 is >= 0 and
// rounding is monotone), so a node that is not admissible is cut with its subtree; a node whose pairings so
// far plus the later bearings with a candidate are fewer than the best count found is cut, and at equal
// potential one whose prefix already exceeds the best NIS at that count (jcbb_cut). Equal potential with a
// prefix not above the best is explored: NIS and lexicographic ties live there.
// The search is depth first, candidates in list order, then nothing. A node is a choice whose row was
// evaluated or a step "nothing"; a choice skipped for exclusivity or cut by the bound is not one. At most
// `budget` nodes are visited; the best hypothesis is updated at every accepted pairing (the hypothesis: the
// choices so far, nothing afterwards), so what an exhausted budget leaves is admissible.
//
// jcbb_search is the serial, literal form; the device kernel (hip/jcbb.hip) runs the same loop with one
// wavefront per frame, lane = column of the new row, and visits the same nodes in the same order.
#pragma once

#include <cstdint>
#include <vector>

#include "joint.hpp"

namespace bos {

constexpr int kJcbbMaxBearings = 32;                // BOS_JCBB_MAX_BEARINGS
constexpr int64_t kJcbbDefaultNodes = 1ll << 22;    // max_nodes == 0
constexpr int64_t kJcbbMaxNodes = 1ll << 26;        // larger budgets are clamped
constexpr int32_t kJcbbNothing = 0x7fffffff;        // the choice "nothing": after every list position

BOS_HD int64_t jcbb_budget(int64_t max_nodes) {
    return max_nodes == 0 ? kJcbbDefaultNodes : (max_nodes > kJcbbMaxNodes ? kJcbbMaxNodes : max_nodes);
}

// ---- the total order -----------------------------------------------------------------------------------
// > 0: (n, nis) beats (best_n, best_nis); < 0: it loses; 0: the choice vectors decide (jcbb_choice_less at
// the first bearing where they differ)
BOS_HD int jcbb_compare(int n, double nis, int best_n, double best_nis) {
    if (n != best_n) return n > best_n ? 1 : -1;
    if (nis != best_nis) return nis < best_nis ? 1 : -1;
    return 0;
}
BOS_HD bool jcbb_choice_less(int32_t a, int32_t b) { return a < b; }

// ---- the prunings --------------------------------------------------------------------------------------
BOS_HD bool jcbb_admissible(double prefix, double D, double gate) {
    return joint_pivot_ok(D) && std::fabs(prefix) <= 1.7976931348623157e308 && prefix <= gate;
}
// potential: the pairings a node's subtree can reach at most; prefix: a lower bound of its joint NIS
BOS_HD bool jcbb_cut(int potential, double prefix, int best_n, double best_nis) {
    return potential < best_n || (potential == best_n && prefix > best_nis);
}

// ---- the row extension ---------------------------------------------------------------------------------
// one subtraction of the recurrence: a - (a_k / D_k) * b
BOS_HD double jcbb_row_step(double a, double a_k, double D_k, double b) { return joint_sub(a, joint_l(a_k, D_k), b); }

// Row n from the rows 0 .. n - 1 (R, stride ld), their pivots D and their y: a [n + 1] holds the entries of
// S_all on entry and the unscaled row on return (a[n] the pivot); returns y_n from e.
BOS_HD double jcbb_extend_row(int n, const double* R, int ld, const double* D, const double* y, double* a, double e) {
    for (int j = 1; j <= n; ++j)
        for (int k = 0; k < j; ++k) a[j] = jcbb_row_step(a[j], a[k], D[k], j == n ? a[k] : R[j * ld + k]);
    for (int k = 0; k < n; ++k) e = jcbb_row_step(e, a[k], D[k], y[k]);
    return e;
}

// ---- the serial search ---------------------------------------------------------------------------------
struct JcbbFrame {
    int m = 0;                                // bearings
    const int32_t* cand_start = nullptr;      // [m + 1]; only differences and offsets from cand_start[0] are used
    const int32_t* cand_landmark = nullptr;   // [P], indexed from the frame's first pairing
    const double *S = nullptr, *e = nullptr;  // S_all (row stride ld), e_all
    int ld = 0;
    const double* gate = nullptr;             // [kJointMaxM]
    int64_t budget = kJcbbDefaultNodes;       // nodes (jcbb_budget)
    bool bound = true;                        // false: jcbb_cut is not applied (tests)
};

struct JcbbResult {
    int32_t choice[kJcbbMaxBearings];    // list position or kJcbbNothing
    double prefix[kJcbbMaxBearings];     // joint NIS of the result's pairings among bearings 0 .. b
    int n = 0;
    double nis = 0.0;
    int64_t nodes = 0;
    bool complete = true;
};

inline void jcbb_search(const JcbbFrame& f, JcbbResult& best) {
    const int m = f.m;
    best = JcbbResult();
    for (int b = 0; b < kJcbbMaxBearings; ++b) {
        best.choice[b] = kJcbbNothing;
        best.prefix[b] = 0.0;
    }
    int cnt[kJcbbMaxBearings + 1], cstart[kJcbbMaxBearings + 1], rem_after[kJcbbMaxBearings + 1];
    for (int b = 0; b < m; ++b) {
        cstart[b] = f.cand_start[b] - f.cand_start[0];
        cnt[b] = f.cand_start[b + 1] - f.cand_start[b];
    }
    rem_after[m] = 0;
    if (m > 0) rem_after[m - 1] = 0;
    for (int b = m - 2; b >= 0; --b) rem_after[b] = rem_after[b + 1] + (cnt[b + 1] > 0 ? 1 : 0);
    // the stack: per bearing the next choice, the pairings and the prefix on entry, the choice taken and the
    // prefix after it; per position the row, pivot, y, pairing and landmark
    int pos[kJcbbMaxBearings + 1], n_at[kJcbbMaxBearings + 1];
    int32_t choice[kJcbbMaxBearings];
    double pref_at[kJcbbMaxBearings + 1], pref_out[kJcbbMaxBearings];
    double R[kJointMaxM * kJointLd], D[kJointMaxM], y[kJointMaxM], a[kJointMaxM + 1];
    int32_t pq[kJointMaxM], lmk[kJointMaxM];
    int b = 0;
    pos[0] = 0; n_at[0] = 0; pref_at[0] = 0.0;
    while (b >= 0) {
        if (b == m) { --b; continue; }
        const int c = pos[b];
        if (c > cnt[b]) { --b; continue; }
        pos[b] = c + 1;
        const int n = n_at[b];
        const double pref = pref_at[b];
        const bool nothing = c == cnt[b];
        if (f.bound && jcbb_cut(n + rem_after[b] + (nothing ? 0 : 1), pref, best.n, best.nis)) continue;
        int32_t q = -1, lm = -1;
        if (!nothing) {
            q = cstart[b] + c;
            lm = f.cand_landmark[q];
            bool used = false;
            for (int t = 0; t < n; ++t) used = used || lmk[t] == lm;
            if (used) continue;
        }
        if (best.nodes >= f.budget) { best.complete = false; break; }
        ++best.nodes;
        if (nothing) {
            choice[b] = kJcbbNothing; pref_out[b] = pref;
            pos[b + 1] = 0; n_at[b + 1] = n; pref_at[b + 1] = pref;
            ++b;
            continue;
        }
        for (int j = 0; j < n; ++j) a[j] = f.S[(int64_t)q * f.ld + pq[j]];
        a[n] = f.S[(int64_t)q * f.ld + q];
        const double yn = jcbb_extend_row(n, R, kJointLd, D, y, a, f.e[q]);
        const double pnew = joint_prefix(pref, yn, a[n]);
        if (!jcbb_admissible(pnew, a[n], f.gate[n])) continue;
        for (int j = 0; j <= n; ++j) R[n * kJointLd + j] = a[j];
        D[n] = a[n]; y[n] = yn; pq[n] = q; lmk[n] = lm;
        choice[b] = c; pref_out[b] = pnew;
        pos[b + 1] = 0; n_at[b + 1] = n + 1; pref_at[b + 1] = pnew;
        // the hypothesis: the choices of bearings 0 .. b, nothing afterwards
        int cmp = jcbb_compare(n + 1, pnew, best.n, best.nis);
        for (int t = 0; t < m && cmp == 0; ++t) {
            const int32_t cur = t <= b ? choice[t] : kJcbbNothing;
            if (cur != best.choice[t]) cmp = jcbb_choice_less(cur, best.choice[t]) ? 1 : -1;
        }
        if (cmp > 0) {
            best.n = n + 1; best.nis = pnew;
            for (int t = 0; t < m; ++t) {
                best.choice[t] = t <= b ? choice[t] : kJcbbNothing;
                best.prefix[t] = t <= b ? pref_out[t] : pnew;
            }
        }
        ++b;
    }
}

// ---- argument rules ------------------------------------------------------------------------------------
// null, or what is wrong with the candidate lists and gates of n_bearings bearings (omega may be null)
inline const char* jcbb_bad_lists(int NL, int32_t n_bearings, const int32_t* cand_start, const int32_t* cand_landmark,
                                  const double* gate, int64_t max_nodes) {
    if (max_nodes < 0) return "max_nodes < 0";
    if (!gate) return "bad argument";
    for (int j = 0; j < kJointMaxM; ++j)
        if (!(gate[j] > 0.0)) return "a gate that is NaN or <= 0";
    if (!cand_start) return "bad argument";
    if (cand_start[0] != 0) return "cand_start[0] is not 0";
    for (int32_t b = 0; b < n_bearings; ++b) {
        if (cand_start[b + 1] < cand_start[b]) return "cand_start decreases";
        if (cand_start[b + 1] - cand_start[b] > kJointMaxM) return "a frame of more than BOS_JOINT_MAX_M pairings";
    }
    if (cand_start[n_bearings] > 0 && !cand_landmark) return "bad argument";
    for (int32_t b = 0; b < n_bearings; ++b)
        for (int32_t q = cand_start[b]; q < cand_start[b + 1]; ++q) {
            if (cand_landmark[q] < 0 || cand_landmark[q] >= NL) return "a landmark outside [0, NL)";
            for (int32_t r = cand_start[b]; r < q; ++r)
                if (cand_landmark[r] == cand_landmark[q]) return "a landmark listed twice for one bearing";
        }
    return nullptr;
}

inline const char* jcbb_bad_argument(int NP, int NL, int32_t n_frames, const int32_t* frame_start, const int32_t* pose, const double* z,
                                     const double* omega, const int32_t* cand_start, const int32_t* cand_landmark, const double* gate,
                                     int64_t max_nodes) {
    if (n_frames < 0 || (n_frames > 0 && !frame_start)) return "bad argument";
    if (n_frames == 0) return nullptr;
    if (frame_start[0] != 0) return "frame_start[0] is not 0";
    for (int32_t f = 0; f < n_frames; ++f) {
        if (frame_start[f + 1] < frame_start[f]) return "frame_start decreases";
        if (frame_start[f + 1] - frame_start[f] > kJcbbMaxBearings) return "a frame of more than BOS_JCBB_MAX_BEARINGS bearings";
    }
    const int32_t nb = frame_start[n_frames];
    if (nb > 0 && (!pose || !z)) return "bad argument";
    if (const char* bad = jcbb_bad_lists(NL, nb, cand_start, cand_landmark, gate, max_nodes)) return bad;
    for (int32_t f = 0; f < n_frames; ++f)
        if (cand_start[frame_start[f + 1]] - cand_start[frame_start[f]] > kJointMaxM) return "a frame of more than BOS_JOINT_MAX_M pairings";
    for (int32_t b = 0; b < nb; ++b) {
        if (pose[b] < 0 || pose[b] >= NP) return "a pose outside [0, NP)";
        if (!std::isfinite(z[b])) return "a bearing that is not finite";
        if (omega && !(std::isfinite(omega[b]) && omega[b] > 0.0)) return "an information that is not finite and positive";
    }
    return nullptr;
}

// ---- frames as all-pairings hypotheses -----------------------------------------------------------------
// hyp_start [n_frames + 1] and per pairing the pose, z and omega (1 without omega) of its bearing: the
// arguments of the joint call for the frames' all-pairings hypotheses (landmark = cand_landmark)
struct JcbbPairings {
    std::vector<int32_t> hyp_start, pose;
    std::vector<double> z, omega;
};
inline void jcbb_pairings(int32_t n_frames, const int32_t* frame_start, const int32_t* pose, const double* z, const double* omega,
                          const int32_t* cand_start, JcbbPairings& A) {
    const int32_t nb = frame_start[n_frames], np = cand_start[nb];
    A.hyp_start.resize((size_t)n_frames + 1);
    for (int32_t f = 0; f <= n_frames; ++f) A.hyp_start[f] = cand_start[frame_start[f]];
    A.pose.resize((size_t)np + 1); A.z.resize((size_t)np + 1); A.omega.resize((size_t)np + 1);
    for (int32_t b = 0; b < nb; ++b)
        for (int32_t q = cand_start[b]; q < cand_start[b + 1]; ++q) {
            A.pose[q] = pose[b]; A.z[q] = z[b]; A.omega[q] = omega ? omega[b] : 1.0;
        }
}

}  // namespace bos
