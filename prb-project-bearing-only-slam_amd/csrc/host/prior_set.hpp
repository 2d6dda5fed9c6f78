// A validated prior set (bos.h bos_set_priors), as the handle and the CPU twin keep it: the arguments'
// checks and their packing (mean, then the upper triangle of Omega) in one place.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace bos {

struct PriorSet {
    std::vector<int32_t> pose, lm;   // the node of each prior
    std::vector<double> pose_rec;    // [n][9] mean[3], Omega (00, 01, 02, 11, 12, 22)
    std::vector<double> lm_rec;      // [n][5] mean[2], Omega (00, 01, 11)
    bool empty() const { return pose.empty() && lm.empty(); }
};

namespace prior_detail {

// dim-by-dim row-major Omega: finite, bit-symmetric, no negative diagonal entry
inline bool omega_ok(const double* om, int dim, std::string& why) {
    for (int i = 0; i < dim * dim; ++i)
        if (!std::isfinite(om[i])) return why = "an information matrix that is not finite", false;
    for (int i = 0; i < dim; ++i) {
        if (om[i * dim + i] < 0.0) return why = "an information matrix with a negative diagonal entry", false;
        for (int j = 0; j < i; ++j)
            if (om[i * dim + j] != om[j * dim + i]) return why = "an information matrix that is not symmetric", false;
    }
    return true;
}

inline std::string kind_check(const char* kind, int32_t n, const int32_t* node, const double* mean, const double* omega, int dim,
                              int32_t count, int32_t fixed) {
    const std::string k(kind);
    if (n < 0) return "negative " + k + " prior count";
    if (n == 0) return "";
    if (!node || !mean || !omega) return k + " priors without their arrays";
    std::vector<char> seen((size_t)std::max<int32_t>(count, 0), 0);
    for (int32_t i = 0; i < n; ++i) {
        const std::string at = k + " prior " + std::to_string(i) + ": ";
        if (node[i] < 0 || node[i] >= count) return at + "index " + std::to_string(node[i]) + " outside [0, " + std::to_string(count) + ")";
        if (seen[node[i]]) return at + k + " " + std::to_string(node[i]) + " listed twice";
        seen[node[i]] = 1;
        if (node[i] == fixed) return at + "the fixed pose takes no prior";
        for (int d = 0; d < dim; ++d)
            if (!std::isfinite(mean[(size_t)dim * i + d])) return at + "a mean that is not finite";
        std::string why;
        if (!omega_ok(omega + (size_t)dim * dim * i, dim, why)) return at + why;
    }
    return "";
}

}  // namespace prior_detail

// Checks bos_set_priors' arguments against a problem of NP poses (pose `fixed` fixed) and NL landmarks and
// packs them into out; returns the reason they are invalid (out untouched), or "".
inline std::string prior_set_build(int32_t NP, int32_t NL, int32_t fixed, int32_t n_pose, const int32_t* pose,
                                   const double* pose_mean, const double* pose_omega, int32_t n_landmark,
                                   const int32_t* landmark, const double* landmark_mean, const double* landmark_omega,
                                   PriorSet& out) {
    std::string err = prior_detail::kind_check("pose", n_pose, pose, pose_mean, pose_omega, 3, NP, fixed);
    if (err.empty()) err = prior_detail::kind_check("landmark", n_landmark, landmark, landmark_mean, landmark_omega, 2, NL, -1);
    if (!err.empty()) return err;
    PriorSet s;
    s.pose.assign(pose, pose + n_pose);
    s.lm.assign(landmark, landmark + n_landmark);
    s.pose_rec.resize(9 * (size_t)n_pose);
    s.lm_rec.resize(5 * (size_t)n_landmark);
    for (int32_t i = 0; i < n_pose; ++i) {
        const double* m = pose_mean + 3 * (size_t)i;
        const double* o = pose_omega + 9 * (size_t)i;
        const double r[9] = {m[0], m[1], m[2], o[0], o[1], o[2], o[4], o[5], o[8]};
        for (int v = 0; v < 9; ++v) s.pose_rec[9 * (size_t)i + v] = r[v];
    }
    for (int32_t i = 0; i < n_landmark; ++i) {
        const double* m = landmark_mean + 2 * (size_t)i;
        const double* o = landmark_omega + 4 * (size_t)i;
        const double r[5] = {m[0], m[1], o[0], o[1], o[3]};
        for (int v = 0; v < 5; ++v) s.lm_rec[5 * (size_t)i + v] = r[v];
    }
    out = std::move(s);
    return "";
}

}  // namespace bos
