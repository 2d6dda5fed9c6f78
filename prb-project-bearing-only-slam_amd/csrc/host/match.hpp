// Node matching (bos_match_landmarks, bos_match_poses): the two gates that, with the bearing association,
// answer what the covariance calls were built for.
//
// Landmark match (are two landmarks one?): query landmark a against every landmark l != a,
//   d = l_a - l_l,  C = cov(l_a - l_l) (bos_node_covariances' projected_landmark of node NP + a, lower
//   triangle c00, c10, c11),  d2 = d^T C^-1 d  through the LDL^T of C:
//   D0 = c00, t = c10 / D0, D1 = c11 - t c10, y1 = d1 - t d0, d2 = (d0 d0) / D0 + (y1 y1) / D1.
// Pose match (which old pose closes a loop?): a relative-pose measurement z = (x, y, theta) in the frame of
// pose a with information Omega against every pose u,
//   e = the odometry error of (a, u, z),  S = P + R, P = projected_pose of node a (lower triangle),
//   R = Omega^-1,  nis = e^T S^-1 e  through the LDL^T of S (match_pose_nis below).
// A pivot that is not finite and positive gives NaN, written as such. Every expression is evaluated with
// plain IEEE + - * / in the order written (no FP contraction, no sqrt), so a caller reproduces a score
// from the listed details. Order and gate are the association's (assoc_less / assoc_inside).
//
// This header holds what the device kernels (hip/match.hip) and the host twins
// (bos_plan_mf_match_landmarks / _poses) share: the expressions, R, and the argument rules.
#pragma once

#include <cmath>
#include <cstdint>

#include "associate.hpp"

namespace bos {

constexpr int kMatchMaxK = kAssocMaxK;   // BOS_MATCH_MAX_K

BOS_HD double match_nan() { return __builtin_nan(""); }

// a pivot of either LDL^T: finite and positive
BOS_HD bool match_pivot_ok(double D) { return std::fabs(D) <= 1.7976931348623157e308 && D > 0.0; }

// ---- landmark match ------------------------------------------------------------------------------------
BOS_HD void match_landmark_diff(double ax, double ay, double lx, double ly, double d[2]) {
    d[0] = ax - lx;
    d[1] = ay - ly;
}

BOS_HD double match_landmark_d2(const double d[2], double c00, double c10, double c11) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double D0 = c00;
    if (!match_pivot_ok(D0)) return match_nan();
    const double t = c10 / D0;
    const double D1 = c11 - t * c10;
    if (!match_pivot_ok(D1)) return match_nan();
    const double y1 = d[1] - t * d[0];
    return (d[0] * d[0]) / D0 + (y1 * y1) / D1;
}

// ---- pose match ----------------------------------------------------------------------------------------
// the query pose's frame: the pose and the fp64 cos / sin of its angle
struct MatchFrame { double x, y, th, c, s; };

BOS_HD MatchFrame match_frame(const double* pose, int a) {
    MatchFrame f;
    f.x = pose[3 * a]; f.y = pose[3 * a + 1]; f.th = pose[3 * a + 2];
    f.c = cos(f.th); f.s = sin(f.th);
    return f;
}

BOS_HD void match_pose_error(const MatchFrame& f, double xu, double yu, double thu, const double z[3], double e[3]) {
    double J[18];
    odometry_error_jacobian<double>(f.x, f.y, f.th, f.c, f.s, xu, yu, thu, z[0], z[1], z[2], e, J);
}

// A symmetric 3 x 3 matrix's lower triangle is kept as [m00, m10, m11, m20, m21, m22].
// S = P + R on the lower triangle: P row-major 3 x 3 (the node call's block), R a lower triangle
BOS_HD void match_pose_S(const double* P, const double R[6], double S[6]) {
    S[0] = P[0] + R[0];
    S[1] = P[3] + R[1];
    S[2] = P[4] + R[2];
    S[3] = P[6] + R[3];
    S[4] = P[7] + R[4];
    S[5] = P[8] + R[5];
}

BOS_HD double match_pose_nis(const double e[3], const double S[6]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s00 = S[0], s10 = S[1], s11 = S[2], s20 = S[3], s21 = S[4], s22 = S[5];
    const double D0 = s00;
    if (!match_pivot_ok(D0)) return match_nan();
    const double l10 = s10 / D0;
    const double l20 = s20 / D0;
    const double D1 = s11 - l10 * s10;
    if (!match_pivot_ok(D1)) return match_nan();
    const double t21 = s21 - l20 * s10;
    const double l21 = t21 / D1;
    const double D2 = (s22 - l20 * s20) - l21 * t21;
    if (!match_pivot_ok(D2)) return match_nan();
    const double y0 = e[0];
    const double y1 = e[1] - l10 * y0;
    const double y2 = (e[2] - l20 * y0) - l21 * y1;
    return ((y0 * y0) / D0 + (y1 * y1) / D1) + (y2 * y2) / D2;
}

// the lower triangle to the row-major 3 x 3, mirrored
BOS_HD void match_mirror(const double S[6], double out[9]) {
    out[0] = S[0];
    out[3] = S[1]; out[1] = S[1];
    out[4] = S[2];
    out[6] = S[3]; out[2] = S[3];
    out[7] = S[4]; out[5] = S[4];
    out[8] = S[5];
}

// R = Omega^-1 (bos_match_information_inverse) through the LDL^T of Omega, Omega = L D L^T and
// R = L^-T D^-1 L^-1: the lower triangle evaluated, R[9] row-major and mirrored. False, R untouched, when
// Omega is not finite, not bit-symmetric, or a pivot is not positive.
inline bool match_information_inverse(const double om[9], double R[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(om[i])) return false;
    if (om[1] != om[3] || om[2] != om[6] || om[5] != om[7]) return false;
    const double D0 = om[0];
    if (!match_pivot_ok(D0)) return false;
    const double l10 = om[3] / D0;
    const double l20 = om[6] / D0;
    const double D1 = om[4] - l10 * om[3];
    if (!match_pivot_ok(D1)) return false;
    const double t21 = om[7] - l20 * om[3];
    const double l21 = t21 / D1;
    const double D2 = (om[8] - l20 * om[6]) - l21 * t21;
    if (!match_pivot_ok(D2)) return false;
    // L^-1 = [[1, 0, 0], [a, 1, 0], [b, c, 1]]
    const double a = 0.0 - l10;
    const double c = 0.0 - l21;
    const double b = l10 * l21 - l20;
    const double lower[6] = {(1.0 / D0 + (a * a) / D1) + (b * b) / D2,
                             a / D1 + (c * b) / D2,
                             1.0 / D1 + (c * c) / D2,
                             b / D2,
                             c / D2,
                             1.0 / D2};
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(lower[i])) return false;
    match_mirror(lower, R);
    return true;
}

// ---- argument rules ------------------------------------------------------------------------------------
inline const char* match_bad_gate_k(double gate, int32_t k) {
    if (!(gate > 0.0)) return "the gate is NaN or not positive";
    if (k < 1 || k > kMatchMaxK) return "k outside 1 .. BOS_MATCH_MAX_K";
    return nullptr;
}

// null, or what is wrong with the arguments of a landmark match
inline const char* match_landmarks_bad_argument(int NL, int32_t n, const int32_t* landmark, double gate, int32_t k) {
    if (n < 0 || (n > 0 && !landmark)) return "bad argument";
    if (const char* bad = match_bad_gate_k(gate, k)) return bad;
    for (int32_t q = 0; q < n; ++q)
        if (landmark[q] < 0 || landmark[q] >= NL) return "a landmark outside [0, NL)";
    return nullptr;
}

// null, or what is wrong with the arguments of a pose match (omega may be null: the identity); R, when not
// null, receives the n inverses ([n][9])
inline const char* match_poses_bad_argument(int NP, int32_t n, const int32_t* pose, const double* z, const double* omega, double gate,
                                            int32_t k, double* R) {
    if (n < 0 || (n > 0 && (!pose || !z))) return "bad argument";
    if (const char* bad = match_bad_gate_k(gate, k)) return bad;
    const double identity[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int32_t q = 0; q < n; ++q) {
        if (pose[q] < 0 || pose[q] >= NP) return "a pose outside [0, NP)";
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(z[3 * q + i])) return "a measurement that is not finite";
        double Rq[9];
        if (!match_information_inverse(omega ? omega + 9 * (int64_t)q : identity, Rq))
            return "an information matrix that is not finite, symmetric and positive definite";
        for (int i = 0; i < 9 && R; ++i) R[9 * (int64_t)q + i] = Rq[i];
    }
    return nullptr;
}

}  // namespace bos
