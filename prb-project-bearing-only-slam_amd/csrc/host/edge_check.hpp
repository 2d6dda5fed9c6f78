// Edge consistency (bos_edge_consistency): the measurements that are in the graph, tested against the
// estimate they produced (Baarda's data snooping). H is sum J^T Omega J + lambda I, the robust kernel scales
// the right-hand side only, so the residual e of an edge at the optimum has the covariance
//   T = R - P,   R = Omega^-1,   P = J Sigma_joint J^T (bos_edge_covariances' bearing_var / odom_cov),
// positive semi-definite in exact arithmetic for every lambda >= 0, and
//   w2 = e^T T^-1 e          the normalised residual: chi^2 with 1 (bearing) or 3 (odometry) degrees of freedom
//   r  = 1 - tr(Omega P) / d  the redundancy number, sum over the edges of tr(Omega P) = n - lambda tr(Sigma)
//   chi2 = e^T Omega e        what the edge adds to the objective
//
// This header holds what the device kernel (hip/edge_check.hip) and the host twin
// (bos_plan_mf_edge_consistency) share: the argument rule, R, and the two per-edge evaluations. Every
// expression is evaluated with plain IEEE + - * / in the order written (no FP contraction), so a caller
// reproduces w2 from the listed e and T. The odometry's w2 is match.hpp's 3 x 3 LDL^T (match_pose_nis).
#pragma once

#include <cmath>
#include <cstdint>

#include "match.hpp"

namespace bos {

constexpr int kEdgeCheckMaxK = kAssocMaxK;   // BOS_EDGE_CHECK_MAX_K

// what an edge's evaluation gives: T and e as the lists return them (T's lower triangle mirrored)
struct EdgeCheckBearing { double e, T, w2, chi2, redundancy; };
struct EdgeCheckOdom { double e[3], T[9], w2, chi2, redundancy; };

// bearing: e the innovation at the state, omega its information, var = bearing_var of the edge
BOS_HD EdgeCheckBearing edge_check_bearing(double e, double omega, double var) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    EdgeCheckBearing o;
    o.e = e;
    o.chi2 = (e * omega) * e;
    const double R = 1.0 / omega;
    o.T = R - var;
    o.w2 = match_pivot_ok(o.T) ? (e * e) / o.T : match_nan();
    o.redundancy = 1.0 - omega * var;
    return o;
}

// odometry: u Omega's upper triangle (00, 01, 02, 11, 12, 22), R the lower triangle of Omega^-1
// (edge_check_information_inverse), P = odom_cov of the edge (row-major 3 x 3, its lower triangle is read for
// T, all nine entries for the trace); a self-loop's w2 and redundancy are NaN
BOS_HD void edge_check_odometry(const double e[3], const double u[6], const double R[6], const double* P, bool self_loop,
                                EdgeCheckOdom& o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    o.e[0] = e[0]; o.e[1] = e[1]; o.e[2] = e[2];
    const double Oe0 = (u[0] * e[0] + u[1] * e[1]) + u[2] * e[2];
    const double Oe1 = (u[1] * e[0] + u[3] * e[1]) + u[4] * e[2];
    const double Oe2 = (u[2] * e[0] + u[4] * e[1]) + u[5] * e[2];
    o.chi2 = (e[0] * Oe0 + e[1] * Oe1) + e[2] * Oe2;
    const double T[6] = {R[0] - P[0], R[1] - P[3], R[2] - P[4], R[3] - P[6], R[4] - P[7], R[5] - P[8]};
    match_mirror(T, o.T);
    // sum over a, b of Omega_ab P_ab, row-major
    double tr = 0.0;
    tr += u[0] * P[0]; tr += u[1] * P[1]; tr += u[2] * P[2];
    tr += u[1] * P[3]; tr += u[3] * P[4]; tr += u[4] * P[5];
    tr += u[2] * P[6]; tr += u[4] * P[7]; tr += u[5] * P[8];
    o.w2 = self_loop ? match_nan() : match_pose_nis(e, T);
    o.redundancy = self_loop ? match_nan() : 1.0 - tr / 3.0;
}

// The lower triangle of R = Omega^-1 for Omega given by its upper triangle u, mirrored: match.hpp's
// match_information_inverse (the code behind bos_match_information_inverse); six NaNs where it refuses Omega
// (not finite, or a pivot of its LDL^T not positive)
inline void edge_check_information_inverse(const double u[6], double R[6]) {
    const double om[9] = {u[0], u[1], u[2], u[1], u[3], u[4], u[2], u[4], u[5]};
    double full[9];
    if (match_information_inverse(om, full)) {
        R[0] = full[0]; R[1] = full[3]; R[2] = full[4]; R[3] = full[6]; R[4] = full[7]; R[5] = full[8];
    } else {
        for (int i = 0; i < 6; ++i) R[i] = match_nan();
    }
}

// null, or what is wrong with the gates and k
inline const char* edge_check_bad_argument(double gate_bearing, double gate_odom, int32_t k) {
    if (!(std::isfinite(gate_bearing) && gate_bearing >= 0.0 && std::isfinite(gate_odom) && gate_odom >= 0.0))
        return "a gate that is NaN, negative or infinite";
    if (k < 1 || k > kEdgeCheckMaxK) return "k outside 1 .. BOS_EDGE_CHECK_MAX_K";
    return nullptr;
}

}  // namespace bos
