// Edge covariances: the per-edge arithmetic shared by edge_project_kernel (hip/edge_cov.hip) and the
// host twin (bos_plan_mf_edge_covariances). Header-only, __host__ __device__.
//
// An edge with nodes (a, b) has Sigma_joint = [[S_aa, S_ab], [S_ab^T, S_bb]]: the diagonal blocks come
// from the marginals' output, S_ab from the pair buffer the selected inverse emitted (plan.hpp
// CrossRecords), zero when the edge involves the fixed pose (whose diagonal block is zero too). The
// projected covariance is J Sigma_joint J^T with J the error Jacobian of bos_math.hpp at the fp64
// master state, cos / sin evaluated in fp64; neither Jacobian depends on the measurement z, which is
// passed as zero.
#pragma once

#include <cstdint>

#include "bos_math.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define BOS_UNROLL _Pragma("unroll")
#else
#define BOS_UNROLL
#endif

namespace bos {

struct EdgeCovIn {
    int Mb = 0, Mo = 0;
    const double *pose = nullptr, *lm = nullptr;           // master state: [3 NP], [2 NL]
    const double *pose_cov = nullptr, *lm_cov = nullptr;   // [9 NP], [4 NL] row-major (marginals)
    const double* pairs = nullptr;                         // [9 n_pairs]
    const int32_t *b_pose = nullptr, *b_lm = nullptr, *o_src = nullptr, *o_dst = nullptr;
    const int32_t *edge_slot = nullptr, *edge_tr = nullptr;   // [Mb + Mo]
};
struct EdgeCovOut {   // any may be null
    double *bearing_cross = nullptr, *odom_cross = nullptr, *bearing_var = nullptr, *odom_cov = nullptr;
};

// J S J^T of a bearing, J = [J_p (3) | J_l (2)]: one sum in a fixed order, the pose block, twice the
// cross block, the landmark block. Zero pose and cross blocks (the fixed pose) leave J_l S_ll J_l^T.
BOS_HD double edge_bearing_var(const double Spp[9], const double Sll[4], const double C[6], const double J[5]) {
    double acc = 0.0;
BOS_UNROLL
    for (int i = 0; i < 3; ++i)
BOS_UNROLL
        for (int j = 0; j < 3; ++j) acc += J[i] * Spp[3 * i + j] * J[j];
BOS_UNROLL
    for (int i = 0; i < 3; ++i)
BOS_UNROLL
        for (int j = 0; j < 2; ++j) acc += 2.0 * (J[i] * C[2 * i + j] * J[3 + j]);
BOS_UNROLL
    for (int i = 0; i < 2; ++i)
BOS_UNROLL
        for (int j = 0; j < 2; ++j) acc += J[3 + i] * Sll[2 * i + j] * J[3 + j];
    return acc;
}

// J S J^T of an odometry edge, J 3 x 6 row-major over [src | dst], C = Sigma(src, dst): T = S J^T, then
// the lower triangle of J T, mirrored
BOS_HD void edge_odom_cov(const double Saa[9], const double Sbb[9], const double C[9], const double J[18], double out[9]) {
    double T[18];
BOS_UNROLL
    for (int i = 0; i < 6; ++i)
BOS_UNROLL
        for (int v = 0; v < 3; ++v) {
            double acc = 0.0;
BOS_UNROLL
            for (int j = 0; j < 6; ++j) {
                const double sij = i < 3 ? (j < 3 ? Saa[3 * i + j] : C[3 * i + (j - 3)])
                                         : (j < 3 ? C[3 * j + (i - 3)] : Sbb[3 * (i - 3) + (j - 3)]);
                acc += sij * J[6 * v + j];
            }
            T[3 * i + v] = acc;
        }
BOS_UNROLL
    for (int u = 0; u < 3; ++u)
BOS_UNROLL
        for (int v = 0; v <= u; ++v) {
            double acc = 0.0;
BOS_UNROLL
            for (int i = 0; i < 6; ++i) acc += J[6 * u + i] * T[3 * i + v];
            out[3 * u + v] = acc;
            out[3 * v + u] = acc;
        }
}

// Covariance of l_a - l_b for two landmarks, J = [I, -I], C = Sigma(a, b): S_aa + S_bb - C - C^T, the
// lower triangle, mirrored
BOS_HD void edge_landmark_diff_cov(const double Saa[4], const double Sbb[4], const double C[4], double out[4]) {
BOS_UNROLL
    for (int u = 0; u < 2; ++u)
BOS_UNROLL
        for (int v = 0; v <= u; ++v) {
            const double acc = Saa[2 * u + v] + Sbb[2 * u + v] - C[2 * u + v] - C[2 * v + u];
            out[2 * u + v] = acc;
            out[2 * v + u] = acc;
        }
}

// bearing e: its cross block Sigma(pose, landmark) (3 x 2) and its variance
BOS_HD void edge_cov_bearing(const EdgeCovIn& in, const EdgeCovOut& o, int64_t e) {
    const int64_t p = in.b_pose[e], l = in.b_lm[e], slot = in.edge_slot[e];
    double C[6];
BOS_UNROLL
    for (int i = 0; i < 6; ++i) C[i] = slot >= 0 ? in.pairs[9 * slot + i] : 0.0;
    if (o.bearing_cross) {
BOS_UNROLL
        for (int i = 0; i < 6; ++i) o.bearing_cross[6 * e + i] = C[i];
    }
    if (!o.bearing_var) return;
    double Spp[9], Sll[4], J[5];
BOS_UNROLL
    for (int i = 0; i < 9; ++i) Spp[i] = in.pose_cov[9 * p + i];
BOS_UNROLL
    for (int i = 0; i < 4; ++i) Sll[i] = in.lm_cov[4 * l + i];
    const double th = in.pose[3 * p + 2];
    (void)bearing_error_jacobian<double>(in.pose[3 * p], in.pose[3 * p + 1], cos(th), sin(th), in.lm[2 * l], in.lm[2 * l + 1], 0.0, J);
    o.bearing_var[e] = edge_bearing_var(Spp, Sll, C, J);
}

// odometry edge e (index among the odometry edges): Sigma(src, dst) (3 x 3) and J Sigma_joint J^T
BOS_HD void edge_cov_odometry(const EdgeCovIn& in, const EdgeCovOut& o, int64_t e) {
    const int64_t a = in.o_src[e], b = in.o_dst[e], slot = in.edge_slot[in.Mb + e];
    const bool tr = in.edge_tr[in.Mb + e] != 0;
    double C[9];
BOS_UNROLL
    for (int i = 0; i < 3; ++i)
BOS_UNROLL
        for (int j = 0; j < 3; ++j) C[3 * i + j] = slot >= 0 ? in.pairs[9 * slot + (tr ? 3 * j + i : 3 * i + j)] : 0.0;
    if (o.odom_cross) {
BOS_UNROLL
        for (int i = 0; i < 9; ++i) o.odom_cross[9 * e + i] = C[i];
    }
    if (!o.odom_cov) return;
    double Saa[9], Sbb[9], J[18], err[3], out[9];
BOS_UNROLL
    for (int i = 0; i < 9; ++i) {
        Saa[i] = in.pose_cov[9 * a + i];
        Sbb[i] = in.pose_cov[9 * b + i];
    }
    const double ths = in.pose[3 * a + 2];
    odometry_error_jacobian<double>(in.pose[3 * a], in.pose[3 * a + 1], ths, cos(ths), sin(ths), in.pose[3 * b], in.pose[3 * b + 1],
                                    in.pose[3 * b + 2], 0.0, 0.0, 0.0, err, J);
    edge_odom_cov(Saa, Sbb, C, J, out);
BOS_UNROLL
    for (int i = 0; i < 9; ++i) o.odom_cov[9 * e + i] = out[i];
}

}  // namespace bos
