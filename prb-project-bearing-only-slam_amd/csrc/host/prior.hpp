// Unary prior factors (bos.h bos_set_priors): the terms a pose prior and a landmark prior add to the
// diagonal block of H, to b and to chi^2. Shared by the device kernel (hip/prior.hip, in the build's
// T), the cost pass (hip/lm.hip, fp64), the CPU twin (cpu_baseline.cpp) and bos_prior_terms, which
// exports them so that a test can pin the operation order written out here bit for bit. Every line is
// one IEEE operation at a time, no FP contraction.
#pragma once

#include "bos_math.hpp"

namespace bos {

// Pose prior. Pose (x, y, th), mean m[3], u the upper triangle of Omega (00, 01, 02, 11, 12, 22). The
// perturbation is left-multiplicative (boxplus_pose: X' = v2t(dx) X), so the error's Jacobian is
// J = [[1, 0, -y], [0, 1, x], [0, 0, 1]]. A = J^T Omega J in the block array's order
// (00, 10, 11, 20, 21, 22), g = J^T Omega e; returns rho = e^T Omega e.
template <typename T> BOS_HD T prior_pose_terms(T x, T y, T th, const T m[3], const T u[6], T A[6], T g[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const T e0 = x - m[0], e1 = y - m[1];
    const T e2 = normalized_angle<T>(th - m[2]);
    const T Oe0 = (u[0] * e0 + u[1] * e1) + u[2] * e2;
    const T Oe1 = (u[1] * e0 + u[3] * e1) + u[4] * e2;
    const T Oe2 = (u[2] * e0 + u[4] * e1) + u[5] * e2;
    const T rho = (e0 * Oe0 + e1 * Oe1) + e2 * Oe2;
    const T ny = -y;
    g[0] = Oe0;
    g[1] = Oe1;
    g[2] = (ny * Oe0 + x * Oe1) + Oe2;
    const T q0 = (ny * u[0] + x * u[1]) + u[2];
    const T q1 = (ny * u[1] + x * u[3]) + u[4];
    const T q2 = (ny * u[2] + x * u[4]) + u[5];
    A[0] = u[0];
    A[1] = u[1];
    A[2] = u[3];
    A[3] = q0;
    A[4] = q1;
    A[5] = (ny * q0 + x * q1) + q2;
    return rho;
}

// rho of a pose prior alone (the cost pass)
template <typename T> BOS_HD T prior_pose_rho(T x, T y, T th, const T m[3], const T u[6]) {
    T A[6], g[3];
    return prior_pose_terms<T>(x, y, th, m, u, A, g);
}

// Landmark prior. Landmark (lx, ly), mean m[2], u = (00, 01, 11), J = I. A = Omega in the order
// (00, 10, 11), g = Omega e; returns rho.
template <typename T> BOS_HD T prior_landmark_terms(T lx, T ly, const T m[2], const T u[3], T A[3], T g[2]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const T e0 = lx - m[0], e1 = ly - m[1];
    g[0] = u[0] * e0 + u[1] * e1;
    g[1] = u[1] * e0 + u[2] * e1;
    A[0] = u[0];
    A[1] = u[1];
    A[2] = u[2];
    return e0 * g[0] + e1 * g[1];
}

template <typename T> BOS_HD T prior_landmark_rho(T lx, T ly, const T m[2], const T u[3]) {
    T A[3], g[2];
    return prior_landmark_terms<T>(lx, ly, m, u, A, g);
}

}  // namespace bos
