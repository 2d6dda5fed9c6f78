// Bearing association (bos_associate_bearings): a new bearing z taken from pose a is gated against every
// landmark l by its normalised innovation squared
//   e = bearing_error(a, l, z),  S = var(a, l) + 1 / omega,  nis = (e * e) / S,
// var(a, l) the variance of the predicted bearing of l from a (bos_node_covariances' projected_landmark
// entry 0), and the landmarks with nis <= gate are listed, the k smallest ascending by (nis, landmark stix).
//
// This header holds what the device kernels (hip/associate.hip) and the host twin
// (bos_plan_mf_associate_bearings) share: the argument rules, the three expressions, evaluated with plain
// IEEE operations in the order written (no FP contraction, so a caller reproduces nis from e and S), the
// order of the candidates, and the register-resident list of the k best the device's selection keeps.
#pragma once

#include <cmath>
#include <cstdint>

#include "edge_cov.hpp"

namespace bos {

constexpr int kAssocMaxK = 8;                // BOS_ASSOC_MAX_K
constexpr int kAssocTile = 1024;             // landmarks per workgroup of the selection's first stage
constexpr int32_t kAssocNone = INT32_MAX;    // the stix of an empty list slot: sorts after every landmark

// the query pose's frame: translation and the fp64 cos / sin of its angle
struct AssocFrame { double px, py, c, s; };

BOS_HD AssocFrame assoc_frame(const double* pose, int a) {
    const double th = pose[3 * a + 2];
    AssocFrame f;
    f.px = pose[3 * a]; f.py = pose[3 * a + 1]; f.c = cos(th); f.s = sin(th);
    return f;
}

BOS_HD double assoc_innovation(const AssocFrame& f, double lx, double ly, double z) {
    double gx, gy;
    return bearing_error<double>(f.px, f.py, f.c, f.s, lx, ly, z, gx, gy);
}

BOS_HD double assoc_innovation_var(double var, double omega) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return var + 1.0 / omega;
}

BOS_HD double assoc_nis(double e, double S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (e * e) / S;
}

// listed and counted: finite and inside the gate (a NaN compares false)
BOS_HD bool assoc_inside(double nis, double gate) { return std::fabs(nis) <= 1.7976931348623157e308 && nis <= gate; }

// the candidates' order: ascending NIS, equal NIS to the lower stix first
BOS_HD bool assoc_less(double nis_a, int32_t l_a, double nis_b, int32_t l_b) {
    return nis_a < nis_b || (nis_a == nis_b && l_a < l_b);
}

// The kAssocMaxK best of what was inserted, ascending; an empty slot is (+inf, kAssocNone). Every index is
// a compile-time constant once unrolled, so the list stays in registers (8 doubles + 8 ints: 24 VGPRs).
struct AssocTop {
    double nis[kAssocMaxK];
    int32_t l[kAssocMaxK];
};

BOS_HD void assoc_top_clear(AssocTop& t) {
BOS_UNROLL
    for (int i = 0; i < kAssocMaxK; ++i) {
        t.nis[i] = HUGE_VAL;
        t.l[i] = kAssocNone;
    }
}

BOS_HD void assoc_top_insert(AssocTop& t, double nis, int32_t l) {
BOS_UNROLL
    for (int i = 0; i < kAssocMaxK; ++i) {
        const bool before = assoc_less(nis, l, t.nis[i], t.l[i]);
        const double tn = t.nis[i];
        const int32_t tl = t.l[i];
        t.nis[i] = before ? nis : tn;
        t.l[i] = before ? l : tl;
        nis = before ? tn : nis;
        l = before ? tl : l;
    }
}

// null, or what is wrong with the arguments of an association call (omega may be null: 1 for every bearing)
inline const char* assoc_bad_argument(int NP, int32_t n, const int32_t* pose, const double* z, const double* omega, double gate,
                                      int32_t k) {
    if (n < 0 || (n > 0 && (!pose || !z))) return "bad argument";
    if (!(gate > 0.0)) return "the gate is NaN or not positive";
    if (k < 1 || k > kAssocMaxK) return "k outside 1 .. BOS_ASSOC_MAX_K";
    for (int32_t q = 0; q < n; ++q) {
        if (pose[q] < 0 || pose[q] >= NP) return "a pose outside [0, NP)";
        if (!std::isfinite(z[q])) return "a bearing that is not finite";
        if (omega && !(std::isfinite(omega[q]) && omega[q] > 0.0)) return "an information that is not finite and positive";
    }
    return nullptr;
}

}  // namespace bos
