// Device side of bos_set_priors (hip/prior.hip): one launch behind the J+H build that adds every prior's
// J^T Omega J to its node's diagonal block of H and J^T Omega e to its segment of b (host/prior.hpp),
// and leaves one chi^2 partial per workgroup for the step's statistics reduction. A plain grid launch:
// at most one prior per node and kind, so no two threads touch one address; no atomics, no waits.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace bos {
namespace dev {

constexpr int kPriorBlock = 256;
// Records in T, padded so that a thread loads its own in whole vectors: a pose prior is
// [m0, m1, m2, u00 | u01, u02, u11, u12 | u22, 0, 0, 0], a landmark prior [m0, m1 | u00, u01 | u11, 0]
constexpr int kPriorPoseRec = 12;
constexpr int kPriorLmRec = 6;

template <typename T> struct PriorParams {
    int n_pose, n_lm;         // threads [0, n_pose) run the pose priors, [n_pose, n_pose + n_lm) the landmark priors
    const int32_t* idx;       // [n_pose + n_lm] the node of each prior (pose index, then landmark index)
    const T* pose_rec;        // [n_pose][kPriorPoseRec]
    const T* lm_rec;          // [n_lm][kPriorLmRec]
    // what the J+H build reads (LinParams)
    const T* pc;              // [NP][4] x, y, cos, sin
    const T* pth;             // [NP] theta
    const T* lc;              // [NL][2]
    int NP, NL;
    T* hval;                  // block array: pose p's diagonal block at 6 p, landmark l's at off_ldiag + 3 l
    T* b;                     // [3 NP + 2 NL]
    int64_t off_ldiag, nval;
    double* part;             // [prior_parts(n_pose + n_lm)] sum of rho of each workgroup's priors
};

inline int prior_parts(int64_t n) { return (int)((n + kPriorBlock - 1) / kPriorBlock); }
template <typename T> hipError_t launch_priors(const PriorParams<T>& p, hipStream_t s);

}  // namespace dev
}  // namespace bos
