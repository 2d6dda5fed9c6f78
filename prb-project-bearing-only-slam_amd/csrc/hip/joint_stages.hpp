// The first two stages that joint_nis_kernel (hip/joint.hip) and jcbb_kernel (hip/jcbb.hip) share: one
// wavefront (one workgroup of 64) evaluates e and J of a hypothesis's m <= 32 pairings at the master state and
// assembles S in LDS through the hypothesis's table (host/joint.hpp joint_S_entry).
#pragma once

#include <hip/hip_runtime.h>

#include "../host/joint.hpp"

namespace bos {
namespace dev {

// Args: a kernel's argument struct with the batch's pairings (pose, landmark, z, omega), the master state
// (state_pose, state_lm), the pair call's blocks (diag, cross), the tables (tab, tab_off), s_off and the outputs
// innovation and cov (either may be null). Hypothesis h has the pairings p0 .. p0 + m - 1.
// 1. lane i < m evaluates e_i and J_i (J_i and omega_i go to LDS, e_i to innovation when asked for) and returns
//    e_i (0 in the other lanes); 2. the lanes stride over the m (m + 1) / 2 lower entries of S and write each to
//    LDS at (i, j) and (j, i), rows padded to kJointLd doubles, and to h's block of cov when asked for. The
//    caller synchronises before it reads S.
template <class Args> __device__ __forceinline__ double joint_assemble(const Args& a, int h, int lane, int p0, int m, double* S, double* Jl,
                                                                        double* om) {
    double y = 0.0;
    if (lane < m) {
        double J[5];
        y = joint_innovation(a.state_pose, a.state_lm, a.pose[p0 + lane], a.landmark[p0 + lane], a.z[p0 + lane], J);
#pragma unroll
        for (int c = 0; c < 5; ++c) Jl[5 * lane + c] = J[c];
        om[lane] = a.omega[p0 + lane];
        if (a.innovation) a.innovation[p0 + lane] = y;
    }
    __syncthreads();
    JointEntryIn in;
    in.pose = a.state_pose; in.lm = a.state_lm; in.diag = a.diag; in.cross = a.cross;
    in.tab = a.tab + 4 * a.tab_off[h];
    in.J = Jl; in.omega = om;
    double* cov = a.cov ? a.cov + a.s_off[h] : nullptr;
    const int entries = m * (m + 1) / 2;
    for (int idx = lane; idx < entries; idx += 64) {
        int i = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
        while (i * (i + 1) / 2 > idx) --i;
        while ((i + 1) * (i + 2) / 2 <= idx) ++i;
        const int j = idx - i * (i + 1) / 2;
        const double v = joint_S_entry(in, i, j);
        S[i * kJointLd + j] = v;
        S[j * kJointLd + i] = v;
        if (cov) {
            cov[i * m + j] = v;
            cov[j * m + i] = v;
        }
    }
    return y;
}

}  // namespace dev
}  // namespace bos
