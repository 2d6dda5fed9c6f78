// Selected inverse of the multifrontal factor (hip/selinv.hip): the marginal covariance block of
// every node from the finished L panels, one top-down pass over the assembly tree.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace bos {
struct Plan;
namespace dev {

struct MfDevice;
struct SelInv;   // launch plan, Sigma-front buffer and output buffer; owned by the MfDevice

// Enqueues the pass on s after the mf_factor (program 0) whose L panels it reads: one launch per tree
// level and front class, top-down, then one for the folded landmarks; plain stream order. out_dev
// receives the device buffer of the blocks, [9 NP pose blocks | 4 NL landmark blocks] doubles,
// row-major, stix order (the fixed pose's block zero), valid once s has drained. The launch plan and
// the buffers are built at the first call (P is the handle's plan) and freed by mf_destroy.
// Returns 0; -1 with err when the plan cannot be used; -2 with err (the byte count) when a device
// allocation fails: nothing is kept then, and the handle's factorization is untouched.
// With emit_cross (after mf_edge_cov_build) every front also writes the cross blocks of its edge pairs
// into the pair buffer (plan.hpp CrossRecords); without it the launches are the marginals' own.
int mf_selected_inverse(MfDevice* d, const Plan& P, const double** out_dev, hipStream_t s, std::string& err,
                        bool emit_cross = false);

// Edge covariances (bos_edge_covariances). The problem's edges, host arrays in measurement order:
struct EdgeList {
    int Mb = 0, Mo = 0;
    const int32_t *b_pose = nullptr, *b_lm = nullptr, *o_src = nullptr, *o_dst = nullptr;
};
// The per-edge results on the device (null where not asked for): [6 Mb], [9 Mo], [Mb], [9 Mo]
struct EdgeCovResult {
    const double *bearing_cross = nullptr, *odom_cross = nullptr, *bearing_var = nullptr, *odom_cov = nullptr;
};
bool mf_edge_cov_built(const MfDevice* d);
// Builds, once, the selected inverse's own state (as mf_selected_inverse does) and the feature's: the
// cross records, the per-edge index arrays, the pair buffer and the per-edge outputs in one allocation,
// owned and freed with the SelInv. Returns as mf_selected_inverse; after -2 the selected inverse itself
// stays usable.
int mf_edge_cov_build(MfDevice* d, const Plan& P, const EdgeList& E, std::string& err);
// Enqueues the projection kernel (hip/edge_cov.hip) on s, after an mf_selected_inverse(emit_cross) on
// the same stream: pose / lm the fp64 master state; want[4] selects bearing_cross, odom_cross,
// bearing_var, odom_cov.
int mf_edge_project(MfDevice* d, const double* pose, const double* lm, const bool want[4], EdgeCovResult* res, hipStream_t s,
                    std::string& err);
// bytes of the feature's allocation (0 before mf_edge_cov_build)
int64_t mf_edge_cov_bytes(const MfDevice* d);
// bytes of the Sigma-front buffer (0 before the first call)
int64_t mf_selinv_sigma_bytes(const MfDevice* d);
// Diagnostics (bos_debug_selinv_fronts, whose layout this fills): fronts [BOS_SELINV_COLS nsuper],
// node_front [NP + NL] and edge_front [Mb + Mo] (either may be null), from what selinv_build noted and
// the host's copies of the records. -1 before the state is built; nothing is launched.
int mf_selinv_report(const MfDevice* d, const Plan& P, int32_t* fronts, int32_t* node_front, int32_t* edge_front);
void selinv_destroy(SelInv* p);

}  // namespace dev
}  // namespace bos
