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
int mf_selected_inverse(MfDevice* d, const Plan& P, const double** out_dev, hipStream_t s, std::string& err);
// bytes of the Sigma-front buffer (0 before the first call)
int64_t mf_selinv_sigma_bytes(const MfDevice* d);
void selinv_destroy(SelInv* p);

}  // namespace dev
}  // namespace bos
