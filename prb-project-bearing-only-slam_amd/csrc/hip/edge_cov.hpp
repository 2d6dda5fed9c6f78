// Edge covariances, projection step (hip/edge_cov.hip): one thread per edge forms the edge's cross
// block and J Sigma_joint J^T from the marginals' blocks and the pair buffer the selected inverse
// emitted (hip/selinv.hip). The arithmetic is host/edge_cov.hpp, shared with the host twin.
#pragma once

#include <hip/hip_runtime.h>

#include "../host/edge_cov.hpp"

namespace bos {
namespace dev {

constexpr int kEdgeBlock = 256;
// Enqueues the kernel over in.Mb + in.Mo edges (bearings first, then odometry); every pointer of `in`
// is device memory, null outputs are not computed. Nothing is launched for an empty problem.
hipError_t launch_edge_project(const EdgeCovIn& in, const EdgeCovOut& out, hipStream_t s);

}  // namespace dev
}  // namespace bos
