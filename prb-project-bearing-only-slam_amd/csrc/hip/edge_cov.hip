// Edge covariances, projection step: see edge_cov.hpp. The kernel keeps an edge's blocks, Jacobian and
// products in registers (every loop of host/edge_cov.hpp is unrolled over constant bounds: no scratch
// arrays in memory) and indexes with 64-bit arithmetic.
#include "edge_cov.hpp"

namespace bos {
namespace dev {

namespace {

__global__ __launch_bounds__(kEdgeBlock) void edge_project_kernel(const EdgeCovIn in, const EdgeCovOut out) {
    const int64_t e = (int64_t)blockIdx.x * kEdgeBlock + threadIdx.x;
    if (e < in.Mb) edge_cov_bearing(in, out, e);
    else if (e < (int64_t)in.Mb + in.Mo) edge_cov_odometry(in, out, e - in.Mb);
}

}  // namespace

hipError_t launch_edge_project(const EdgeCovIn& in, const EdgeCovOut& out, hipStream_t s) {
    const int64_t edges = (int64_t)in.Mb + in.Mo;
    if (edges <= 0) return hipSuccess;
    edge_project_kernel<<<(unsigned)((edges + kEdgeBlock - 1) / kEdgeBlock), kEdgeBlock, 0, s>>>(in, out);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace bos
