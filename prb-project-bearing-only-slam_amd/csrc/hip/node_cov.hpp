// Node covariances on the device (hip/node_cov.hip): see host/node_cov.hpp for the identity. Per query
// node, in plain stream order after the mf_factor whose L panels they read: the pair feature's path solve
// for the one node, the scatter of its rows into X, the backward sweep (one launch per tree level and
// front class, root first, then the folded landmarks) and the gather + projection (one thread per target
// node). No kernel communicates between workgroups.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../host/node_cov.hpp"
#include "multifrontal.hpp"
#include "pair_cov.hpp"

namespace bos {
namespace dev {

struct NodeCov;   // the feature's device arena; owned by the solver handle

// device results of the last enqueued query, one node's blocks (null where not asked for)
struct NodeCovDev {
    const double *cross_pose = nullptr, *cross_landmark = nullptr, *projected_pose = nullptr, *projected_landmark = nullptr;
};

NodeCov* node_cov_create();
void node_cov_destroy(NodeCov* p);
int64_t node_cov_bytes(const NodeCov* p);
bool node_cov_built(const NodeCov* p);
// Builds, once, the arena: the index arrays of np / pp / P, X, the path solve's slice and one node's
// output blocks. 0; -2 with err (the byte count) when the allocation fails: nothing is kept then.
int node_cov_build(NodeCov* p, const Plan& P, const PairPaths& pp, const NodeCovPlan& np, std::string& err);
// Enqueues one query on s: node a through path solve, scatter and sweep (none of them with fixed: a is the
// fixed pose, whose column is zero), after_solve recorded behind them, then the gather + projection of the
// outputs in want[4] (cross_pose, cross_landmark, projected_pose, projected_landmark). sig: the selected
// inverse's blocks (null when no projection is asked for); pose / lm: the fp64 master state.
int node_cov_enqueue(NodeCov* p, const MfView& v, int a, bool fixed, const bool want[4], const double* sig, const double* pose, const double* lm,
                     hipStream_t s, hipEvent_t after_solve, NodeCovDev* out, std::string& err);

}  // namespace dev
}  // namespace bos
