// Pair covariances on the device (hip/pair_cov.hip): see host/pair_cov.hpp for the identity. Three
// kernels per batch, plain stream order after the mf_factor whose L panels they read: the path solve
// (one wavefront per distinct node), the product (one wavefront per block) and the projection (one
// thread per query, host/pair_cov.hpp pair_cov_query). No kernel communicates between waves.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../host/pair_cov.hpp"
#include "multifrontal.hpp"

namespace bos {
namespace dev {

struct PairCov;   // the feature's device arena; owned by the solver handle

// One batch as the host prepared it (host arrays). Distinct node i: its start supernode, its first dof
// inside it, its dofs (3 / 2), its path's dofs and its Y slice y_off[i] (doubles; the slice holds len * d).
// Query q: the two node ids, their distinct-node slots (-1: the fixed pose), the rows of the two slices
// where the common tail starts and its length (0: the fixed pose, or two roots).
struct PairCovBatch {
    int32_t n_nodes = 0;
    int64_t n_queries = 0, y_count = 0;
    const int64_t* y_off = nullptr;
    const int32_t *n_sn = nullptr, *n_loc = nullptr, *n_d = nullptr, *n_len = nullptr;
    const int32_t *q_a = nullptr, *q_b = nullptr, *q_slot_a = nullptr, *q_slot_b = nullptr, *q_off_a = nullptr, *q_off_b = nullptr,
                  *q_c = nullptr;
};
// device results of the last enqueued batch, [9 n_queries] each (null where not asked for)
struct PairCovOut {
    const double *cross = nullptr, *projected = nullptr, *cov_a = nullptr, *cov_b = nullptr;
};

constexpr int64_t kPairYBudgetBytes = 64ll << 20;   // Y slices of one batch (bos_pair_covariances batches past it)
constexpr int64_t kPairMaxQueries = 1 << 17;        // queries of one batch
// rows of the largest front the path solve takes: two w buffers of max_m x 3 doubles in 64 KiB of LDS
constexpr int kPairMaxM = 64 * 1024 / (2 * 3 * (int)sizeof(double));

PairCov* pair_cov_create();
void pair_cov_destroy(PairCov* p);
int64_t pair_cov_bytes(const PairCov* p);
// Grows the arena to the batch's size when needed and uploads the batch (synchronous copies: the arena
// is idle between batches). want[4]: cross, projected, cov_a, cov_b. 0; -2 with err (the byte count) when
// the allocation fails: the arena is then empty, nothing else is touched.
int pair_cov_upload(PairCov* p, const PairCovBatch& b, const bool want[4], std::string& err);
// The same with no per-query output: the diagonal and cross blocks alone (bos_joint_compatibility reads
// them on the device)
int pair_cov_upload_blocks(PairCov* p, const PairCovBatch& b, std::string& err);
// The path solve alone (bos_node_covariances' forward half): one wavefront per node i < n_nodes, its start
// supernode n_sn[i], first dof inside it n_loc[i] and dofs n_d[i], its slice at Y + y_off[i]; device arrays.
// max_m <= kPairMaxM is the caller's to check.
hipError_t pair_path_enqueue(const MfView& v, int max_m, int n_nodes, const int32_t* n_sn, const int32_t* n_loc, const int32_t* n_d,
                             const int64_t* y_off, double* Y, hipStream_t s);
// Enqueues the three kernels of the uploaded batch on s; after_solve (may be null) is recorded behind the
// path solve. v: the factor's view; max_m: PairPaths::max_m (<= kPairMaxM); pose / lm: the fp64 master state.
int pair_cov_enqueue(PairCov* p, const MfView& v, int max_m, int NP, const double* pose, const double* lm, hipStream_t s,
                     hipEvent_t after_solve, PairCovOut* out, std::string& err);

// The first two kernels alone, after pair_cov_upload_blocks: *diag [9 n_nodes] and *cross [9 n_queries] are
// the device blocks the product kernel fills (Sigma(a, a) per distinct node, Sigma(a, b) per query).
int pair_cov_enqueue_blocks(PairCov* p, const MfView& v, int max_m, int NP, hipStream_t s, hipEvent_t after_solve, const double** diag,
                            const double** cross, std::string& err);

}  // namespace dev
}  // namespace bos
