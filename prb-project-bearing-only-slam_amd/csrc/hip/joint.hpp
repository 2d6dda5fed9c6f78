// Joint compatibility on the device (hip/joint.hip): see host/joint.hpp for the quantities and the order of
// every operation. Per batch of whole hypotheses, in plain stream order after the pair call's path solve
// and products (hip/pair_cov.hpp pair_cov_enqueue_blocks), whose diagonal and cross blocks it reads in
// place: joint_nis_kernel, one wavefront (one workgroup) per hypothesis. No wave communicates with another,
// none uses an atomic, and a hypothesis's bits depend on its own pairings alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../host/joint.hpp"

namespace bos {
namespace dev {

struct Joint;   // the feature's device arena; owned by the solver handle

// One batch as the host prepared it (host arrays): hyp_start [n_hyp + 1] relative to the batch's first
// pairing, per pairing its pose, landmark, z and omega (never null here), per hypothesis the first entry of
// its table and the first double of its block of innovation_cov, and the table (4 references per entry).
struct JointBatch {
    int32_t n_hyp = 0, n_pair = 0;
    int64_t n_entries = 0, s_count = 0;
    const int32_t *hyp_start = nullptr, *pose = nullptr, *landmark = nullptr, *tab = nullptr;
    const int64_t *tab_off = nullptr, *s_off = nullptr;
    const double *z = nullptr, *omega = nullptr;
};
// device results of the last enqueued batch (null where not asked for)
struct JointOut {
    const double *prefix_nis = nullptr, *joint_nis = nullptr, *innovation = nullptr, *innovation_cov = nullptr;
};

constexpr int64_t kJointMaxHyp = 1 << 16;   // hypotheses of one batch (a grid dimension)

Joint* joint_create();
void joint_destroy(Joint* p);
int64_t joint_bytes(const Joint* p);
// Grows the arena to the batch's size when needed and uploads the batch (synchronous copies: the arena is
// idle between batches). want[4]: prefix_nis, joint_nis, innovation, innovation_cov. 0; -2 with err (the byte
// count) when the allocation fails: the arena is then empty.
int joint_upload(Joint* p, const JointBatch& b, const bool want[4], std::string& err);
// Enqueues the kernel of the uploaded batch on s. pose / lm: the fp64 master state; diag / cross: the pair
// call's device blocks of the same batch.
int joint_enqueue(Joint* p, const double* pose, const double* lm, const double* diag, const double* cross, hipStream_t s, JointOut* out,
                  std::string& err);

}  // namespace dev
}  // namespace bos
