// Joint-compatibility branch and bound on the device (hip/jcbb.hip): see host/jcbb.hpp for the quantities, the
// total order, the prunings and the order of every operation. Per batch of whole frames, in plain stream order
// after the pair call's path solve and products (hip/pair_cov.hpp pair_cov_enqueue_blocks), whose diagonal and
// cross blocks it reads in place: jcbb_kernel, one wavefront (one workgroup) per frame. No wave communicates
// with another, none uses an atomic, and a frame's results depend on its own bearings alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../host/jcbb.hpp"

namespace bos {
namespace dev {

struct Jcbb;   // the feature's device arena; owned by the solver handle

// One batch as the host prepared it (host arrays). Frames: bearing_start [n_frames + 1] relative to the batch's
// first bearing, cand_start [n_bearings + 1] relative to the batch's first pairing. All-pairings hypotheses
// (joint.hpp JointBatch): hyp_start [n_frames + 1] relative to the batch's first pairing, per pairing its pose,
// landmark, z and omega, per frame the first entry of its table and the first double of its block of
// innovation_cov, and the table. gate [kJointMaxM]; budget: nodes per frame (jcbb_budget).
struct JcbbBatch {
    int32_t n_frames = 0, n_bearings = 0, n_pair = 0;
    int64_t n_entries = 0, s_count = 0;
    const int32_t *bearing_start = nullptr, *cand_start = nullptr;
    const int32_t *hyp_start = nullptr, *pose = nullptr, *landmark = nullptr, *tab = nullptr;
    const int64_t *tab_off = nullptr, *s_off = nullptr;
    const double *z = nullptr, *omega = nullptr, *gate = nullptr;
    int64_t budget = 0;
};
// what the call asked for
struct JcbbWant {
    bool assignment = false, n_paired = false, joint_nis = false, prefix_nis = false, complete = false, innovation = false, cov = false;
    bool search() const { return assignment || n_paired || joint_nis || prefix_nis || complete; }
};
// device results of the last enqueued batch (null where not asked for; nodes: always, when the search ran)
struct JcbbOut {
    const int32_t *assignment = nullptr, *n_paired = nullptr, *complete = nullptr;
    const double *joint_nis = nullptr, *prefix_nis = nullptr, *innovation = nullptr, *innovation_cov = nullptr;
    const int64_t* nodes = nullptr;
};

Jcbb* jcbb_create();
void jcbb_destroy(Jcbb* p);
int64_t jcbb_bytes(const Jcbb* p);
// Grows the arena to the batch's size when needed and uploads the batch (synchronous copies: the arena is idle
// between batches). 0; -2 with err (the byte count) when the allocation fails: the arena is then empty.
int jcbb_upload(Jcbb* p, const JcbbBatch& b, const JcbbWant& want, std::string& err);
// Enqueues the kernel of the uploaded batch on s. pose / lm: the fp64 master state; diag / cross: the pair
// call's device blocks of the same batch.
int jcbb_enqueue(Jcbb* p, const double* pose, const double* lm, const double* diag, const double* cross, hipStream_t s, JcbbOut* out,
                 std::string& err);

}  // namespace dev
}  // namespace bos
