// bos_set_priors on the C ABI handle (solver_handle.hpp): the checks and packing of host/prior_set.hpp,
// the device copies the prior kernel (hip/prior.hpp) and the cost pass (hip/lm.hpp) read, and the swap of
// the handle's set. The kernel itself is launched by enqueue_linearize (solver_step.hip).
#include "solver_handle.hpp"

#include "../host/prior_set.hpp"

using namespace bos::capi;

namespace {

// the records in T, padded for the kernel's vector loads (hip/prior.hpp)
template <typename T> void pack_records(const bos::PriorSet& P, std::vector<T>& pose, std::vector<T>& lm) {
    pose.assign((size_t)bos::dev::kPriorPoseRec * P.pose.size(), (T)0);
    lm.assign((size_t)bos::dev::kPriorLmRec * P.lm.size(), (T)0);
    for (size_t i = 0; i < P.pose.size(); ++i)
        for (int v = 0; v < 9; ++v) pose[bos::dev::kPriorPoseRec * i + v] = (T)P.pose_rec[9 * i + v];
    for (size_t i = 0; i < P.lm.size(); ++i)
        for (int v = 0; v < 5; ++v) lm[bos::dev::kPriorLmRec * i + v] = (T)P.lm_rec[5 * i + v];
}

}  // namespace

extern "C" {

int bos_set_priors(bos_solver* s, int32_t n_pose, const int32_t* pose, const double* pose_mean, const double* pose_omega,
                   int32_t n_landmark, const int32_t* landmark, const double* landmark_mean, const double* landmark_omega) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    int rc;
    if ((rc = require_one_gpu(s, "bos_set_priors", false, " (a rank builds part of H)"))) return rc;
    bos::PriorSet P;
    const std::string err = bos::prior_set_build(s->NP, s->NL, s->plan.fixed, n_pose, pose, pose_mean, pose_omega, n_landmark,
                                                 landmark, landmark_mean, landmark_omega, P);
    if (!err.empty()) return fail(BOS_ERR_INVALID, "bos_set_priors: " + err);
    HIP_TRY(hipSetDevice(s->device));
    // the new set's buffers first: a failure leaves the handle with the set it had
    char* arena = nullptr;
    int32_t* idx = nullptr;
    void *rp = nullptr, *rl = nullptr;
    double *rp64 = nullptr, *rl64 = nullptr, *part = nullptr;
    if (!P.empty()) {
        std::vector<int32_t> nodes(P.pose);
        nodes.insert(nodes.end(), P.lm.begin(), P.lm.end());
        bos::dev::Arena ar;
        ar.add(&idx, nodes);
        ar.add(&rp64, P.pose_rec);
        ar.add(&rl64, P.lm_rec);
        std::vector<float> fp, fl;
        std::vector<double> dp, dl;
        float *rpf = nullptr, *rlf = nullptr;
        double *rpd = nullptr, *rld = nullptr;
        if (s->precision == BOS_FP32) {
            pack_records<float>(P, fp, fl);
            ar.add(&rpf, fp);
            ar.add(&rlf, fl);
        } else {
            pack_records<double>(P, dp, dl);
            ar.add(&rpd, dp);
            ar.add(&rld, dl);
        }
        ar.zeros(&part, (size_t)bos::dev::prior_parts((int64_t)nodes.size()));
        if (!ar.commit(s->mem, &arena))
            return fail(BOS_ERR_DEVICE, "bos_set_priors: cannot allocate or upload " + std::to_string(ar.bytes()) + " bytes");
        rp = s->precision == BOS_FP32 ? (void*)rpf : (void*)rpd;
        rl = s->precision == BOS_FP32 ? (void*)rlf : (void*)rld;
    }
    // the captured step graphs and LM iteration hold the old launches and arguments (drop_graph waits for
    // the stream first: a graph may still be running, and reads the old set's buffers)
    drop_graph(s);
    s->mem.release(s->prior_arena);
    s->prior_arena = arena;
    s->n_pose_priors = (int)P.pose.size();
    s->n_lm_priors = (int)P.lm.size();
    s->pr_idx = idx;
    s->pr_pose = rp;
    s->pr_lm = rl;
    s->pr_pose64 = rp64;
    s->pr_lm64 = rl64;
    s->pr_part = part;
    return BOS_OK;
}

}  // extern "C"
