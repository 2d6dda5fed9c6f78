// The covariance calls built on the pair call's root-path solves (hip/pair_cov.hpp): bos_pair_covariances,
// bos_joint_compatibility (hip/joint.hpp) and bos_jcbb (hip/jcbb.hpp), their timing getters and batch knobs.
// The calls' frame is cov_call.hpp's.
#include "cov_call.hpp"

namespace bos {
namespace capi {

// One batch of bos_joint_compatibility and of bos_jcbb, which runs on the joint call's batches of all-pairings
// hypotheses: the batch from h0 on (joint_batch_build), the pair call's blocks uploaded, the feature's own batch
// uploaded by upload(B, err) (0, or pair_cov's codes), then between the handle's events 3 .. 6 the pair call's path
// solve and products and the feature's kernel, enqueued by enqueue(diag, cross, err), and the wait. batch_limit:
// the feature's knob (0: kJointMaxHyp); ms: the feature's seven slots (0, 3, 4, 5 are added to).
template <class Upload, class Enqueue>
int joint_batch_run(bos_solver* s, int32_t n_hyp, const int32_t* hyp_start, const int32_t* pose, const int32_t* landmark, int32_t h0,
                    int64_t batch_limit, bos::JointBatchHost& B, double* ms, Upload upload, Enqueue enqueue) {
    const auto t_prep = Clock::now();
    const int64_t max_hyp = batch_limit > 0 ? batch_limit : bos::dev::kJointMaxHyp;
    if (s->joint_slot_of.empty()) s->joint_slot_of.assign((size_t)s->NP + s->NL, -1);   // all -1 between batches
    bos::joint_batch_build(s->plan, s->pair_paths, n_hyp, hyp_start, pose, landmark, h0,
                           bos::dev::kPairYBudgetBytes / (int64_t)sizeof(double), max_hyp, bos::dev::kPairMaxQueries, s->joint_slot_of, B);
    std::string err;
    int prc = bos::dev::pair_cov_upload_blocks(s->pair, pair_batch_view(B.pairs, B.pair_a.data(), B.pair_b.data()), err);
    if (!prc) prc = upload(B, err);
    if (prc) return dev_fail(prc, err);
    ms[0] += ms_since(t_prep);
    const double *diag = nullptr, *cross = nullptr;
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    prc = bos::dev::pair_cov_enqueue_blocks(s->pair, bos::dev::mf_view(s->mf), s->pair_paths.max_m, s->NP, s->stream, s->ev[4], &diag,
                                            &cross, err);
    hipError_t e = hipEventRecord(s->ev[5], s->stream);
    if (!prc && e == hipSuccess) prc = enqueue(diag, cross, err);
    if (e == hipSuccess) e = hipEventRecord(s->ev[6], s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    HIP_TRY(e);
    if (prc) return dev_fail(prc, err);
    ms[3] += elapsed(s->ev[3], s->ev[4]);
    ms[4] += elapsed(s->ev[4], s->ev[5]);
    ms[5] += elapsed(s->ev[5], s->ev[6]);
    return BOS_OK;
}

}  // namespace capi
}  // namespace bos

using namespace bos::capi;

extern "C" {

int bos_pair_covariances(bos_solver* s, int64_t n_pairs, const int32_t* node_a, const int32_t* node_b, double* cross,
                         double* projected, double* cov_a, double* cov_b, int32_t* solver_info) {
    const char* name = "bos_pair_covariances";
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!node_a || !node_b))) return fail(BOS_ERR_INVALID, std::string(name) + ": bad argument");
    if (n_pairs == 0) return BOS_OK;
    if (!bos::pair_ids_valid(s->NP, s->NL, n_pairs, node_a, node_b))
        return fail(BOS_ERR_INVALID, std::string(name) + ": a node id outside [0, NP + NL), or a mixed pair not written (pose, landmark)");
    double* const outs[4] = {cross, projected, cov_a, cov_b};
    bool want[4];
    for (int i = 0; i < 4; ++i) want[i] = outs[i] != nullptr;
    CovCall c{s, s->pair_ms, 6, solver_info};
    if ((rc = c.begin())) return rc;
    if (s->plan.n == 0) {   // the fixed pose alone
        for (int i = 0; i < 4; ++i)
            if (want[i]) std::fill(outs[i], outs[i] + 9 * n_pairs, 0.0);
        return BOS_OK;
    }
    if ((rc = pair_paths_setup(s, name))) return rc;
    if (!s->pair) s->pair = bos::dev::pair_cov_create();
    if ((rc = c.factor())) return rc;
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    const int64_t max_nodes = s->pair_batch_nodes > 0 ? std::max<int64_t>(s->pair_batch_nodes, 2) : INT32_MAX;
    std::vector<int32_t> slot_of((size_t)s->NP + s->NL, -1);
    bos::PairBatchHost B;
    for (int64_t q0 = 0; q0 < n_pairs; q0 += B.nq) {
        const auto t_prep = Clock::now();
        bos::pair_batch_build(s->plan, s->pair_paths, n_pairs, node_a, node_b, q0, max_nodes,
                              bos::dev::kPairYBudgetBytes / (int64_t)sizeof(double), bos::dev::kPairMaxQueries, slot_of, B);
        std::string err;
        int prc = bos::dev::pair_cov_upload(s->pair, pair_batch_view(B, node_a + q0, node_b + q0), want, err);
        if (prc) return dev_fail(prc, err);
        c.host_ms(0, t_prep);
        bos::dev::PairCovOut res;
        HIP_TRY(hipEventRecord(s->ev[3], s->stream));
        prc = bos::dev::pair_cov_enqueue(s->pair, view, s->pair_paths.max_m, s->NP, s->d_pose, s->d_lm, s->stream, s->ev[4], &res, err);
        if ((rc = c.drain(5, prc, err))) return rc;
        s->pair_ms[3] += elapsed(s->ev[3], s->ev[4]);
        s->pair_ms[4] += elapsed(s->ev[4], s->ev[5]);
        const auto t_dl = Clock::now();
        const double* dev[4] = {res.cross, res.projected, res.cov_a, res.cov_b};
        for (int i = 0; i < 4; ++i)
            if (want[i]) HIP_TRY(hipMemcpy(outs[i] + 9 * q0, dev[i], 9 * (size_t)B.nq * sizeof(double), hipMemcpyDeviceToHost));
        c.host_ms(5, t_dl);
    }
    return c.done();
}

int bos_pair_covariances_timing(const bos_solver* s, double ms[6], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->pair_ms, 6, ms, bytes, bos::dev::pair_cov_bytes(s->pair));
}

int bos_debug_set_pair_batch(bos_solver* s, int64_t max_distinct_nodes) {
    if (!s || max_distinct_nodes < 0) return fail(BOS_ERR_INVALID, "bad argument");
    s->pair_batch_nodes = max_distinct_nodes;
    return BOS_OK;
}

int bos_joint_compatibility(bos_solver* s, int32_t n_hyp, const int32_t* hyp_start, const int32_t* pose, const int32_t* landmark,
                            const double* z, const double* omega, double* prefix_nis, double* joint_nis, double* innovation,
                            double* innovation_cov, int32_t* solver_info) {
    const char* name = "bos_joint_compatibility";
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
    if (const char* bad = bos::joint_bad_argument(s->NP, s->NL, n_hyp, hyp_start, pose, landmark, z, omega))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_hyp == 0) return BOS_OK;
    double* const outs[4] = {prefix_nis, joint_nis, innovation, innovation_cov};
    bool want[4];
    for (int i = 0; i < 4; ++i) want[i] = outs[i] != nullptr;
    CovCall c{s, s->joint_ms, 7, solver_info};
    if ((rc = c.begin())) return rc;
    if (s->plan.n == 0) {   // the fixed pose alone: no landmark, so every hypothesis is empty
        if (joint_nis) std::fill(joint_nis, joint_nis + n_hyp, 0.0);
        return BOS_OK;
    }
    if ((rc = pair_paths_setup(s, name))) return rc;
    if (!s->pair) s->pair = bos::dev::pair_cov_create();
    if (!s->joint) s->joint = bos::dev::joint_create();
    const int32_t n_pair = hyp_start[n_hyp];
    std::vector<double> ones;
    if (!omega) ones.assign((size_t)n_pair + 1, 1.0);
    const double* om = omega ? omega : ones.data();
    if ((rc = c.factor())) return rc;
    std::vector<int32_t> local_start;
    bos::JointBatchHost B;
    int64_t s_done = 0;
    for (int32_t h0 = 0; h0 < n_hyp; h0 += B.nh) {
        int32_t p0 = 0, np = 0;
        bos::dev::JointOut res;
        rc = joint_batch_run(
            s, n_hyp, hyp_start, pose, landmark, h0, s->joint_batch, B, s->joint_ms,
            [&](const bos::JointBatchHost& B, std::string& err) {
                p0 = hyp_start[h0];
                np = hyp_start[h0 + B.nh] - p0;
                local_start.resize((size_t)B.nh + 1);
                for (int32_t h = 0; h <= B.nh; ++h) local_start[h] = hyp_start[h0 + h] - p0;
                bos::dev::JointBatch jb;
                jb.n_hyp = B.nh; jb.n_pair = np; jb.n_entries = B.n_entries; jb.s_count = B.s_count;
                jb.hyp_start = local_start.data(); jb.pose = pose + p0; jb.landmark = landmark + p0; jb.tab = B.tab.data();
                jb.tab_off = B.tab_off.data(); jb.s_off = B.s_off.data(); jb.z = z + p0; jb.omega = om + p0;
                return bos::dev::joint_upload(s->joint, jb, want, err);
            },
            [&](const double* diag, const double* cross, std::string& err) {
                return bos::dev::joint_enqueue(s->joint, s->d_pose, s->d_lm, diag, cross, s->stream, &res, err);
            });
        if (rc) return rc;
        const auto t_dl = Clock::now();
        const double* dev[4] = {res.prefix_nis, res.joint_nis, res.innovation, res.innovation_cov};
        double* const dst[4] = {prefix_nis ? prefix_nis + p0 : nullptr, joint_nis ? joint_nis + h0 : nullptr,
                                innovation ? innovation + p0 : nullptr, innovation_cov ? innovation_cov + s_done : nullptr};
        const size_t count[4] = {(size_t)np, (size_t)B.nh, (size_t)np, (size_t)B.s_count};
        for (int i = 0; i < 4; ++i)
            if (want[i] && count[i]) HIP_TRY(hipMemcpy(dst[i], dev[i], count[i] * sizeof(double), hipMemcpyDeviceToHost));
        s_done += B.s_count;
        c.host_ms(6, t_dl);
    }
    return c.done();
}

int bos_joint_compatibility_timing(const bos_solver* s, double ms[7], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->joint_ms, 7, ms, bytes, bos::dev::joint_bytes(s->joint) + bos::dev::pair_cov_bytes(s->pair));
}

int bos_debug_set_joint_batch(bos_solver* s, int64_t max_hypotheses) {
    if (!s || max_hypotheses < 0) return fail(BOS_ERR_INVALID, "bos_debug_set_joint_batch: bad argument");
    s->joint_batch = max_hypotheses;
    return BOS_OK;
}

int bos_jcbb(bos_solver* s, int32_t n_frames, const int32_t* frame_start, const int32_t* pose, const double* z, const double* omega,
             const int32_t* cand_start, const int32_t* cand_landmark, const double* gate, int64_t max_nodes, int32_t* assignment,
             int32_t* n_paired, double* joint_nis, double* prefix_nis, int32_t* complete, double* innovation, double* innovation_cov,
             int32_t* solver_info) {
    const char* name = "bos_jcbb";
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
    if (const char* bad = bos::jcbb_bad_argument(s->NP, s->NL, n_frames, frame_start, pose, z, omega, cand_start, cand_landmark, gate,
                                                 max_nodes))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_frames == 0) return BOS_OK;
    bos::dev::JcbbWant want;
    want.assignment = assignment != nullptr; want.n_paired = n_paired != nullptr; want.joint_nis = joint_nis != nullptr;
    want.prefix_nis = prefix_nis != nullptr; want.complete = complete != nullptr; want.innovation = innovation != nullptr;
    want.cov = innovation_cov != nullptr;
    CovCall c{s, s->jcbb_ms, 7, solver_info};
    if ((rc = c.begin())) return rc;
    const int32_t n_bearings = frame_start[n_frames];
    s->jcbb_nodes.assign((size_t)n_frames, 0);
    if (s->plan.n == 0) {   // the fixed pose alone: no landmark, so every list is empty
        if (assignment) std::fill(assignment, assignment + n_bearings, -1);
        if (n_paired) std::fill(n_paired, n_paired + n_frames, 0);
        if (joint_nis) std::fill(joint_nis, joint_nis + n_frames, 0.0);
        if (prefix_nis) std::fill(prefix_nis, prefix_nis + n_bearings, 0.0);
        if (complete) std::fill(complete, complete + n_frames, 1);
        return BOS_OK;
    }
    if ((rc = pair_paths_setup(s, name))) return rc;
    if (!s->pair) s->pair = bos::dev::pair_cov_create();
    if (!s->jcbb) s->jcbb = bos::dev::jcbb_create();
    bos::JcbbPairings A;   // the frames as all-pairings hypotheses
    bos::jcbb_pairings(n_frames, frame_start, pose, z, omega, cand_start, A);
    const int32_t* hyp_start = A.hyp_start.data();
    if ((rc = c.factor())) return rc;
    std::vector<int32_t> local_hyp, local_bearing, local_cand;
    bos::JointBatchHost B;
    int64_t s_done = 0;
    for (int32_t h0 = 0; h0 < n_frames; h0 += B.nh) {
        int32_t p0 = 0, np = 0, b0 = 0, nb = 0;
        bos::dev::JcbbOut res;
        rc = joint_batch_run(
            s, n_frames, hyp_start, A.pose.data(), cand_landmark, h0, s->jcbb_batch, B, s->jcbb_ms,
            [&](const bos::JointBatchHost& B, std::string& err) {
                p0 = hyp_start[h0];
                np = hyp_start[h0 + B.nh] - p0;
                b0 = frame_start[h0];
                nb = frame_start[h0 + B.nh] - b0;
                local_hyp.resize((size_t)B.nh + 1);
                local_bearing.resize((size_t)B.nh + 1);
                for (int32_t h = 0; h <= B.nh; ++h) {
                    local_hyp[h] = hyp_start[h0 + h] - p0;
                    local_bearing[h] = frame_start[h0 + h] - b0;
                }
                local_cand.resize((size_t)nb + 1);
                for (int32_t i = 0; i <= nb; ++i) local_cand[i] = cand_start[b0 + i] - p0;
                bos::dev::JcbbBatch jb;
                jb.n_frames = B.nh; jb.n_bearings = nb; jb.n_pair = np; jb.n_entries = B.n_entries; jb.s_count = B.s_count;
                jb.bearing_start = local_bearing.data(); jb.cand_start = local_cand.data();
                jb.hyp_start = local_hyp.data(); jb.pose = A.pose.data() + p0; jb.landmark = cand_landmark ? cand_landmark + p0 : nullptr;
                jb.tab = B.tab.data(); jb.tab_off = B.tab_off.data(); jb.s_off = B.s_off.data();
                jb.z = A.z.data() + p0; jb.omega = A.omega.data() + p0; jb.gate = gate; jb.budget = bos::jcbb_budget(max_nodes);
                return bos::dev::jcbb_upload(s->jcbb, jb, want, err);
            },
            [&](const double* diag, const double* cross, std::string& err) {
                return bos::dev::jcbb_enqueue(s->jcbb, s->d_pose, s->d_lm, diag, cross, s->stream, &res, err);
            });
        if (rc) return rc;
        const auto t_dl = Clock::now();
        auto download = [&](void* dst, const void* src, size_t bytes) {
            return dst && src && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
        };
        HIP_TRY(download(assignment ? assignment + b0 : nullptr, res.assignment, (size_t)nb * sizeof(int32_t)));
        HIP_TRY(download(n_paired ? n_paired + h0 : nullptr, res.n_paired, (size_t)B.nh * sizeof(int32_t)));
        HIP_TRY(download(complete ? complete + h0 : nullptr, res.complete, (size_t)B.nh * sizeof(int32_t)));
        HIP_TRY(download(joint_nis ? joint_nis + h0 : nullptr, res.joint_nis, (size_t)B.nh * sizeof(double)));
        HIP_TRY(download(prefix_nis ? prefix_nis + b0 : nullptr, res.prefix_nis, (size_t)nb * sizeof(double)));
        HIP_TRY(download(innovation ? innovation + p0 : nullptr, res.innovation, (size_t)np * sizeof(double)));
        HIP_TRY(download(innovation_cov ? innovation_cov + s_done : nullptr, res.innovation_cov, (size_t)B.s_count * sizeof(double)));
        HIP_TRY(download(s->jcbb_nodes.data() + h0, res.nodes, (size_t)B.nh * sizeof(int64_t)));
        s_done += B.s_count;
        c.host_ms(6, t_dl);
    }
    return c.done();
}

int bos_jcbb_timing(const bos_solver* s, double ms[7], int64_t* bytes, int64_t capacity, int64_t* nodes, int32_t* n_frames) {
    if (!s || !ms || capacity < 0 || (capacity > 0 && !nodes)) return fail(BOS_ERR_INVALID, "bos_jcbb_timing: bad argument");
    timing_out(s->jcbb_ms, 7, ms, bytes, bos::dev::jcbb_bytes(s->jcbb) + bos::dev::pair_cov_bytes(s->pair));
    const int64_t n = std::min<int64_t>(capacity, (int64_t)s->jcbb_nodes.size());
    for (int64_t i = 0; i < n; ++i) nodes[i] = s->jcbb_nodes[(size_t)i];
    if (n_frames) *n_frames = (int32_t)s->jcbb_nodes.size();
    return BOS_OK;
}

int bos_debug_set_jcbb_batch(bos_solver* s, int64_t max_frames) {
    if (!s || max_frames < 0) return fail(BOS_ERR_INVALID, "bos_debug_set_jcbb_batch: bad argument");
    s->jcbb_batch = max_frames;
    return BOS_OK;
}

}  // extern "C"
