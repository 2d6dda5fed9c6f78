// Covariances from the multifrontal factor on the C ABI handle (solver_handle.hpp): what every covariance call
// shares (cov_call.hpp), and the pass over the whole selected inverse, bos_marginals and bos_edge_covariances
// (hip/selinv.hpp), with bos_edge_consistency, which scores every edge against that pass's projection
// (hip/edge_check.hpp). The pair-path calls are in solver_cov_pair.hip, the node-column calls in solver_cov_node.hip.
#include <cmath>

#include "cov_call.hpp"

namespace bos {
namespace capi {

// The feature's device state at the first bos_edge_covariances (hip/selinv.hip mf_edge_cov_build): the
// edges in measurement order are the handle's table of the bearings' landmarks and the device copies it
// already keeps (the bearings' poses, the odometry's endpoints)
int edge_cov_setup(bos_solver* s) {
    if (bos::dev::mf_edge_cov_built(s->mf)) return BOS_OK;
    std::vector<int32_t> bp(s->Mb, 0), os(s->Mo, 0), od(s->Mo, 0);
    const std::vector<int32_t>& bl = s->bearing_lm;
    if (s->Mb) HIP_TRY(hipMemcpy(bp.data(), s->tri_pose, bp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (s->Mo) {
        HIP_TRY(hipMemcpy(os.data(), s->o_src, os.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(od.data(), s->o_dst, od.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    bos::dev::EdgeList E;
    E.Mb = s->Mb; E.Mo = s->Mo;
    E.b_pose = bp.data(); E.b_lm = bl.data(); E.o_src = os.data(); E.o_dst = od.data();
    std::string err;
    const int rc = bos::dev::mf_edge_cov_build(s->mf, s->plan, E, err);
    if (rc) return dev_fail(rc, err);
    return BOS_OK;
}

// the factorization's word read and cleared (a step expects it zero), the stream drained
hipError_t take_factor_info(bos_solver* s, int32_t* info) {
    hipError_t e = hipMemcpyAsync(info, bos::dev::mf_info_ptr(s->mf), sizeof(*info), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(bos::dev::mf_info_ptr(s->mf), 0, sizeof(int32_t), s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    return e;
}

// The shared start of a covariance call: the system of bos_linearize and its factorization, as a step
// enqueues them (bos_step returns on its status word, before the stream has drained: everything here is
// ordered after it by the stream), between events 0, 1 and 2. With info_now the factorization's word is
// read and cleared and the stream drained before anything reads the panels; a caller that passes null
// takes the word later (take_factor_info).
int enqueue_factorization(bos_solver* s, int32_t* info_now) {
    int rc;
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    if ((rc = enqueue_linearize(s))) return rc;
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    if ((rc = enqueue_solver_inputs(s))) return rc;   // opens the flows' epoch, as a step does
    HIP_TRY(bos::dev::mf_factor(s->mf, 0, mf_matrix(s), s->d_rhs, s->stream));
    s->have_dx = false;   // d_rhs now holds L^-1 b of this factorization
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    if (info_now) HIP_TRY(take_factor_info(s, info_now));
    return BOS_OK;
}

// The static path data of the pair and node covariances, at the first call of either
int pair_paths_setup(bos_solver* s, const char* name) {
    if (s->pair_paths_built) return BOS_OK;
    std::string err;
    if (!bos::pair_paths_build(s->plan, s->pair_paths, err)) return fail(BOS_ERR_UNSUPPORTED, err);
    if (s->pair_paths.max_m > bos::dev::kPairMaxM)
        return fail(BOS_ERR_UNSUPPORTED, std::string(name) + ": a front exceeds the path solve's LDS");
    s->pair_paths_built = true;
    return BOS_OK;
}

// The node call's plan and arena, at the first call that needs a node column
int node_cov_setup(bos_solver* s, const char* name) {
    if (bos::dev::node_cov_built(s->node)) return BOS_OK;
    int rc;
    std::string err;
    if ((rc = pair_paths_setup(s, name))) return rc;
    if (!bos::node_cov_plan_build(s->plan, s->pair_paths, s->node_plan, err)) return fail(BOS_ERR_UNSUPPORTED, err);
    if (!s->node) s->node = bos::dev::node_cov_create();
    if (bos::dev::node_cov_build(s->node, s->plan, s->pair_paths, s->node_plan, err)) return fail(BOS_ERR_DEVICE, err);
    return BOS_OK;
}

int cov_handle_check(const bos_solver* s, const char* name) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    return require_one_gpu(s, name, true, " (a rank holds part of the factor)");
}

int CovCall::begin() {
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    std::fill_n(ms, n_ms, 0.0);
    t_begin = Clock::now();
    return BOS_OK;
}

int CovCall::factor() {
    int rc;
    host_ms(0, t_begin);
    if ((rc = enqueue_factorization(s, &info))) return rc;
    ms[1] = elapsed(s->ev[0], s->ev[1]);
    ms[2] = elapsed(s->ev[1], s->ev[2]);
    return info & bos::dev::kMfStall ? stall_fail() : BOS_OK;
}

int CovCall::selected_inverse(const double** sig, bool emit_cross) {
    int rc;
    std::string err;
    if ((rc = drain(3, bos::dev::mf_selected_inverse(s->mf, s->plan, sig, s->stream, err, emit_cross), err))) return rc;
    ms[3] = elapsed(s->ev[2], s->ev[3]);
    return BOS_OK;
}

int CovCall::drain(int ev, int prc, const std::string& err) {
    hipError_t e = hipEventRecord(s->ev[ev], s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    HIP_TRY(e);
    return prc ? dev_fail(prc, err) : BOS_OK;
}

}  // namespace capi
}  // namespace bos

using namespace bos::capi;

namespace {

// bos_marginals (edge = nullptr) and bos_edge_covariances (edge[4] = bearing_cross, odom_cross,
// bearing_var, odom_cov; with all four null the pass is the marginals' own). Not a CovCall: the slots are
// not cleared, and the factorization's word is taken after the selected inverse has been enqueued.
int covariance_pass(bos_solver* s, const char* name, double* const* edge, double* pose_cov, double* landmark_cov,
                    int32_t* solver_info) {
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    const int64_t n = s->plan.n;
    const size_t np9 = 9 * (size_t)s->NP, nl4 = 4 * (size_t)s->NL;
    const size_t ecount[4] = {6 * (size_t)s->Mb, 9 * (size_t)s->Mo, (size_t)s->Mb, 9 * (size_t)s->Mo};
    bool want[4] = {false, false, false, false};
    bool any_edge = false;
    for (int i = 0; i < 4 && edge; ++i) any_edge |= want[i] = edge[i] != nullptr && ecount[i] > 0;
    if (n == 0) {   // the fixed pose alone: every block and every cross block is zero
        if (pose_cov) std::fill(pose_cov, pose_cov + np9, 0.0);
        if (landmark_cov) std::fill(landmark_cov, landmark_cov + nl4, 0.0);
        for (int i = 0; i < 4; ++i)
            if (want[i]) std::fill(edge[i], edge[i] + ecount[i], 0.0);
        return BOS_OK;
    }
    if (any_edge && (rc = edge_cov_setup(s))) return rc;
    if ((rc = enqueue_factorization(s, nullptr))) return rc;
    const double* out = nullptr;
    std::string err;
    int src = bos::dev::mf_selected_inverse(s->mf, s->plan, &out, s->stream, err, any_edge);
    // the factorization's word, read and cleared whatever happened next: a step expects it zero
    int32_t info = 0;
    hipError_t e = hipEventRecord(s->ev[3], s->stream);
    bos::dev::EdgeCovResult er;
    if (any_edge && !src && e == hipSuccess) {
        src = bos::dev::mf_edge_project(s->mf, s->d_pose, s->d_lm, want, &er, s->stream, err);
        e = hipEventRecord(s->ev[4], s->stream);
    }
    if (e == hipSuccess) e = take_factor_info(s, &info);
    HIP_TRY(e);
    if (src) return dev_fail(src, err);
    if (info & bos::dev::kMfStall) return stall_fail();
    const auto t0 = Clock::now();
    if (pose_cov) HIP_TRY(hipMemcpy(pose_cov, out, np9 * sizeof(double), hipMemcpyDeviceToHost));
    if (landmark_cov && nl4) HIP_TRY(hipMemcpy(landmark_cov, out + np9, nl4 * sizeof(double), hipMemcpyDeviceToHost));
    if (any_edge) {
        const double* dev[4] = {er.bearing_cross, er.odom_cross, er.bearing_var, er.odom_cov};
        for (int i = 0; i < 4; ++i)
            if (want[i]) HIP_TRY(hipMemcpy(edge[i], dev[i], ecount[i] * sizeof(double), hipMemcpyDeviceToHost));
    }
    const double dl = ms_since(t0);
    if (edge) {
        for (int i = 0; i < 3; ++i) s->edge_ms[i] = elapsed(s->ev[i], s->ev[i + 1]);
        s->edge_ms[3] = any_edge ? elapsed(s->ev[3], s->ev[4]) : 0.0;
        s->edge_ms[4] = dl;
    } else {
        s->marg_ms[3] = dl;
        for (int i = 0; i < 3; ++i) s->marg_ms[i] = elapsed(s->ev[i], s->ev[i + 1]);
    }
    if (solver_info) *solver_info = info;
    return BOS_OK;
}

// bos_edge_consistency's state at its first call: the edge call's (whose projection it reads in place), the cost
// pass's fp64 measurements, and its own arena with R = Omega^-1 of every odometry edge, formed here once
int edge_check_setup(bos_solver* s) {
    if (bos::dev::edge_check_built(s->edge_check)) return BOS_OK;
    int rc;
    if ((rc = edge_cov_setup(s))) return rc;
    if ((rc = lm_buffers_setup(s))) return rc;
    std::vector<double> R(6 * (size_t)s->Mo);
    for (size_t k = 0; k < (size_t)s->Mo; ++k) bos::edge_check_information_inverse(&s->h_oom[6 * k], &R[6 * k]);
    if (!s->edge_check) s->edge_check = bos::dev::edge_check_create();
    std::string err;
    if (bos::dev::edge_check_build(s->edge_check, s->Mb, s->Mo, R.data(), err)) return fail(BOS_ERR_DEVICE, err);
    return BOS_OK;
}

// One kind's host outputs of bos_edge_consistency (any may be null): the lists of k entries, e of D and T of
// D x D doubles per entry, the count, and the rows over the kind's M edges
struct CheckOutputs {
    int32_t* cand;
    double *cand_w2, *cand_e, *cand_T;
    int32_t* n_over;
    double *w2, *chi2, *red;
    size_t D, M;

    bool lists() const { return cand || cand_w2 || cand_e || cand_T || n_over; }
    bool rows() const { return w2 || chi2 || red; }
    // the first k entries of the device's lists, or (L null) the lists as they stay where nothing is listed
    void take(const bos::dev::EdgeCheckLists* L, size_t k) const {
        for (size_t j = 0; j < k; ++j) {
            if (cand) cand[j] = L ? L->ix[j] : -1;
            if (cand_w2) cand_w2[j] = L ? L->w2[j] : -HUGE_VAL;
            for (size_t i = 0; i < D && cand_e; ++i) cand_e[j * D + i] = L ? L->e[j][i] : 0.0;
            for (size_t i = 0; i < D * D && cand_T; ++i) cand_T[j * D * D + i] = L ? L->T[j][i] : 0.0;
        }
        if (n_over) *n_over = L ? L->n_over : 0;
    }
    // the rows from the device: w2 is the exact negation of the scores the selection read
    int download(const double* d_neg, const double* d_chi2, const double* d_red) const {
        if (w2) {
            HIP_TRY(hipMemcpy(w2, d_neg, M * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < M; ++i) w2[i] = -w2[i];
        }
        if (chi2) HIP_TRY(hipMemcpy(chi2, d_chi2, M * sizeof(double), hipMemcpyDeviceToHost));
        if (red) HIP_TRY(hipMemcpy(red, d_red, M * sizeof(double), hipMemcpyDeviceToHost));
        return BOS_OK;
    }
};

// The fixed pose alone (plan.n == 0: no landmark, hence no bearing, and every odometry edge a self-loop on that
// pose): P is zero everywhere, the lists are padding, the counts 0, w2 and the redundancy NaN, and chi2 is
// evaluated here by the shared code at the handle's state
int edge_check_fixed_pose_alone(bos_solver* s, const CheckOutputs& b, const CheckOutputs& o, size_t k) {
    b.take(nullptr, k);
    o.take(nullptr, k);
    if (!o.rows() || s->Mo == 0) return BOS_OK;
    double x[3];
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(x, s->d_pose, sizeof(x), hipMemcpyDeviceToHost));
    const double zero[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t j = 0; j < (size_t)s->Mo; ++j) {
        double e[3], J[18], R[6];
        const double* z = &s->h_oz[3 * j];
        bos::odometry_error_jacobian<double>(x[0], x[1], x[2], std::cos(x[2]), std::sin(x[2]), x[0], x[1], x[2], z[0], z[1], z[2], e, J);
        bos::edge_check_information_inverse(&s->h_oom[6 * j], R);
        bos::EdgeCheckOdom r;
        bos::edge_check_odometry(e, &s->h_oom[6 * j], R, zero, true, r);
        if (o.w2) o.w2[j] = r.w2;
        if (o.chi2) o.chi2[j] = r.chi2;
        if (o.red) o.red[j] = r.redundancy;
    }
    return BOS_OK;
}

}  // namespace

extern "C" {

int bos_edge_consistency(bos_solver* s, double gate_bearing, double gate_odom, int32_t k, int32_t* cand_bearing, double* cand_bearing_w2,
                         double* cand_bearing_innovation, double* cand_bearing_resvar, int32_t* n_over_bearing, int32_t* cand_odom,
                         double* cand_odom_w2, double* cand_odom_innovation, double* cand_odom_rescov, int32_t* n_over_odom,
                         double* bearing_w2, double* bearing_chi2, double* bearing_redundancy, double* odom_w2, double* odom_chi2,
                         double* odom_redundancy, int32_t* solver_info) {
    const char* name = "bos_edge_consistency";
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
    if (const char* bad = bos::edge_check_bad_argument(gate_bearing, gate_odom, k)) return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    const CheckOutputs b = {cand_bearing, cand_bearing_w2, cand_bearing_innovation, cand_bearing_resvar, n_over_bearing,
                            bearing_w2, bearing_chi2, bearing_redundancy, 1, (size_t)s->Mb};
    const CheckOutputs o = {cand_odom, cand_odom_w2, cand_odom_innovation, cand_odom_rescov, n_over_odom,
                            odom_w2, odom_chi2, odom_redundancy, 3, (size_t)s->Mo};
    CovCall c{s, s->check_ms, 7, solver_info};
    if ((rc = c.begin())) return rc;
    if (s->plan.n == 0) return edge_check_fixed_pose_alone(s, b, o, (size_t)k);
    // a kind without edges is padding; one nothing is asked of is neither scored nor selected
    const bool kind[2] = {s->Mb > 0 && (b.lists() || b.rows()), s->Mo > 0 && (o.lists() || o.rows())};
    const bool select[2] = {kind[0] && b.lists(), kind[1] && o.lists()};
    const bool any = kind[0] || kind[1];
    if (any && (rc = edge_check_setup(s))) return rc;
    if ((rc = c.factor())) return rc;
    if (!kind[0]) b.take(nullptr, (size_t)k);
    if (!kind[1]) o.take(nullptr, (size_t)k);
    if (!any) return c.done();
    const double* sig = nullptr;
    if ((rc = c.selected_inverse(&sig, true))) return rc;
    const bool want[4] = {false, false, kind[0], kind[1]};
    std::string err;
    bos::dev::EdgeCovResult er;
    bos::dev::EdgeCheckDev res;
    int prc = bos::dev::mf_edge_project(s->mf, s->d_pose, s->d_lm, want, &er, s->stream, err);
    if (!prc) {
        bos::dev::EdgeCheckIn in;
        in.Mb = s->Mb; in.Mo = s->Mo;
        in.pose = s->d_pose; in.lm = s->d_lm;
        in.b_pose = s->tri_pose; in.b_lm = s->lm_blm; in.o_src = s->o_src; in.o_dst = s->o_dst;
        in.b_z = s->tri_z; in.b_w = s->lm_bw; in.o_z = s->lm_oz; in.o_om = s->lm_oom;
        in.bearing_var = er.bearing_var; in.odom_cov = er.odom_cov;
        prc = bos::dev::edge_check_enqueue(s->edge_check, in, kind, select, b.rows() || o.rows(), gate_bearing, gate_odom, s->stream,
                                           s->ev[4], &res, err);
    }
    if ((rc = c.drain(5, prc, err))) return rc;
    c.ms[4] = elapsed(s->ev[3], s->ev[4]);
    c.ms[5] = elapsed(s->ev[4], s->ev[5]);
    const auto t_dl = Clock::now();
    if (select[0] || select[1]) {   // both kinds' lists in one copy
        bos::dev::EdgeCheckLists L[2];
        HIP_TRY(hipMemcpy(L, res.lists, sizeof(L), hipMemcpyDeviceToHost));
        if (select[0]) b.take(&L[0], (size_t)k);
        if (select[1]) o.take(&L[1], (size_t)k);
    }
    if (kind[0] && (rc = b.download(res.b_neg, res.b_chi2, res.b_red))) return rc;
    if (kind[1] && (rc = o.download(res.o_neg, res.o_chi2, res.o_red))) return rc;
    c.host_ms(6, t_dl);
    return c.done();
}

int bos_edge_consistency_timing(const bos_solver* s, double ms[7], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->check_ms, 7, ms, bytes, bos::dev::edge_check_bytes(s->edge_check));
}

int bos_debug_selinv_fronts(bos_solver* s, int64_t capacity, int32_t* fronts, int32_t* nsuper, int32_t* node_front,
                            int32_t* edge_front) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (!uses_mf(s)) return fail(BOS_ERR_UNSUPPORTED, "multifrontal handles only");
    const bos::Multifrontal& F = s->plan.mf;
    if (nsuper) *nsuper = F.nsuper;
    if (!fronts && capacity == 0 && nsuper) return BOS_OK;
    if (!fronts || capacity < (int64_t)BOS_SELINV_COLS * F.nsuper)
        return fail(BOS_ERR_INVALID, "selinv fronts: capacity BOS_SELINV_COLS * supernodes");
    if (bos::dev::mf_selinv_report(s->mf, s->plan, fronts, node_front, edge_front))
        return fail(BOS_ERR_INVALID, "selinv fronts: no bos_marginals / bos_edge_covariances call has built the plan on this handle yet");
    return BOS_OK;
}

int bos_marginals(bos_solver* s, double* pose_cov, double* landmark_cov, int32_t* solver_info) {
    return covariance_pass(s, "bos_marginals", nullptr, pose_cov, landmark_cov, solver_info);
}

int bos_edge_covariances(bos_solver* s, double* bearing_cross, double* odom_cross, double* bearing_var, double* odom_cov,
                         double* pose_cov, double* landmark_cov, int32_t* solver_info) {
    double* const edge[4] = {bearing_cross, odom_cross, bearing_var, odom_cov};
    return covariance_pass(s, "bos_edge_covariances", edge, pose_cov, landmark_cov, solver_info);
}

int bos_edge_covariances_timing(const bos_solver* s, double ms[5], int64_t* edge_bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->edge_ms, 5, ms, edge_bytes, s->mf ? bos::dev::mf_edge_cov_bytes(s->mf) : 0);
}

int bos_marginals_timing(const bos_solver* s, double ms[4], int64_t* sigma_bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->marg_ms, 4, ms, sigma_bytes, s->mf ? bos::dev::mf_selinv_sigma_bytes(s->mf) : 0);
}

}  // extern "C"
