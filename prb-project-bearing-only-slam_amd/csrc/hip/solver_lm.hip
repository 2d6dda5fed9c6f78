// bos_cost / bos_optimize on the C ABI handle (solver_handle.hpp): Levenberg-Marquardt with on-device
// step control (hip/lm.hpp, host/lm_rule.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "solver_handle.hpp"

using namespace bos::capi;

namespace {

// word counts of the five state arrays the trial box-plus writes (d_pose, d_lm, d_pc, d_pth, d_lc)
void lm_state_words(const bos_solver* s, int64_t w[5]) {
    const int64_t tw = (int64_t)s->tsize / 4;
    w[0] = 6 * (int64_t)s->NP;
    w[1] = 4 * (int64_t)s->NL;
    w[2] = 4 * (int64_t)s->NP * tw;
    w[3] = (int64_t)s->NP * tw;
    w[4] = 2 * (int64_t)s->NL * tw;
}

// The feature's buffers, at its first use: the fp64 observations of the cost pass, the partials, the
// state backup, the control block and the trace in one allocation, and the control block's host-mapped
// copy. Built aside and moved into the handle on success: a failure leaves the handle as it was.
int lm_setup(bos_solver* s) {
    if (s->lm_arena) return BOS_OK;
    const bos::Plan& P = s->plan;
    int64_t w[5];
    lm_state_words(s, w);
    // the partials' room covers any later prior set (at most one prior per node)
    const size_t nc = (size_t)std::max(1, bos::dev::lm_cost_parts(s->Mb, s->Mo, (int64_t)s->NP + s->NL));
    const size_t nm = (size_t)std::max(1, bos::dev::lm_model_parts(P.n));
    bos::dev::Arena ar;
    ar.add(&s->lm_blm, s->bearing_lm);
    ar.add(&s->lm_lane_lm, P.blk.lm_lane_lm);
    ar.add(&s->lm_bw, s->h_bw);
    ar.add(&s->lm_oz, s->h_oz);
    ar.add(&s->lm_oom, s->h_oom);
    ar.zeros(&s->lm_pF, nc);
    ar.zeros(&s->lm_pchi, nc);
    ar.zeros(&s->lm_pnrob, nc);
    ar.zeros(&s->lm_pxx, nm);
    ar.zeros(&s->lm_pxb, nm);
    for (int a = 0; a < 5; ++a) ar.zeros(&s->lm_backup[a], (size_t)w[a]);
    ar.zeros(&s->lm_ctl, 1);
    ar.zeros(&s->lm_trace, (size_t)kLmTraceCap);
    bos::dev::DeviceMem mem;
    bos::dev::LmControl *hctl = nullptr, *mctl = nullptr;
    if (!mem.host_mapped(&hctl, &mctl)) return fail(BOS_ERR_DEVICE, "bos_optimize / bos_cost: host-mapped status allocation failed");
    if (!ar.commit(mem, &s->lm_arena))
        return fail(BOS_ERR_DEVICE, "bos_optimize / bos_cost: cannot allocate or upload " + std::to_string(ar.bytes()) + " bytes");
    s->lm_mem = std::move(mem);
    s->lm_hctl = hctl;
    s->lm_mctl = mctl;
    return BOS_OK;
}

// the objective's constant terms: the odometry self-loops (e = -z whatever the state), in fp64
void lm_loop_terms(const bos_solver* s, double& F, double& chi, int32_t& nrob) {
    F = chi = 0.0;
    nrob = 0;
    for (size_t i = 0; i < s->loop_z.size() / 3; ++i) {
        const double* z = &s->loop_z[3 * i];
        const double* u = &s->loop_om[6 * i];
        const double e0 = 0.0 - z[0], e1 = 0.0 - z[1];
        const double e2 = bos::normalized_angle<double>(bos::normalized_angle<double>(0.0) - z[2]);
        const double Oe0 = u[0] * e0 + u[1] * e1 + u[2] * e2;
        const double Oe1 = u[1] * e0 + u[3] * e1 + u[4] * e2;
        const double Oe2 = u[2] * e0 + u[4] * e1 + u[5] * e2;
        const double rho = e0 * Oe0 + e1 * Oe1 + e2 * Oe2;
        chi += rho;
        if (rho > s->kt) ++nrob;
        F += bos::lm_huber(rho, s->kt, rho > s->kt ? std::sqrt(s->kt * rho) : 0.0);
    }
}

// the fp64 cost pass at the master state (partials; the decision launch sums them)
int enqueue_lm_cost(bos_solver* s) {
    bos::dev::CostParams c;
    c.NP = s->NP; c.NL = s->NL; c.Mb = s->Mb; c.Mo = s->Mo;
    c.pose = s->d_pose; c.lm = s->d_lm;
    c.b_pose = s->tri_pose; c.b_lm = s->lm_blm; c.b_z = s->tri_z; c.b_w = s->lm_bw;
    c.o_src = s->o_src; c.o_dst = s->o_dst; c.o_z = s->lm_oz; c.o_om = s->lm_oom;
    c.n_pose_priors = s->n_pose_priors; c.n_lm_priors = s->n_lm_priors;
    c.pr_idx = s->pr_idx; c.pr_pose = s->pr_pose64; c.pr_lm = s->pr_lm64;
    c.kt = s->kt;
    c.part_F = s->lm_pF; c.part_chi = s->lm_pchi; c.part_nrob = s->lm_pnrob;
    c.n_parts = bos::dev::lm_cost_parts(s->Mb, s->Mo, n_priors(s));
    HIP_TRY(bos::dev::launch_lm_cost(c, s->stream));
    return BOS_OK;
}

int enqueue_lm_decide(bos_solver* s, int mode) {
    bos::dev::DecideParams d;
    d.part_F = s->lm_pF; d.part_chi = s->lm_pchi; d.part_nrob = s->lm_pnrob;
    d.n_cost = bos::dev::lm_cost_parts(s->Mb, s->Mo, n_priors(s));
    lm_loop_terms(s, d.F_const, d.chi_const, d.nrob_const);
    d.part_xx = s->lm_pxx; d.part_xb = s->lm_pxb;
    d.n_model = bos::dev::lm_model_parts(s->plan.n);
    d.max_part = s->d_maxpart;
    d.n_max = (s->NP + s->NL + bos::dev::kUpdateBlock - 1) / bos::dev::kUpdateBlock;
    d.info = mode == 0 && uses_mf(s) ? bos::dev::mf_info_ptr(s->mf) : nullptr;
    d.lambda_fp32 = s->precision == BOS_FP32 ? 1 : 0;
    d.ctl = s->lm_ctl;
    d.mirror = s->lm_mctl;
    d.trace = s->lm_trace;
    d.mode = mode;
    HIP_TRY(bos::dev::launch_lm_decide(d, s->stream));
    return BOS_OK;
}

bos::dev::CopySet lm_copy_set(const bos_solver* s, bool restore) {
    bos::dev::CopySet c;
    void* state[5] = {s->d_pose, s->d_lm, s->d_pc, s->d_pth, s->d_lc};
    lm_state_words(s, c.words);
    for (int a = 0; a < 5; ++a) {
        c.dst[a] = restore ? static_cast<uint32_t*>(state[a]) : s->lm_backup[a];
        c.src[a] = restore ? s->lm_backup[a] : static_cast<const uint32_t*>(state[a]);
        if (!c.dst[a] || !c.src[a]) c.words[a] = 0;
    }
    return c;
}

int launch_lm_iteration(bos_solver* s) {
    int rc;
    if (!s->lm_exec && !s->graph_failed && (rc = capture(s, -3, &s->lm_graph, &s->lm_exec))) return rc;
    if (s->lm_exec) HIP_TRY(hipGraphLaunch(s->lm_exec, s->stream));
    else if ((rc = enqueue_lm_iteration(s))) return rc;
    return BOS_OK;
}

}  // namespace

namespace bos {
namespace capi {

int lm_buffers_setup(bos_solver* s) { return lm_setup(s); }

// The device work of one LM iteration (multifrontal handles, one GPU): the undamped J+H, lambda from
// device memory onto its diagonal (the same launch backs the state up), the step's own solve, the
// model's predicted reduction, the trial box-plus, the fp64 cost of the trial state, the decision (host/lm_rule.hpp) and
// the rollback of a rejected trial. Every argument is fixed (the kernel threshold is baked in, as in
// the step's graphs): captured once and replayed.
int enqueue_lm_iteration(bos_solver* s) {
    int rc;
    const bos::Plan& P = s->plan;
    const bool f32 = s->precision == BOS_FP32;
    const int64_t nb = 3 * (int64_t)s->NP + 2 * (int64_t)s->NL;
    const int n_groups = (int)P.blk.lane_pose.size(), n_lanes = (int)P.blk.lm_lane_lm.size();
    const int32_t* lane_pose = s->lane_identity ? nullptr : s->lane_pose;
    if ((rc = enqueue_linearize(s, nullptr, true))) return rc;
    const bos::dev::CopySet backup = lm_copy_set(s, false);
    HIP_TRY(f32 ? bos::dev::launch_lm_damping<float>((float*)s->d_val, P.blk.size, P.blk.off_ldiag, lane_pose, n_groups, s->NP,
                                                     s->lm_lane_lm, n_lanes, s->NL, s->lm_ctl, backup, s->stream)
                : bos::dev::launch_lm_damping<double>((double*)s->d_val, P.blk.size, P.blk.off_ldiag, lane_pose, n_groups,
                                                      s->NP, s->lm_lane_lm, n_lanes, s->NL, s->lm_ctl, backup, s->stream));
    bool analysed_now = false;
    if ((rc = enqueue_solve(s, analysed_now))) return rc;
    HIP_TRY(f32 ? bos::dev::launch_lm_model<float>(s->d_rhs, (const float*)s->d_b, s->elim_ref, P.n, nb, s->lm_pxx, s->lm_pxb,
                                                   s->stream)
                : bos::dev::launch_lm_model<double>(s->d_rhs, (const double*)s->d_b, s->elim_ref, P.n, nb, s->lm_pxx,
                                                    s->lm_pxb, s->stream));
    if ((rc = enqueue_update(s)) || (rc = enqueue_lm_cost(s)) || (rc = enqueue_lm_decide(s, 0))) return rc;
    HIP_TRY(bos::dev::launch_lm_copy(lm_copy_set(s, true), s->lm_ctl, s->stream));
    return BOS_OK;
}

}  // namespace capi
}  // namespace bos

extern "C" {

void bos_lm_default_options(bos_lm_options* o) {
    if (o) bos::lm_default_options(*o);
}

int bos_cost(bos_solver* s, double* cost, double* chi2, int32_t* n_robust) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    int rc;
    if ((rc = require_one_gpu(s, "bos_cost", false, " (a rank's state is current on its own nodes only)"))) return rc;
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = lm_setup(s)) || (rc = enqueue_lm_cost(s)) || (rc = enqueue_lm_decide(s, 2))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    bos::dev::LmControl h;
    std::memcpy(&h, (const void*)s->lm_hctl, sizeof(h));
    if (cost) *cost = h.cost_eval;
    if (chi2) *chi2 = h.chi2;
    if (n_robust) *n_robust = h.n_robust;
    return BOS_OK;
}

int bos_time_cost(bos_solver* s, int32_t n, double* ms_per_pass) {
    if (!s || n <= 0 || !ms_per_pass) return fail(BOS_ERR_INVALID, "bad argument");
    int rc;
    if ((rc = require_one_gpu(s, "bos_time_cost", false))) return rc;
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = lm_setup(s))) return rc;
    return time_enqueues(s, n, [s] { return enqueue_lm_cost(s); }, ms_per_pass);
}

int bos_optimize(bos_solver* s, const bos_lm_options* options, bos_lm_result* result, bos_lm_iteration* trace,
                 int32_t trace_capacity) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    int rc;
    if ((rc = require_one_gpu(s, "bos_optimize", true))) return rc;
    bos_lm_options o;
    bos::lm_default_options(o);
    if (options) o = *options;
    if (o.max_iterations < 1 || o.max_iterations > kLmTraceCap) return fail(BOS_ERR_INVALID, "bos_optimize: max_iterations must be 1 .. 4096");
    if (o.check_every < 1) return fail(BOS_ERR_INVALID, "bos_optimize: check_every must be >= 1");
    if (!(o.lambda0 >= 0.0) || !(o.lambda_min > 0.0) || !(o.lambda_max >= o.lambda_min) || !(o.dx_tol >= 0.0) || !(o.f_tol >= 0.0))
        return fail(BOS_ERR_INVALID, "bos_optimize: bad lambda0 / lambda_min / lambda_max / dx_tol / f_tol");
    if (trace_capacity < 0 || (trace_capacity > 0 && !trace)) return fail(BOS_ERR_INVALID, "bos_optimize: trace_capacity without a trace");
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = lm_setup(s))) return rc;
    // bos_step returns on its status word, before the stream has drained
    HIP_TRY(hipStreamSynchronize(s->stream));
    bos::dev::LmControl h;
    std::memset(&h, 0, sizeof(h));
    h.opt = o;
    if (o.lambda0 > 0.0) {
        h.st.lambda = o.lambda0;
        h.st.nu = 2.0;
    } else {
        h.st.lambda = s->lm_started ? s->lm_lambda : s->damping;
        h.st.nu = s->lm_started ? s->lm_nu : 2.0;
    }
    h.trace_cap = kLmTraceCap;
    h.seq = s->lm_hctl->seq;
    HIP_TRY(hipMemcpy(s->lm_ctl, &h, sizeof(h), hipMemcpyHostToDevice));
    s->have_dx = false;   // d_rhs will hold the last trial's solution, accepted or not
    if ((rc = enqueue_lm_cost(s)) || (rc = enqueue_lm_decide(s, 1))) return rc;
    int enqueued = 0;
    while (enqueued < o.max_iterations) {
        const int batch = std::min<int>(o.check_every, o.max_iterations - enqueued);
        for (int i = 0; i < batch; ++i)
            if ((rc = launch_lm_iteration(s))) return rc;
        enqueued += batch;
        HIP_TRY(hipStreamSynchronize(s->stream));
        std::memcpy(&h, (const void*)s->lm_hctl, sizeof(h));
        if (h.st.done) break;
    }
    s->lm_started = true;
    s->lm_lambda = h.st.lambda;
    s->lm_nu = h.st.nu;
    if (result) {
        result->iterations = h.st.iteration;
        result->accepted = h.st.accepted;
        result->rejected = h.st.rejected;
        result->reason = h.st.reason;
        result->cost_initial = h.cost_start;
        result->cost_final = h.st.cost;
        result->lambda_final = h.st.lambda;
    }
    const int32_t nrec = std::min<int32_t>(h.st.iteration, trace_capacity);
    if (trace && nrec > 0) HIP_TRY(hipMemcpy(trace, s->lm_trace, (size_t)nrec * sizeof(bos_lm_iteration), hipMemcpyDeviceToHost));
    if (h.aborted)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out (state at the "
                                    "last accepted iterate)");
    return BOS_OK;
}

}  // extern "C"
