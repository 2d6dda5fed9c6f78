// The Gauss-Newton step on the C ABI handle (solver_handle.hpp) and the entry points that belong to it.
//
// One GN iteration (reference Solver::step, slam/solver.cpp:27-97):
//   1. linearize_kernel          J+H build into the block array of H and b (+ damping)
//   2. sparse Cholesky factorization + solve: the GPU supernodal multifrontal solver (default;
//      structure analysed once, like SimplicialLDLT::analyzePattern at solver.cpp:77-80), or
//      rocSOLVER csrrf / dense potrf-potrs on a gathered CSR copy
//   3. boxplus_kernel            left-multiplicative box-plus with dx = -x (state.cpp:69-80)
// The multi-rank forms of the step are in solver_shard.hip.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>

#include "solver_handle.hpp"

using namespace bos::capi;

namespace {

template <typename T> bos::dev::LinParams<T> lin_params(const bos_solver* s) {
    bos::dev::LinParams<T> p;
    p.pc = (const T*)s->d_pc;
    p.pth = (const T*)s->d_pth;
    p.lc = (const T*)s->d_lc;
    const bos::Plan& P = s->plan;
    p.NP = s->NP;
    p.lane_pose = s->lane_identity ? nullptr : s->lane_pose;
    p.n_groups = (int)P.blk.lane_pose.size();
    p.n_lm_lanes = (int)P.blk.lm_lane_lm.size();
    p.pose_blocks = s->pose_blocks;
    p.pose_b0 = (int)s->pose_b0;
    p.n_pose_run = (int)s->n_pose_run;
    p.lm_b0 = (int)s->lm_b0;
    p.n_lm_run = (int)s->n_lm_run;
    p.pw_base = s->pw_base; p.pw_stride = s->pw_stride; p.pl_cnt = s->pl_cnt;
    p.pb_idx = s->pb_idx; p.pb_z = (const T*)s->pb_z; p.pb_w = (const T*)s->pb_w;
    p.po_ptr = s->po_ptr; p.po_ent = s->po_ent; p.po_oth = s->po_oth; p.po_blk = s->po_blk;
    p.o_src = s->o_src; p.o_dst = s->o_dst; p.o_z = (const T*)s->o_z; p.o_om = (const T*)s->o_om;
    p.om_stride = s->om_stride;
    p.lw_base = s->lw_base; p.lw_stride = s->lw_stride; p.ll_cnt = s->ll_cnt; p.ll_lm = s->ll_lm;
    p.lb_idx = s->lb_idx; p.lb_z = (const T*)s->lb_z; p.lb_w = (const T*)s->lb_w; p.ll_run = s->ll_run;
    p.ll_hdr = reinterpret_cast<const int2*>(s->ll_hdr);
    p.hval = (T*)s->d_val;
    p.b = (T*)s->d_b;
    p.off_ldiag = (int)P.blk.off_ldiag; p.off_pl = (int)P.blk.off_pl; p.off_pp = (int)P.blk.off_pp;
    p.chi2_part = s->d_chi_part;
    p.nrob_part = s->d_nrob_part;
    p.pl_factored = s->pl_factored ? 1 : 0;
    p.kt = (T)s->kt;
    p.lambda = (T)s->damping;
    p.diag_stamps = nullptr;
    p.t_start = nullptr;
    return p;
}

// the J+H launch: t_start the step's stamp slot, diag_stamps the per-wave timeline (or null)
hipError_t launch_jh(bos_solver* s, unsigned long long* t_start, bool undamped, unsigned long long* diag_stamps) {
    const int lpp = s->plan.blk.lpp;
    if (s->precision == BOS_FP32) {
        bos::dev::LinParams<float> p = lin_params<float>(s);
        p.t_start = t_start;
        p.diag_stamps = diag_stamps;
        if (undamped) p.lambda = 0.f;
        return bos::dev::launch_linearize<float>(p, lpp, s->has_w, s->has_dups, s->stream);
    }
    bos::dev::LinParams<double> p = lin_params<double>(s);
    p.t_start = t_start;
    p.diag_stamps = diag_stamps;
    if (undamped) p.lambda = 0.0;
    return bos::dev::launch_linearize<double>(p, lpp, s->has_w, s->has_dups, s->stream);
}

template <typename T> bos::dev::PriorParams<T> prior_params(const bos_solver* s) {
    bos::dev::PriorParams<T> p;
    p.n_pose = s->n_pose_priors; p.n_lm = s->n_lm_priors;
    p.idx = s->pr_idx; p.pose_rec = (const T*)s->pr_pose; p.lm_rec = (const T*)s->pr_lm;
    p.pc = (const T*)s->d_pc; p.pth = (const T*)s->d_pth; p.lc = (const T*)s->d_lc;
    p.NP = s->NP; p.NL = s->NL;
    p.hval = (T*)s->d_val; p.b = (T*)s->d_b;
    p.off_ldiag = s->plan.blk.off_ldiag; p.nval = s->plan.blk.size;
    p.part = s->pr_part;
    return p;
}

template <typename T> bos::dev::UpdateParams<T> upd_params(const bos_solver* s) {
    bos::dev::UpdateParams<T> u;
    u.NP = s->NP; u.NL = s->NL; u.fixed = s->plan.fixed;
    u.node_dof = s->node_dof;
    u.x = s->d_rhs;
    u.pose = s->d_pose; u.lm = s->d_lm;
    u.pc = (T*)s->d_pc; u.pth = (T*)s->d_pth; u.lc = (T*)s->d_lc;
    u.max_part = s->d_maxpart;
    // sharded: the abort bits of every rank's exchange-2 header (the local word was moved into it)
    // (sharded: the local word is zeroed by exchange 2's packing; it can then only carry the abort bit
    // of a direct-exchange wait that timed out)
    u.info = uses_mf(s) ? bos::dev::mf_info_ptr(s->mf) : nullptr;
    u.ex_hdr = s->sharded ? s->ex2_recv + 1 : nullptr;
    u.ex_stride = s->ex2_count;
    u.ex_world = s->world;
    u.nodes = s->sharded ? s->upd_nodes : nullptr;
    u.n_nodes = s->n_upd;
    u.t_start = nullptr;
    return u;
}

// chi^2 and robust count of the odometry self-loops: constant (e = -z whatever the state, their
// Jacobian is zero, see host/plan.cpp build_layout), evaluated in T like the kernel. No J+H lane
// counts them, so every rank adds them once to the step's combined (summed over ranks) chi^2.
template <typename T> void self_loop_terms(const bos_solver* s, double& chi, int32_t& nrob) {
    chi = 0.0;
    nrob = 0;
    const T kt = (T)s->kt;
    for (size_t i = 0; i < s->loop_z.size() / 3; ++i) {
        T z[3], u[6];
        for (int v = 0; v < 3; ++v) z[v] = (T)s->loop_z[3 * i + v];
        for (int v = 0; v < 6; ++v) u[v] = (T)s->loop_om[6 * i + v];
        const T e0 = (T)0 - z[0], e1 = (T)0 - z[1];
        const T e2 = bos::normalized_angle<T>(bos::normalized_angle<T>((T)0) - z[2]);
        const T Oe0 = u[0] * e0 + u[1] * e1 + u[2] * e2;
        const T Oe1 = u[1] * e0 + u[3] * e1 + u[4] * e2;
        const T Oe2 = u[2] * e0 + u[4] * e1 + u[5] * e2;
        const T rho = e0 * Oe0 + e1 * Oe1 + e2 * Oe2;
        chi += (double)rho;
        if (rho > kt) ++nrob;
    }
}

int enqueue_stats(bos_solver* s, bool with_update) {
    int32_t* info = uses_mf(s) ? bos::dev::mf_info_ptr(s->mf) : (s->solver_kind == BOS_SOLVER_DENSE_CHOL ? s->d_info : nullptr);
    const int nupd = (s->NP + s->NL + bos::dev::kUpdateBlock - 1) / bos::dev::kUpdateBlock;
    int32_t nrob_c = 0;
    const double chi_c = self_loop_chi(s, nrob_c);
    // observations partition: the all-reduced header [chi^2, robust count] instead of the partials
    HIP_TRY(bos::dev::launch_reduce_stats(s->obs ? s->ex1_recv : s->d_chi_part, s->obs ? nullptr : s->d_nrob_part,
                                          s->chi_parts, chi_c, nrob_c, with_update ? s->d_maxpart : nullptr, nupd, info,
                                          s->d_status, s->m_status, s->stream, n_priors(s) ? s->pr_part : nullptr,
                                          bos::dev::prior_parts(n_priors(s))));
    return BOS_OK;
}

// State caches in T precision (x, y, cos, sin per pose; theta; landmark x, y) computed on the host
// from the master state with the host libm, exactly as the CPU oracle evaluates them, so that
// iteration 0 is bit-reproducible against it (see host/det_atan2.hpp); the box-plus kernel keeps
// them current afterwards.
template <typename T> int upload_cache_T(bos_solver* s) {
    const int NP = s->NP, NL = s->NL;
    std::vector<double> pose(3 * (size_t)NP), lm(2 * (size_t)NL);
    HIP_TRY(hipMemcpy(pose.data(), s->d_pose, pose.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (NL) HIP_TRY(hipMemcpy(lm.data(), s->d_lm, lm.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<T> pc(4 * (size_t)NP), pth(NP), lc(2 * (size_t)NL);
    for (int i = 0; i < NP; ++i) {
        const T th = (T)pose[3 * (size_t)i + 2];
        pc[4 * (size_t)i] = (T)pose[3 * (size_t)i];
        pc[4 * (size_t)i + 1] = (T)pose[3 * (size_t)i + 1];
        pc[4 * (size_t)i + 2] = std::cos(th);
        pc[4 * (size_t)i + 3] = std::sin(th);
        pth[i] = th;
    }
    for (size_t j = 0; j < lc.size(); ++j) lc[j] = (T)lm[j];
    HIP_TRY(hipMemcpy(s->d_pc, pc.data(), pc.size() * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_pth, pth.data(), pth.size() * sizeof(T), hipMemcpyHostToDevice));
    if (NL) HIP_TRY(hipMemcpy(s->d_lc, lc.data(), lc.size() * sizeof(T), hipMemcpyHostToDevice));
    return BOS_OK;
}

template <typename T> bos::dev::TriParams<T> tri_params(const bos_solver* s) {
    bos::dev::TriParams<T> p;
    p.NL = s->NL;
    p.lm_ptr = s->tri_ptr; p.lm_obs = s->tri_obs; p.b_pose = s->tri_pose; p.b_z = s->tri_z;
    p.pose = s->d_pose; p.scratch = s->tri_scr; p.lm = s->d_lm; p.lc = (T*)s->d_lc;
    return p;
}

// The step status (one copy). The sticky abort flag is cleared here once reported, so every
// bos_step / bos_step_n batch starts with it clear.
// Waits for the status of the last enqueued step. One GPU: the host polls the sequence number the
// step's last kernel writes to the host-mapped mirror after the summary (a system-scope release in
// between), which it sees ~10 us before a stream synchronisation returns (tools/sync_step_trace.py);
// the stream is not synchronised (every later call that reads device memory synchronises it, and
// launches are stream ordered). A fault or an unexpected state falls back to the stream wait.
int wait_status(bos_solver* s, bool sync) {
    if (!sync && s->seq_pending > 0) {
        const int32_t target = s->seq_seen + s->seq_pending;
        s->seq_seen = target;
        s->seq_pending = 0;
        const volatile int32_t* q = &s->h_status->seq;
        for (uint64_t it = 1;; ++it) {
            if (*q == target) {
                std::atomic_thread_fence(std::memory_order_acquire);
                return BOS_OK;
            }
            if ((it & 4095) == 0) {   // the stream done (or failed) without the number: report it
                const hipError_t e = hipStreamQuery(s->stream);
                if (e != hipErrorNotReady) {
                    if (*q == target) break;
                    s->seq_seen = *q;   // what the device actually wrote: the next step waits for its own number
                    if (e != hipSuccess) HIP_TRY(e);
                    return fail(BOS_ERR_DEVICE, "step status sequence number not written");
                }
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return BOS_OK;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->seq_seen = s->h_status->seq;   // the device counter, whatever ran
    s->seq_pending = 0;
    return BOS_OK;
}

int enqueue_step(bos_solver* s) {
    int rc;
    if ((rc = enqueue_linearize(s, s->d_status->stamp))) return rc;
    return enqueue_step_tail(s);
}

// The launches of one one-GPU GN iteration (see do_step)
int launch_step(bos_solver* s, bool sync) {
    int rc;
    if (uses_mf(s) && !s->graph_exec && !s->graph_failed && (rc = capture(s, -1, &s->graph, &s->graph_exec))) return rc;
    if (uses_mf(s) && !s->exec_full && !s->graph_failed && (rc = capture(s, -2, &s->graph_full, &s->exec_full)))
        return rc;   // both graphs at the first step, so neither kind of call pays a capture later
    if (!sync && s->exec_full) {
        // a batch's step before its last: the host is ahead of the device, one graph per step
        HIP_TRY(hipGraphLaunch(s->exec_full, s->stream));
    } else if (s->graph_exec) {
        // synchronous: the J+H build launched directly (it starts a few us after the call), the
        // rest of the step as the graph, submitted while the build runs (a graph's first kernel
        // starts 13-25 us after hipGraphLaunch, tools/sync_step_trace.py; launching the input
        // gather directly too measured slower: 1 760 against 1 790 it/s)
        if ((rc = enqueue_linearize(s, s->d_status->stamp))) return rc;
        HIP_TRY(hipGraphLaunch(s->graph_exec, s->stream));
    } else if ((rc = enqueue_step(s))) {
        return rc;
    }
    return BOS_OK;
}

// One GN iteration. sync: read the status back (the last step of a bos_step_n batch). A
// factorization whose dataflow launch timed out leaves the state untouched (the box-plus kernel
// checks the solver word) and fails the call.
int do_step(bos_solver* s, bos_step_stats* st, bool sync) {
    if (s->sharded) return do_step_sharded(s, st, sync);
    int rc;
    if (s->obs) {
        if (!s->comm) return fail(BOS_ERR_INVALID, "observations-partition handle without a communicator: drive bos_step_phase");
        if ((rc = launch_rccl_step(s, sync))) return rc;
    } else if ((rc = launch_step(s, sync))) {
        return rc;
    } else {
        ++s->seq_pending;   // the step's status launch (now enqueued) bumps the device counter once
    }
    s->have_dx = true;
    return sync ? finish_step(s, st) : BOS_OK;
}

// 512 MiB read (2x the Infinity Cache) from one of two buffers, alternately: afterwards L2 and the
// Infinity Cache hold none of the build's inputs, and no scrub finds the previous scrub's lines there
// (so the time of a scrub does not depend on what ran before it)
int scrub_caches(bos_solver* s) {
    constexpr int64_t kScrub = (int64_t)1 << 26;   // doubles per buffer
    if (!s->scrub && !s->mem.alloc(&s->scrub, 2 * kScrub + 1, true)) return fail(BOS_ERR_DEVICE, "cache scrub: device allocation failed");
    const double* buf = s->scrub + (s->scrub_turn++ & 1) * kScrub;
    HIP_TRY(bos::dev::launch_cache_scrub(buf, kScrub, s->scrub + 2 * kScrub, s->stream));
    return BOS_OK;
}

}  // namespace

namespace bos {
namespace capi {

int require_one_gpu(const bos_solver* s, const char* name, bool need_mf, const char* why) {
    if (need_mf && !uses_mf(s))
        return fail(BOS_ERR_UNSUPPORTED, std::string(name) + " needs a multifrontal solver (BOS_SOLVER_SCHUR or BOS_SOLVER_SUPERNODAL)");
    if (s->sharded || s->obs || s->world > 1 || s->comm || s->external || s->p2p)
        return fail(BOS_ERR_UNSUPPORTED, std::string(name) + " on a sharded handle" + why);
    return BOS_OK;
}

// undamped: lambda 0 in the launch arguments (an LM iteration adds its own from device memory)
int enqueue_linearize(bos_solver* s, unsigned long long* t_start, bool undamped) {
    const hipError_t e = launch_jh(s, t_start, undamped, nullptr);
    if (e != hipSuccess) return fail(BOS_ERR_DEVICE, std::string("linearize launch: ") + hipGetErrorString(e));
    // the priors (bos_set_priors) onto the diagonal blocks and b the build has just written: every
    // consumer of H comes through here. A handle without priors launches nothing more.
    if (n_priors(s)) {
        const hipError_t ep = s->precision == BOS_FP32 ? bos::dev::launch_priors<float>(prior_params<float>(s), s->stream)
                                                       : bos::dev::launch_priors<double>(prior_params<double>(s), s->stream);
        if (ep != hipSuccess) return fail(BOS_ERR_DEVICE, std::string("prior launch: ") + hipGetErrorString(ep));
    }
    return BOS_OK;
}

double self_loop_chi(const bos_solver* s, int32_t& nrob) {
    double c = 0.0;
    if (s->precision == BOS_FP32) self_loop_terms<float>(s, c, nrob);
    else self_loop_terms<double>(s, c, nrob);
    return c;
}

// right-hand side in elimination order, and the fp64 copy of an fp32 block array. The gather also
// stamps the solve's start and opens the step's flow epoch (the first solver launch of a GN step).
int enqueue_solver_inputs(bos_solver* s) {
    const int64_t n = s->plan.n;
    const bool f32 = s->precision == BOS_FP32;
    unsigned long long* stamp = s->d_status->stamp + s->solve_stamp;
    uint32_t* epoch = uses_mf(s) ? bos::dev::mf_epoch_ptr(s->mf) : nullptr;
    const bool conv = f32 && uses_mf(s);   // the fp64 copy of the block array, in the same launch
    if (s->fold32) {   // the copy skips what the folds read from the fp32 array
        HIP_TRY(bos::dev::launch_gather_f64_ranges((const float*)s->sys_b, s->elim_ref, s->d_rhs, n, s->stream, stamp,
                                                   epoch, (const float*)s->sys_val, s->d_val64, s->plan.blk.size,
                                                   s->plan.blk.off_ldiag, s->plan.blk.off_pp));
        return BOS_OK;
    }
    if (s->pl_factored) {   // the copy expands the factored pose-landmark blocks
        HIP_TRY(bos::dev::launch_gather_f64_factored((const float*)s->sys_b, s->elim_ref, s->d_rhs, n, s->stream, stamp,
                                                     epoch, (const float*)s->sys_val, s->d_val64, s->plan.blk.size,
                                                     s->plan.blk.off_pl, s->plan.blk.pose_lanes.slots()));
        return BOS_OK;
    }
    HIP_TRY(f32 ? bos::dev::launch_gather_f64<float>((const float*)s->sys_b, s->elim_ref, s->d_rhs, n, s->stream, stamp, epoch,
                                                     conv ? (const float*)s->sys_val : nullptr, conv ? s->d_val64 : nullptr,
                                                     conv ? s->plan.blk.size : 0)
                : bos::dev::launch_gather_f64<double>((const double*)s->sys_b, s->elim_ref, s->d_rhs, n, s->stream, stamp, epoch));
    return BOS_OK;
}

int enqueue_solve(bos_solver* s, bool& ran_analysis) {
    const int64_t n = s->plan.n;
    ran_analysis = false;
    if (n == 0) return BOS_OK;
    const bool f32 = s->precision == BOS_FP32;
    int rc;
    if ((rc = enqueue_solver_inputs(s))) return rc;
    const rocblas_int nn = (rocblas_int)n;
    if (uses_mf(s)) {   // reads the block array through its assembly map
        HIP_TRY(bos::dev::mf_factor(s->mf, 0, mf_matrix(s), s->d_rhs, s->stream));
        HIP_TRY(bos::dev::mf_solve(s->mf, 0, s->d_rhs, s->stream));
        return BOS_OK;
    }
    double* A = s->d_csr64;
    HIP_TRY(f32 ? bos::dev::launch_gather_f64<float>((const float*)s->sys_val, s->csr_src, A, s->plan.nnzA(), s->stream)
                : bos::dev::launch_gather_f64<double>((const double*)s->sys_val, s->csr_src, A, s->plan.nnzA(), s->stream));
    if (s->solver_kind == BOS_SOLVER_DENSE_CHOL) {
        HIP_TRY(hipMemsetAsync(s->d_dense, 0, (size_t)n * n * sizeof(double), s->stream));
        HIP_TRY(bos::dev::launch_scatter_dense(s->d_rowptr, s->d_colind, A, nn, s->d_dense, s->stream));
        RB_TRY(rocsolver_dpotrf(s->rb, rocblas_fill_lower, nn, s->d_dense, nn, s->d_info));
        RB_TRY(rocsolver_dpotrs(s->rb, rocblas_fill_lower, nn, 1, s->d_dense, nn, s->d_rhs, nn));
        return BOS_OK;
    }
    const rocblas_int nnzA = (rocblas_int)s->plan.nnzA(), nnzT = (rocblas_int)s->plan.nnzL();
    if (!s->analyzed) {
        RB_TRY(rocsolver_dcsrrf_analysis(s->rb, nn, 1, nnzA, s->d_rowptr, s->d_colind, A, nnzT, s->d_Lptr, s->d_Lind,
                                         s->d_Lval, nullptr, s->d_pivQ, s->d_rhs, nn, s->rf));
        s->analyzed = true;
        ran_analysis = true;
    }
    RB_TRY(rocsolver_dcsrrf_refactchol(s->rb, nn, nnzA, s->d_rowptr, s->d_colind, A, nnzT, s->d_Lptr, s->d_Lind,
                                       s->d_Lval, s->d_pivQ, s->rf));
    RB_TRY(rocsolver_dcsrrf_solve(s->rb, nn, 1, nnzT, s->d_Lptr, s->d_Lind, s->d_Lval, nullptr, s->d_pivQ, s->d_rhs,
                                  nn, s->rf));
    return BOS_OK;
}

int enqueue_update(bos_solver* s) {
    hipError_t e;
    if (s->precision == BOS_FP32) {
        bos::dev::UpdateParams<float> u = upd_params<float>(s);
        u.t_start = s->d_status->stamp + 2;
        e = bos::dev::launch_boxplus<float>(u, s->stream);
    } else {
        bos::dev::UpdateParams<double> u = upd_params<double>(s);
        u.t_start = s->d_status->stamp + 2;
        e = bos::dev::launch_boxplus<double>(u, s->stream);
    }
    if (e != hipSuccess) return fail(BOS_ERR_DEVICE, std::string("boxplus launch: ") + hipGetErrorString(e));
    return BOS_OK;
}

int upload_cache(bos_solver* s) { return s->precision == BOS_FP32 ? upload_cache_T<float>(s) : upload_cache_T<double>(s); }

int enqueue_triangulate(bos_solver* s) {
    const hipError_t e = s->precision == BOS_FP32 ? bos::dev::launch_triangulate<float>(tri_params<float>(s), s->stream)
                                                  : bos::dev::launch_triangulate<double>(tri_params<double>(s), s->stream);
    if (e != hipSuccess) return fail(BOS_ERR_DEVICE, std::string("triangulate launch: ") + hipGetErrorString(e));
    return BOS_OK;
}

// sync: wait for the stream (callers that read events or device memory next), not only the status
int read_stats(bos_solver* s, bos_step_stats* st, int32_t* aborted, bool sync) {
    int rc;
    if ((rc = wait_status(s, sync))) return rc;
    bos::dev::StepStatus h;
    std::memcpy(&h, (const void*)s->h_status, sizeof(h));   // written by the step's last kernel
    if (h.aborted) {
        HIP_TRY(hipMemsetAsync(&s->d_status->aborted, 0, sizeof(int32_t), s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    if (st) {
        std::memset(st, 0, sizeof(*st));
        st->chi2 = h.chi2;
        st->n_robust = h.n_robust;
        st->solver_info = h.info & ~bos::dev::kStepAbort;
        st->max_abs_dx = h.max_dx;
        if (!s->sharded) {   // phase boundaries stamped by the step's kernels
            auto d = [](unsigned long long a, unsigned long long b) { return b > a ? (double)(b - a) * bos::dev::kStampMs : 0.0; };
            st->t_linearize_ms = d(h.stamp[0], h.stamp[1]);
            // observations partition: J+H end [1], the all-reduce, solve start [4]
            st->t_exchange_ms = s->obs ? d(h.stamp[1], h.stamp[4]) : 0.0;
            st->t_solve_ms = d(h.stamp[s->solve_stamp], h.stamp[2]);
            st->t_update_ms = d(h.stamp[2], h.stamp[3]);
        }
    }
    if (aborted) *aborted = h.aborted;
    return BOS_OK;
}

// The device work of one GN iteration on one GPU: J+H (stamp 0 at its start), solve (its first
// launch stamps 1 and opens the flows' epoch), box-plus (stamp 2), status (stamp 3 at its end, then
// the host-mapped copy). No events, no marker launches, no host synchronisation: the sequence after
// the J+H build is captured once into a hipGraph and replayed (do_step).
// reads the status of the step just enqueued (sharded: phases 0-2 and their times), fails an aborted one
int finish_step(bos_solver* s, bos_step_stats* st) {
    int rc;
    int32_t aborted = 0;
    if ((rc = read_stats(s, st, &aborted))) return rc;
    if (aborted) {
        s->have_dx = false;
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out (state "
                                    "left unchanged by the failed iteration)");
    }
    if (st && s->sharded) {   // phase boundaries stamped by the phases' kernels (StepStatus::stamp)
        bos::dev::StepStatus h;
        std::memcpy(&h, (const void*)s->h_status, sizeof(h));
        auto d = [](unsigned long long a, unsigned long long b) { return b > a ? (double)(b - a) * bos::dev::kStampMs : 0.0; };
        st->t_linearize_ms = d(h.stamp[0], h.stamp[1]);
        st->t_solve_ms = d(h.stamp[1], h.stamp[4]) + d(h.stamp[5], h.stamp[6]);
        st->t_exchange_ms = d(h.stamp[4], h.stamp[5]) + d(h.stamp[6], h.stamp[7]);
        st->t_update_ms = d(h.stamp[7], h.stamp[3]);
    }
    return BOS_OK;
}

// the step after the J+H build (the captured graph: see do_step)
int enqueue_step_tail(bos_solver* s) {
    int rc;
    bool analysed_now = false;
    if ((rc = enqueue_solve(s, analysed_now))) return rc;
    if ((rc = enqueue_update(s))) return rc;
    return enqueue_stats(s, true);
}

void drop_graph(bos_solver* s) {
    // bos_step returns on the status sequence number, before the stream has drained: a graph may
    // still be running
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    auto drop = [](hipGraph_t& g, hipGraphExec_t& e) {
        if (e) (void)hipGraphExecDestroy(e);
        if (g) (void)hipGraphDestroy(g);
        e = nullptr;
        g = nullptr;
    };
    drop(s->graph, s->graph_exec);
    drop(s->graph_full, s->exec_full);
    for (int i = 0; i < 3; ++i) drop(s->pgraph[i], s->pexec[i]);
    drop(s->sgraph, s->sexec);
    drop(s->stail, s->stail_exec);
    drop(s->lm_graph, s->lm_exec);
}

// Capture the launches of one GN step (phase -1: the one-GPU step after its J+H build,
// enqueue_step_tail; -2: the whole one-GPU step; -3: one LM iteration, enqueue_lm_iteration; 0-2: a subtree-sharded phase; 10-11: an
// observations-partition phase) into *exec (multifrontal
// solvers: rocSOLVER's paths are not captured). A stream that cannot be captured leaves
// graph_failed set and the launches run eagerly, the same ones in the same order.
int capture(bos_solver* s, int phase, hipGraph_t* graph, hipGraphExec_t* exec) {
    if (hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        s->graph_failed = true;
        return BOS_OK;
    }
    const int rc = phase == -1   ? enqueue_step_tail(s)
                   : phase == -2 ? enqueue_step(s)
                   : phase == -3 ? enqueue_lm_iteration(s)
                   : phase >= 10 ? obs_enqueue(s, phase - 10)
                                 : shard_enqueue(s, phase);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s->stream, &g);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) return fail(BOS_ERR_DEVICE, std::string("step graph capture: ") + hipGetErrorString(e));
    *graph = g;
    HIP_TRY(hipGraphInstantiate(exec, g, nullptr, nullptr, 0));
    return BOS_OK;
}

}  // namespace capi
}  // namespace bos

extern "C" {

int bos_abi_version(void) { return BOS_ABI_VERSION; }

int bos_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bos_device_peer_access(int32_t capacity, int32_t* out, int32_t* n_out) {
    if (!out || !n_out || capacity < 0) return fail(BOS_ERR_INVALID, "bad argument");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess) {
        (void)hipGetLastError();
        nd = 0;
    }
    const int n = std::min<int>(nd, capacity);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            int ok = i == j;
            if (i != j && hipDeviceCanAccessPeer(&ok, i, j) != hipSuccess) {
                (void)hipGetLastError();
                ok = 0;
            }
            out[(int64_t)i * n + j] = ok ? 1 : 0;
        }
    *n_out = n;
    return BOS_OK;
}

int bos_set_kernel_threshold(bos_solver* s, double kt) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (kt != s->kt) drop_graph(s);
    s->kt = kt;
    return BOS_OK;
}

int bos_set_damping_factor(bos_solver* s, double df) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (df != s->damping) drop_graph(s);
    s->damping = df;
    return BOS_OK;
}

int bos_step(bos_solver* s, bos_step_stats* st) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(s->device));
    return do_step(s, st, true);
}

int bos_step_n(bos_solver* s, int n, bos_step_stats* last) {
    if (!s || n < 0) return fail(BOS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    for (int i = 0; i < n; ++i) {
        int rc = do_step(s, last, i + 1 == n);
        if (rc) return rc;
    }
    return BOS_OK;
}

int bos_linearize_async(bos_solver* s) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    return enqueue_linearize(s);
}

int bos_debug_linearize_timeline(bos_solver* s, int64_t capacity, uint64_t* stamps, int64_t* n_waves, int32_t flush_caches) {
    if (!s || !n_waves) return fail(BOS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    const bos::Plan& P = s->plan;
    const int64_t grid = s->pose_blocks + ((int64_t)P.blk.lm_lane_lm.size() + bos::dev::kBlock - 1) / bos::dev::kBlock;
    const int64_t waves = grid * (bos::dev::kBlock / 64);
    *n_waves = waves;
    if (!stamps || capacity < waves) return BOS_OK;
    bos::dev::DeviceMem tmp;   // the stamps, freed on every return
    unsigned long long* d = nullptr;
    if (!tmp.alloc(&d, 8 * (size_t)waves, false)) return fail(BOS_ERR_DEVICE, "timeline: device allocation failed");
    HIP_TRY(hipMemsetAsync(d, 0, 8 * (size_t)waves * sizeof(unsigned long long), s->stream));
    int rc;
    if (flush_caches && (rc = scrub_caches(s))) return rc;
    hipError_t e = launch_jh(s, nullptr, false, d);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipMemcpy(stamps, d, 8 * (size_t)waves * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(BOS_ERR_DEVICE, std::string("timeline: ") + hipGetErrorString(e));
    return BOS_OK;
}

int bos_time_linearize(bos_solver* s, int32_t n, int32_t flush_caches, double* ms_per_build) {
    if (!s || n <= 0 || !ms_per_build) return fail(BOS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    // back to back: the block array and lists stay in L2 / Infinity Cache
    if (!flush_caches) return time_enqueues(s, n, [s] { return enqueue_linearize(s); }, ms_per_build);
    // cold: before every build, 512 MiB are read (scrub_caches) so the build's inputs come from HBM,
    // as inside a GN step where the solver streams its factor between two builds; each build is
    // bracketed by its own events (their cost included: conservative)
    double total = 0.0;
    for (int i = 0; i < n; ++i) {
        if ((rc = scrub_caches(s))) return rc;
        HIP_TRY(hipEventRecord(s->ev[0], s->stream));
        if ((rc = enqueue_linearize(s))) return rc;
        HIP_TRY(hipEventRecord(s->ev[1], s->stream));
        HIP_TRY(hipEventSynchronize(s->ev[1]));
        total += elapsed(s->ev[0], s->ev[1]);
    }
    *ms_per_build = total / n;
    return BOS_OK;
}

int bos_time_triangulate(bos_solver* s, int32_t n, double* ms_per_call) {
    if (!s || n <= 0 || !ms_per_call) return fail(BOS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    s->have_dx = false;
    return time_enqueues(s, n, [s] { return enqueue_triangulate(s); }, ms_per_call);
}

int bos_time_steps(bos_solver* s, int32_t n, double* ms_per_step) {
    if (!s || n <= 0 || !ms_per_step) return fail(BOS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    bos_step_stats st;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) {   // exactly bos_step: launch, wait, status read and checked
        const int rc = do_step(s, &st, true);
        if (rc) return rc;
    }
    const auto t1 = std::chrono::steady_clock::now();
    *ms_per_step = std::chrono::duration<double, std::milli>(t1 - t0).count() / n;
    return BOS_OK;
}

int bos_debug_inject_stall(bos_solver* s) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (!uses_mf(s)) return fail(BOS_ERR_UNSUPPORTED, "no dataflow launch in this solver");
    HIP_TRY(hipSetDevice(s->device));
    const hipError_t e = bos::dev::mf_debug_skip_next_front(s->mf, s->stream);
    if (e == hipErrorInvalidValue)
        return fail(BOS_ERR_UNSUPPORTED, "no dataflow launch in this plan whose first front another front of it waits for");
    HIP_TRY(e);
    return BOS_OK;
}

int bos_debug_solver_stamps(bos_solver* s, int64_t capacity, uint64_t* stamps, int32_t* meta) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (!uses_mf(s) || s->sharded || s->obs) return fail(BOS_ERR_UNSUPPORTED, "one-GPU multifrontal handles only");
    const bos::Multifrontal& F = s->plan.mf;
    const int64_t need = 16 * (int64_t)F.nsuper;
    if (!stamps || !meta || capacity < need) return fail(BOS_ERR_INVALID, "stamps: capacity 16 * supernodes");
    HIP_TRY(hipSetDevice(s->device));
    bos::dev::DeviceMem tmp;   // the stamps, freed on every return
    unsigned long long* d = nullptr;
    if (!tmp.alloc(&d, (size_t)need, true)) return fail(BOS_ERR_DEVICE, "stamps: device allocation failed");
    int rc;
    drop_graph(s);
    const bool gf = s->graph_failed;
    s->graph_failed = true;   // one eager step with the stamps
    bos::dev::mf_debug_set_stamps(s->mf, d);
    rc = do_step(s, nullptr, true);
    if (!rc && hipStreamSynchronize(s->stream) != hipSuccess) rc = fail(BOS_ERR_DEVICE, "stamps step");
    bos::dev::mf_debug_set_stamps(s->mf, nullptr);
    s->graph_failed = gf;
    if (!rc && hipMemcpy(stamps, d, need * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(BOS_ERR_DEVICE, "stamps copy");
    if (rc) return rc;
    std::vector<int32_t> lev(F.nsuper, -1);
    for (int l = 0; l < F.nlevels; ++l)
        for (int q = F.level_ptr[l]; q < F.level_ptr[l + 1]; ++q) lev[F.level[q]] = l;
    for (int x = 0; x < F.nsuper; ++x) {
        meta[4 * x] = lev[x];
        meta[4 * x + 1] = F.k[x];
        meta[4 * x + 2] = F.r[x];
        meta[4 * x + 3] = F.fold_cnt.empty() ? 0 : F.fold_cnt[x];
    }
    return BOS_OK;
}

int bos_debug_solver_routes(bos_solver* s, int64_t capacity, int32_t* routes, int32_t* nsuper) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (!uses_mf(s)) return fail(BOS_ERR_UNSUPPORTED, "multifrontal handles only");
    const bos::Multifrontal& F = s->plan.mf;
    if (nsuper) *nsuper = F.nsuper;
    if (!routes && capacity == 0 && nsuper) return BOS_OK;
    if (!routes || capacity < 4 * (int64_t)F.nsuper) return fail(BOS_ERR_INVALID, "routes: capacity 4 * supernodes");
    std::vector<int8_t> rf(F.nsuper), rb(F.nsuper);
    if (bos::dev::mf_debug_routes(s->mf, rf.data(), rb.data()))
        return fail(BOS_ERR_INVALID, "routes: no step has been enqueued on this handle yet");
    for (int x = 0; x < F.nsuper; ++x) {
        routes[4 * x] = rf[x];
        routes[4 * x + 1] = rb[x];
        routes[4 * x + 2] = F.k[x];
        routes[4 * x + 3] = F.r[x];
    }
    return BOS_OK;
}

int bos_debug_set_step_graph(bos_solver* s, int32_t enable) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    drop_graph(s);
    s->graph_failed = !enable;
    return BOS_OK;
}

int bos_triangulate(bos_solver* s) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(s->device));
    int rc = enqueue_triangulate(s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->have_dx = false;
    return BOS_OK;
}

int bos_triangulate_async(bos_solver* s) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    return enqueue_triangulate(s);
}

int bos_synchronize(bos_solver* s) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    HIP_TRY(hipStreamSynchronize(s->stream));
    return BOS_OK;
}

int bos_linearize(bos_solver* s, bos_step_stats* st) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (s->sharded || s->obs) return fail(BOS_ERR_UNSUPPORTED, "bos_linearize on a sharded handle (a rank builds part of H)");
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    if ((rc = enqueue_linearize(s))) return rc;
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    if ((rc = enqueue_stats(s, false))) return rc;
    if ((rc = read_stats(s, st, nullptr, true))) return rc;   // the events are read next
    if (st) {
        st->t_linearize_ms = elapsed(s->ev[0], s->ev[1]);
        st->t_exchange_ms = elapsed(s->ev[1], s->ev[2]);
        st->t_solve_ms = st->t_update_ms = 0.0;
    }
    return BOS_OK;
}

int bos_system_info_get(const bos_solver* s, bos_system_info* info) {
    if (!s || !info) return fail(BOS_ERR_INVALID, "null argument");
    std::memset(info, 0, sizeof(*info));
    const bos::Plan& P = s->plan;
    info->n = P.n;
    info->nnz_lower = P.nnzA();
    info->nnz_factor = uses_mf(s) ? P.mf.L_size : P.nnzL();
    const int64_t Mb = s->Mb, Mo = s->Mo, NP = s->NP, NL = s->NL;
    // compulsory reads of inputs + state, one write of every output block
    info->algorithmic_bytes = s->precision == BOS_FP32 ? 36 * Mb + 80 * Mo + 60 * NP + 32 * NL
                                                       : 64 * Mb + 152 * Mo + 120 * NP + 64 * NL;
    info->pl_factored = s->pl_factored ? 1 : 0;
    info->fold_fp32 = s->fold32 ? 1 : 0;
    info->layout_bytes = info->algorithmic_bytes - (s->pl_factored ? 12 * Mb : 0);
    info->num_block_values = P.blk.size;
    info->lanes_per_pose = P.blk.lpp;
    info->pose_lane_groups = (int32_t)P.blk.lane_pose.size();
    info->landmark_lanes = (int32_t)P.blk.lm_lane_lm.size();
    info->own_fronts = P.shard.n_own_fronts;
    info->top_fronts = P.shard.n_top_fronts;
    info->partition = s->partition;
    info->comm_ranks = 0;
    if (s->comm) {
        int count = 0;
        NC_TRY(ncclCommCount(s->comm, &count));
        info->comm_ranks = count;
    }
    return BOS_OK;
}

int bos_export_system(const bos_solver* s, int64_t capacity, int32_t* rows, int32_t* cols, double* vals, double* b) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (s->sharded) return fail(BOS_ERR_UNSUPPORTED, "bos_export_system on a subtree-sharded handle (a rank holds part of H)");
    const bos::Plan& P = s->plan;
    const int64_t nnz = P.nnzA();
    if ((rows || cols || vals) && capacity < nnz) return fail(BOS_ERR_INVALID, "export capacity < nnz_lower");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (vals) {
        const int64_t nv = P.blk.size;
        std::vector<double> v(nv);
        if (s->precision == BOS_FP32) {
            std::vector<float> f(nv);
            if (nv) HIP_TRY(hipMemcpy(f.data(), s->sys_val, nv * sizeof(float), hipMemcpyDeviceToHost));
            if (s->pl_factored) bos::dev::expand_factored_host(f.data(), v.data(), nv, P.blk.off_pl, P.blk.pose_lanes.slots());
            else for (int64_t i = 0; i < nv; ++i) v[i] = f[i];
        } else if (nv) {
            HIP_TRY(hipMemcpy(v.data(), s->sys_val, nv * sizeof(double), hipMemcpyDeviceToHost));
        }
        for (int64_t e = 0; e < nnz; ++e) vals[e] = v[P.blk.csr_src[e]];
    }
    if (rows || cols) {
        for (int64_t r = 0; r < P.n; ++r)
            for (int64_t e = P.rowptr[r]; e < P.rowptr[r + 1]; ++e) {
                const int32_t a = s->ref_dof[r], c = s->ref_dof[P.colind[e]];
                if (rows) rows[e] = std::max(a, c);
                if (cols) cols[e] = std::min(a, c);
            }
    }
    if (b) {   // b is kept in the reference numbering; the fixed pose's entries are not part of H_nf
        const int64_t nb = 3 * (int64_t)s->NP + 2 * (int64_t)s->NL;
        if (s->precision == BOS_FP32) {
            std::vector<float> v(nb);
            HIP_TRY(hipMemcpy(v.data(), s->sys_b, nb * sizeof(float), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < nb; ++i) b[i] = v[i];
        } else {
            HIP_TRY(hipMemcpy(b, s->sys_b, nb * sizeof(double), hipMemcpyDeviceToHost));
        }
        for (int d = 0; d < 3; ++d) b[3 * (int64_t)P.fixed + d] = 0.0;
    }
    return BOS_OK;
}

int bos_get_state(const bos_solver* s, double* pose_xyt, double* landmark_xy) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (pose_xyt) HIP_TRY(hipMemcpy(pose_xyt, s->d_pose, 3 * (size_t)s->NP * sizeof(double), hipMemcpyDeviceToHost));
    if (landmark_xy && s->NL)
        HIP_TRY(hipMemcpy(landmark_xy, s->d_lm, 2 * (size_t)s->NL * sizeof(double), hipMemcpyDeviceToHost));
    return BOS_OK;
}

int bos_set_state(bos_solver* s, const double* pose_xyt, const double* landmark_xy) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (pose_xyt) {
        std::vector<double> p(pose_xyt, pose_xyt + 3 * (size_t)s->NP);
        for (int i = 0; i < s->NP; ++i) p[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(p[3 * i + 2]));
        HIP_TRY(hipMemcpy(s->d_pose, p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (landmark_xy && s->NL)
        HIP_TRY(hipMemcpy(s->d_lm, landmark_xy, 2 * (size_t)s->NL * sizeof(double), hipMemcpyHostToDevice));
    int rc = upload_cache(s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return BOS_OK;
}

int bos_last_step_stamps(const bos_solver* s, uint64_t stamps[8]) {
    if (!s || !stamps) return fail(BOS_ERR_INVALID, "null argument");
    bos::dev::StepStatus h;
    std::memcpy(&h, (const void*)s->h_status, sizeof(h));   // the last step's summary (host-mapped)
    for (int i = 0; i < 8; ++i) stamps[i] = h.stamp[i];
    return BOS_OK;
}

int bos_get_last_dx(const bos_solver* s, double* dx) {
    if (!s || !dx) return fail(BOS_ERR_INVALID, "null argument");
    if (s->sharded) return fail(BOS_ERR_UNSUPPORTED, "bos_get_last_dx on a subtree-sharded handle (a rank holds part of x)");
    if (!s->have_dx) return fail(BOS_ERR_INVALID, "no step has been run");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int64_t n = s->plan.n;
    std::vector<double> x(n);
    if (n) HIP_TRY(hipMemcpy(x.data(), s->d_rhs, n * sizeof(double), hipMemcpyDeviceToHost));
    const int64_t N = n + 3;
    for (int64_t i = 0; i < N; ++i) dx[i] = 0.0;
    for (int64_t i = 0; i < n; ++i) dx[s->ref_dof[i]] = -x[i];
    return BOS_OK;
}

}  // extern "C"
