// The C ABI handle (include/bos.h) and what its implementation files share: solver_create.hip (plan,
// uploads, bos_create / bos_destroy), solver_step.hip (the GN step, its graphs and the step's entry
// points), solver_prior.hip (bos_set_priors), solver_shard.hip (the multi-rank phases and exchanges), solver_lm.hip (bos_cost / bos_optimize)
// and the covariance calls, which share cov_call.hpp: solver_cov.hip (marginals, edge covariances and edge consistency),
// solver_cov_pair.hip (pair covariances, joint compatibility, JCBB) and solver_cov_node.hip (node covariances,
// bearing association, node matching). The handle owns every device buffer (mem), the static plan
// (host/plan.hpp), the rocSOLVER refactorization state and the RCCL communicator.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/bos.h"
#include "../../../include/bos_host.h"
#include "../host/bos_math.hpp"
#include "../host/error.hpp"
#include "../host/plan.hpp"
#include "associate.hpp"
#include "device_mem.hpp"
#include "edge_check.hpp"
#include "jcbb.hpp"
#include "joint.hpp"
#include "kernels.hpp"
#include "lm.hpp"
#include "match.hpp"
#include "multifrontal.hpp"
#include "node_cov.hpp"
#include "pair_cov.hpp"
#include "prior.hpp"
#include "selinv.hpp"

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return bos::capi::fail(BOS_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define RB_TRY(expr)                                                                                   \
    do {                                                                                               \
        rocblas_status s_ = (expr);                                                                    \
        if (s_ != rocblas_status_success)                                                              \
            return bos::capi::fail(BOS_ERR_SOLVER, std::string(#expr) + ": " + rocblas_status_to_string(s_)); \
    } while (0)
#define NC_TRY(expr)                                                                                   \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess) return bos::capi::fail(BOS_ERR_COMM, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

struct bos_solver {
    bos::dev::DeviceMem mem;   // every device and host-mapped buffer below
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int precision = BOS_FP64;
    int solver_kind = BOS_SOLVER_SUPERNODAL;
    int rank = 0, world = 1;
    double kt = 1.0, damping = 0.01;
    bos::Plan plan;
    int NP = 0, NL = 0, Mb = 0, Mo = 0;
    bool has_w = false, has_dups = false;
    // fp32 build with a multifrontal solve, unit weights, no duplicate pairs: the J+H writes the
    // pose-landmark blocks factored (LinParams::pl_factored), the solver's fp64 conversion expands them
    bool pl_factored = false;
    // ... and the folds read them (and the landmark diagonal blocks) from the fp32 array themselves, so
    // the fp64 copy skips that region (bos::mf_fold_reads_fp32, mf_set_fold_source)
    bool fold32 = false;
    size_t tsize = 8;   // sizeof(T)
    // state
    double* d_pose = nullptr;
    double* d_lm = nullptr;
    // The J+H build's static inputs, carved from one allocation (solver_create.hip stage_jh_inputs): the
    // state caches in T, the work lists (host/plan.hpp BlockLayout), the records and the odometry
    void* d_pc = nullptr;
    void* d_pth = nullptr;
    void* d_lc = nullptr;
    int32_t *pw_base = nullptr, *pw_stride = nullptr, *pl_cnt = nullptr, *lw_base = nullptr, *lw_stride = nullptr, *ll_cnt = nullptr, *ll_lm = nullptr, *po_ptr = nullptr, *po_ent = nullptr, *po_oth = nullptr, *po_blk = nullptr;
    int32_t *pb_idx = nullptr, *lb_idx = nullptr, *ll_run = nullptr, *ll_hdr = nullptr;
    void *pb_z = nullptr, *pb_w = nullptr, *lb_z = nullptr, *lb_w = nullptr;
    int32_t *o_src = nullptr, *o_dst = nullptr;
    void *o_z = nullptr, *o_om = nullptr;
    int32_t* lane_pose = nullptr;            // J+H pose lane groups (Shard::lane_poses)
    int pose_blocks = 0;
    int om_stride = 6;                         // 0: every edge has the same information (LinParams)
    bool lane_identity = false;              // group i runs pose i (one GPU): the kernel skips the table
    int chi_parts = 0;                       // J+H chi^2 partial blocks this rank counts
    // node layout
    int32_t* node_dof = nullptr;
    // system
    void* d_val = nullptr;      // T, block array of H (BlockLayout)
    void* d_b = nullptr;        // T, 3 NP + 2 NL, reference dof numbering (obs: inside d_val's allocation)
    double* d_val64 = nullptr;  // fp32 build: fp64 copy of the block array for the solver
    double* d_csr64 = nullptr;  // dense / csrrf solvers: CSR values of P^T H_nf P (fp64)
    double* d_rhs = nullptr;    // n, permuted order; solution in place
    int32_t *csr_src = nullptr, *elim_ref = nullptr;
    int32_t *d_rowptr = nullptr, *d_colind = nullptr;
    int32_t *d_Lptr = nullptr, *d_Lind = nullptr, *d_pivQ = nullptr;
    double* d_Lval = nullptr;
    double* d_dense = nullptr;
    int32_t* d_info = nullptr;
    double* d_chi_part = nullptr;
    int32_t* d_nrob_part = nullptr;
    bos::dev::StepStatus* d_status = nullptr;   // end-of-iteration summary (device)
    bos::dev::StepStatus* h_status = nullptr;   // its host-mapped mirror, written by the step's last kernel
    bos::dev::StepStatus* m_status = nullptr;   // device address of h_status
    // sharded step (world > 1): BOS_PARTITION_SUBTREE (sharded) or _OBSERVATIONS (obs)
    bool sharded = false, external = false;
    int partition = BOS_PARTITION_SUBTREE;
    bool obs = false;
    int64_t pose_b0 = 0, n_pose_run = 0, lm_b0 = 0, n_lm_run = 0;   // J+H blocks this rank runs
    void* d_sys = nullptr;        // obs: the all-reduced [H values | b] (T) the solve reads
    void* sys_val = nullptr;      // the block array and b the solve reads (d_val / d_b, or d_sys)
    void* sys_b = nullptr;
    int64_t vb_count = 0;         // obs: T values of [block array (even length) | b]
    int solve_stamp = 1;          // StepStatus stamp slot the solve's first launch writes
    // ex1_recv / ex2_recv: inside the mailbox (sharded), an allocation of its own (obs: ex1_recv)
    double *ex1_send = nullptr, *ex1_recv = nullptr, *ex2_send = nullptr, *ex2_recv = nullptr;
    // every rank's exchange-1 header (chi^2, robust count), copied out of the mailbox by phase 1's
    // unpack right after its wait: a faster rank may push the next iteration's exchange 1 into the
    // mailbox before this rank's phase 2 combines the headers
    double* hdr1 = nullptr;
    uint64_t ex_timeout_ticks = 200000000ull;  // direct-exchange flag waits: 2 s (bos_set_exchange_timeout)
    // sharded: the receive buffers of both exchanges and the direct exchange's flags live in one
    // mailbox, uncached device memory (bos_exchange_p2p_connect maps every rank's into the others)
    char* mailbox = nullptr;
    bool mailbox_uncached = false;
    int64_t mb_ex1 = 0, mb_ex2 = 0, mb_flag1 = 0, mb_flag2 = 0;   // byte offsets
    bool p2p = false;                          // direct peer exchange connected
    double** d_peers = nullptr;                // [world] every rank's mailbox (own included)
    std::vector<void*> peer_maps;              // opened IPC mappings (closed at destroy)
    int64_t ex1_count = 0, ex2_count = 0;
    bos::dev::ExSeg *ex1_pack = nullptr, *ex1_unpack = nullptr;
    int n_abs = 1;                          // max |x| partials of exchange 2 (direct exchange)
    int n1p = 0, n1u = 0;
    int64_t maxlen1p = 0, maxlen1u = 0;
    int32_t *ex2_bnd = nullptr, *ex2_usrc = nullptr, *ex2_udst = nullptr;   // pack / unpack index lists
    int n_bnd = 0, n_bnd_remote = 0;
    int32_t* upd_nodes = nullptr;
    int n_upd = 0, n_upd_local = 0;
    double* abs_part = nullptr;
    int phase = 0;                           // next bos_step_phase expected (external mode)
    // triangulation inputs: bearings grouped by landmark (file order), their pose and z (fp64)
    int32_t *tri_ptr = nullptr, *tri_obs = nullptr, *tri_pose = nullptr;
    double *tri_z = nullptr, *tri_scr = nullptr;
    std::vector<int32_t> bearing_lm;             // landmark of every bearing, measurement order
    double* d_maxpart = nullptr;                 // box-plus max |dx| per update block
    rocblas_handle rb = nullptr;
    rocsolver_rfinfo rf = nullptr;
    bos::dev::MfDevice* mf = nullptr;
    bool analyzed = false;
    ncclComm_t comm = nullptr;
    hipEvent_t ev[8] = {};
    std::vector<int32_t> ref_dof;   // permuted dof -> reference dof (size n + 3)
    bool have_dx = false;
    // odometry self-loops: z[3] and Omega upper triangle [6] each (constant chi^2 terms)
    std::vector<double> loop_z, loop_om;
    double* scrub = nullptr;   // bos_time_linearize(flush_caches): 2 x 512 MiB, one read between launches
    int scrub_turn = 0;
    // one-GPU multifrontal GN step captured once into a graph (every launch argument is fixed:
    // kernel threshold and damping are baked in, so setting them drops the graph)
    hipGraph_t graph = nullptr;          // the step after its J+H build (synchronous steps)
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph_full = nullptr;     // the whole step (the steps of a batch before its last)
    hipGraphExec_t exec_full = nullptr;
    hipGraph_t pgraph[3] = {};          // sharded step, external exchanges: one graph per phase
    hipGraphExec_t pexec[3] = {};
    // sharded step with a communicator: the whole iteration (phases and their RCCL collectives) as
    // one graph; rccl_capture_failed: RCCL could not be captured, the phase graphs run instead
    hipGraph_t sgraph = nullptr, stail = nullptr;   // the whole iteration; the iteration after its J+H build
    hipGraphExec_t sexec = nullptr, stail_exec = nullptr;
    bool rccl_capture_failed = false;
    bool graph_failed = false;   // capture not possible on this stream (e.g. the legacy null stream)
    // one GPU: the status sequence number last seen, and the status launches enqueued since (each
    // bumps the device counter once; wait_status polls for seq_seen + seq_pending)
    int32_t seq_seen = 0, seq_pending = 0;
    // the last bos_marginals: J+H, factorization, selected inverse (events), download (host clock)
    double marg_ms[4] = {};
    // the last bos_edge_covariances: the same, the projection kernel (events) before the download
    double edge_ms[5] = {};
    // bos_pair_covariances (hip/pair_cov.hpp): the static path data and the device arena, both built at
    // the first call; the last call's split (host preparation and upload, J+H, factorization, path solve,
    // product and projection, download); bos_debug_set_pair_batch's limit (0: the byte budget alone)
    bos::PairPaths pair_paths;
    bool pair_paths_built = false;
    bos::dev::PairCov* pair = nullptr;
    double pair_ms[6] = {};
    int64_t pair_batch_nodes = 0;
    // bos_node_covariances (hip/node_cov.hpp): the sweep's order and the device arena, both built at the
    // first call (with pair_paths); the last call's split (host preparation and upload, J+H, factorization,
    // selected inverse, column solve, gather + projection, download)
    bos::NodeCovPlan node_plan;
    bos::dev::NodeCov* node = nullptr;
    double node_ms[7] = {};
    // bos_associate_bearings (hip/associate.hpp): the chunk buffers, built at the first call (with the node
    // call's plan and arena); the last call's split (host preparation, J+H, factorization, selected inverse,
    // column solve + gather, NIS kernel, selection, download); bos_debug_set_associate_chunk's limit (0: the
    // byte budget alone)
    bos::dev::Associate* assoc = nullptr;
    double assoc_ms[8] = {};
    int64_t assoc_chunk = 0;
    // bos_match_landmarks / bos_match_poses (hip/match.hpp): the chunk buffers, built at the first call of
    // either; the last call's split, the association's slots with the score kernel in the NIS kernel's;
    // bos_debug_set_match_chunk's limit (0: the byte budget alone)
    bos::dev::Match* match = nullptr;
    double match_ms[8] = {};
    int64_t match_chunk = 0;
    // bos_joint_compatibility (hip/joint.hpp): the batch's tables and outputs, built at the first call (with
    // pair_paths and the pair call's arena, whose blocks it reads); the last call's split (host preparation
    // and upload, J+H, factorization, path solve, products, NIS kernel, download);
    // bos_debug_set_joint_batch's limit (0: the budgets alone); the batch builder's [NP + NL] scratch
    bos::dev::Joint* joint = nullptr;
    std::vector<int32_t> joint_slot_of;
    double joint_ms[7] = {};
    int64_t joint_batch = 0;
    // bos_jcbb (hip/jcbb.hpp): the batch's frames, tables and outputs, built at the first call (with pair_paths
    // and the pair call's arena; joint_slot_of is shared); the last call's split in the joint call's slots and
    // the nodes its search visited per frame; bos_debug_set_jcbb_batch's limit (0: the budgets alone)
    bos::dev::Jcbb* jcbb = nullptr;
    double jcbb_ms[7] = {};
    std::vector<int64_t> jcbb_nodes;
    int64_t jcbb_batch = 0;
    // bos_edge_consistency (hip/edge_check.hpp): the feature's arena, built at the first call (with the edge
    // call's state and the cost pass's fp64 measurements, which it reads); the last call's split (host
    // preparation, J+H, factorization, selected inverse + emission, projection + scoring, selection, download)
    bos::dev::EdgeCheck* edge_check = nullptr;
    double check_ms[7] = {};
    // bos_set_priors (hip/prior.hpp, solver_prior.hip): the current set in one allocation of mem (null:
    // no priors). Nodes (pose priors, then landmark priors), the records in T the prior kernel reads, their
    // fp64 originals (mean[3] + upper triangle[6] per pose prior, mean[2] + [3] per landmark prior) for the
    // cost pass, and the kernel's chi^2 partials
    int n_pose_priors = 0, n_lm_priors = 0;
    char* prior_arena = nullptr;
    int32_t* pr_idx = nullptr;
    void *pr_pose = nullptr, *pr_lm = nullptr;
    double *pr_pose64 = nullptr, *pr_lm64 = nullptr, *pr_part = nullptr;
    // ---- bos_cost / bos_optimize (hip/lm.hpp). The fp64 originals of what the cost pass reads and the
    // J+H keeps only in T: odometry z / information (upper triangle) and the bearing weights (has_w)
    std::vector<double> h_oz, h_oom, h_bw;
    // device buffers, one allocation (lm_arena, null until the first use of either call) and lm_hctl
    bos::dev::DeviceMem lm_mem;
    char* lm_arena = nullptr;
    int32_t *lm_blm = nullptr, *lm_lane_lm = nullptr, *lm_pnrob = nullptr;
    double *lm_bw = nullptr, *lm_oz = nullptr, *lm_oom = nullptr;
    double *lm_pF = nullptr, *lm_pchi = nullptr, *lm_pxx = nullptr, *lm_pxb = nullptr;
    uint32_t* lm_backup[5] = {};                 // d_pose, d_lm, d_pc, d_pth, d_lc before the trial box-plus
    bos::dev::LmControl* lm_ctl = nullptr;       // the loop's state (device)
    bos::dev::LmControl* lm_hctl = nullptr;      // its host-mapped copy, written by the decision kernel
    bos::dev::LmControl* lm_mctl = nullptr;      // device address of lm_hctl
    bos_lm_iteration* lm_trace = nullptr;        // [kLmTraceCap]
    bool lm_started = false;                     // lm_lambda / lm_nu hold the last call's final values
    double lm_lambda = 0.0, lm_nu = 2.0;
    hipGraph_t lm_graph = nullptr;               // one LM iteration (multifrontal handles)
    hipGraphExec_t lm_exec = nullptr;
};
constexpr int32_t kLmTraceCap = 4096;   // bos_lm_options.max_iterations' upper limit

static_assert(bos::dev::kStepAbort == bos::dev::kMfStall, "solver abort bit");
static_assert(bos::dev::kExHeader == bos::kExHeader, "exchange header size");

// What the implementation files call in one another (each defined in the file named)
namespace bos {
namespace capi {

inline int fail(int code, const std::string& msg) { return bos::set_error(code, msg); }
// both multifrontal orderings (nested dissection / landmarks-first Schur) share the GPU engine
inline bool uses_mf(const bos_solver* s) {
    return s->solver_kind == BOS_SOLVER_SUPERNODAL || s->solver_kind == BOS_SOLVER_SCHUR;
}
inline int n_priors(const bos_solver* s) { return s->n_pose_priors + s->n_lm_priors; }
// the block array as the multifrontal solver reads it (fp64)
inline const double* mf_matrix(const bos_solver* s) {
    return s->precision == BOS_FP32 ? s->d_val64 : (const double*)s->sys_val;
}
inline float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.f;
    return ms;
}
// n calls of enqueue() back to back between events 0 and 1: the mean time of one, in ms
template <typename F> int time_enqueues(bos_solver* s, int n, F enqueue, double* ms) {
    int rc;
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    for (int i = 0; i < n; ++i)
        if ((rc = enqueue())) return rc;
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    HIP_TRY(hipEventSynchronize(s->ev[1]));
    *ms = elapsed(s->ev[0], s->ev[1]) / n;
    return BOS_OK;
}
// Calls that need the whole factor or state on this GPU: fails `name` on a rocSOLVER handle (need_mf)
// or on a multi-rank one ("<name> on a sharded handle<why>")
int require_one_gpu(const bos_solver* s, const char* name, bool need_mf, const char* why = "");

// solver_step.hip
int enqueue_linearize(bos_solver* s, unsigned long long* t_start = nullptr, bool undamped = false);
int enqueue_solver_inputs(bos_solver* s);
int enqueue_solve(bos_solver* s, bool& ran_analysis);
int enqueue_update(bos_solver* s);
int enqueue_step_tail(bos_solver* s);
int enqueue_triangulate(bos_solver* s);
int upload_cache(bos_solver* s);
double self_loop_chi(const bos_solver* s, int32_t& nrob);
int read_stats(bos_solver* s, bos_step_stats* st, int32_t* aborted = nullptr, bool sync = false);
int finish_step(bos_solver* s, bos_step_stats* st);
void drop_graph(bos_solver* s);
int capture(bos_solver* s, int phase, hipGraph_t* graph, hipGraphExec_t* exec);
// solver_shard.hip
int shard_enqueue(bos_solver* s, int phase, bool with_jh = true);
int obs_enqueue(bos_solver* s, int phase, bool with_jh = true);
int launch_rccl_step(bos_solver* s, bool sync);
int do_step_sharded(bos_solver* s, bos_step_stats* st, bool sync);
// solver_lm.hip
int enqueue_lm_iteration(bos_solver* s);
// the cost pass's buffers (the fp64 measurements among them) at their first use
int lm_buffers_setup(bos_solver* s);

}  // namespace capi
}  // namespace bos
