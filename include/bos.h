/*
 * bos.h — C ABI of the MI355X-native Gauss-Newton solver for 2-D bearing-only SLAM.
 *
 * Drop-in boundary for the reference's `proj02::Solver` (torchipeppo/prb-project-bearing-only-slam,
 * slam/solver.hpp:21-92). Plain pointers and sizes only, no exceptions across the boundary,
 * status 0 = OK, < 0 = error with a message from bos_last_error().
 *
 * Ownership and semantics follow the reference:
 *  - bos_create COPIES the problem (the reference's Solver ctor copies State and observation
 *    vectors, slam/solver.cpp:5-8); the caller's arrays are not referenced afterwards.
 *  - bos_step is synchronous: on return the state held by the handle has been updated
 *    (Solver::step, slam/solver.cpp:27-97).
 *  - one handle = one host thread; concurrent calls on one handle are undefined (the reference
 *    mutates its members H, b and the LDLT object in step(), slam/solver.hpp:58-82).
 *
 * Reference-side binding: see INTEGRATION.md.
 */
#ifndef BOS_H_
#define BOS_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BOS_ABI_VERSION 3

/* status codes */
#define BOS_OK 0
#define BOS_ERR_INVALID -1      /* bad argument / malformed problem                         */
#define BOS_ERR_DEVICE -2       /* HIP runtime error or no device                            */
#define BOS_ERR_SOLVER -3       /* rocSOLVER / rocBLAS failure                               */
#define BOS_ERR_IO -4           /* file not found / parse error                              */
#define BOS_ERR_UNSUPPORTED -5  /* input the build does not handle (see bos_last_error)     */
#define BOS_ERR_COMM -6         /* RCCL failure                                              */

/* arithmetic of the J+H build (the solve is always fp64) */
#define BOS_FP64 64
#define BOS_FP32 32

/* linear solver for H_nf dx = -b_nf (the reference: Eigen SimplicialLDLT, slam/solver.hpp:71-72) */
#define BOS_SOLVER_SUPERNODAL 0   /* GPU multifrontal supernodal Cholesky, nested dissection          */
#define BOS_SOLVER_DENSE_CHOL 1   /* rocSOLVER potrf/potrs on a dense copy (small problems)          */
#define BOS_SOLVER_ROCSOLVER_RF 2 /* rocSOLVER csrrf analysis/refactchol/solve (level-scheduled)      */
#define BOS_SOLVER_SCHUR 3        /* same GPU engine, landmarks eliminated first (default): the pose fronts
                                     factor the Schur complement S = H_pp - H_pl H_ll^-1 H_lp (config 5) */
#define BOS_SOLVER_SPARSE_CHOL BOS_SOLVER_SCHUR

/* how a world_size > 1 step is split over the ranks */
#define BOS_PARTITION_SUBTREE 0       /* default: per-rank subtrees of the Schur assembly tree below a
                                         replicated top; a rank builds only the H its fronts read, two
                                         all-gathers per iteration (subtree roots' updates, boundary x) */
#define BOS_PARTITION_OBSERVATIONS 1  /* BASELINE north star: the J+H lanes (observations in measurement
                                         order) split into contiguous ranges, one all-reduce (sum) of the
                                         whole (H, b) per iteration, the solve and update replicated */

/*
 * Problem in stix order (framework/state.hpp:47-53): poses in file order, landmarks in
 * ascending-id order (slam/triangulation.cpp:68-73). Replaces the (State, BearingObservationVector,
 * OdometryObservationVector, fixed_pose_id) arguments of Solver::Solver (slam/solver.hpp:30);
 * ids are resolved to stix once here instead of std::map::at per observation per iteration
 * (framework/state.cpp:43-63).
 */
typedef struct bos_problem {
    int32_t num_poses;              /* NP                                                        */
    int32_t num_landmarks;          /* NL                                                        */
    int32_t num_bearings;           /* M_b                                                       */
    int32_t num_odometry;           /* M_o                                                       */
    const double* pose_xyt;         /* [NP*3] x, y, theta                                        */
    const double* landmark_xy;      /* [NL*2], or NULL: triangulated on the device (bos_triangulate) */
    const int32_t* bearing_pose;    /* [M_b] pose stix                                           */
    const int32_t* bearing_landmark;/* [M_b] landmark stix                                       */
    const double* bearing_z;        /* [M_b] bearing, already smallestAngle-wrapped              */
    const double* bearing_omega;    /* [M_b] information, or NULL for 1 (observation.hpp:16,22)  */
    const int32_t* odom_src;        /* [M_o] pose stix                                           */
    const int32_t* odom_dst;        /* [M_o] pose stix                                           */
    const double* odom_z;           /* [M_o*3] x, y, theta in the source frame                   */
    const double* odom_omega;       /* [M_o*9] row-major symmetric information matrix            */
    int32_t fixed_pose;             /* stix of the pose held fixed (solver.cpp:99-125)           */
} bos_problem;

typedef struct bos_options {
    int32_t precision;              /* BOS_FP64 (default) or BOS_FP32                            */
    int32_t solver;                 /* BOS_SOLVER_SCHUR (default) / _SUPERNODAL / _DENSE_CHOL / _ROCSOLVER_RF */
    int32_t device;                 /* HIP device ordinal, -1 = current                          */
    int32_t rank;                   /* shard index (0 for one GPU)                               */
    int32_t world_size;             /* number of shards (1 for one GPU)                          */
    const void* nccl_unique_id;     /* 128-byte ncclUniqueId: bos_step runs the sharded step's two
                                       exchanges as RCCL all-gathers. NULL with world_size > 1:
                                       external exchange, the caller drives bos_step_phase and moves
                                       the buffers (bos_exchange_*). Given with world_size 1 it runs
                                       the sharded phases and RCCL with one rank (one-GPU test)      */
    double kernel_threshold;        /* robust kernel threshold, reference default 1.0 (:16)      */
    double damping;                 /* damping factor, reference default 0.01 (:17)              */
    void* stream;                   /* hipStream_t to launch on, NULL = the handle's own stream  */
    int32_t partition;              /* BOS_PARTITION_SUBTREE (default) / _OBSERVATIONS (world_size > 1) */
    int32_t lanes_per_pose;         /* J+H lanes per pose: 0 = the plan's choice, else 1, 2 or 4   */
    int32_t schur_leaf;             /* poses per nested-dissection leaf of the Schur ordering: 0 = the
                                       default (10); larger leaves give fronts over 64 rows, which run
                                       on the workgroup kernels (a planning option: the arithmetic of
                                       a front is the same)                                         */
} bos_options;

/* Per-iteration statistics (the reference prints nothing; step() returns void). */
typedef struct bos_step_stats {
    double chi2;                    /* sum e^T Omega e over all edges before the robust kernel   */
    int32_t n_robust;               /* observations scaled by the robust kernel                  */
    int32_t solver_info;            /* 0 ok, >0 number of non-positive pivots the factorization met
                                       (reported and continued, like the reference's NumericalIssue
                                       message, slam/solver.cpp:82-84)                            */
    double max_abs_dx;              /* max |dx| of the applied update (NaN if the update was not finite) */
    double t_linearize_ms;          /* J+H build only (the exchange is t_exchange_ms), timed on the
                                       device by the step's own kernels (realtime clock stamps)     */
    double t_exchange_ms;           /* RCCL exchange part (0 on one GPU)                         */
    double t_solve_ms;              /* factorization + triangular solves                         */
    double t_update_ms;             /* box-plus                                                  */
} bos_step_stats;

/* Static sizes of the linear system built by bos_create (for export buffers / roofline). */
typedef struct bos_system_info {
    int64_t n;                      /* N - 3 (fixed pose removed)                                */
    int64_t nnz_lower;              /* stored entries of the lower triangle of H_nf              */
    int64_t nnz_factor;             /* entries of the Cholesky factor (sparse solver)            */
    int64_t algorithmic_bytes;      /* SURVEY §8(d) J+H bytes for this problem and precision      */
    int64_t num_block_values;       /* size of the block array of H the J+H kernel writes        */
    int32_t lanes_per_pose;         /* J+H work split: lanes per pose (1 or 2)                   */
    int32_t pose_lane_groups;       /* J+H pose lane groups this rank runs (own, padding, top)   */
    int32_t landmark_lanes;         /* J+H landmark lanes this rank runs                         */
    int32_t own_fronts;             /* multifrontal fronts of this rank's subtrees               */
    int32_t top_fronts;             /* fronts of the replicated top (0 on one GPU)               */
    int32_t comm_ranks;             /* ranks the RCCL communicator holds (ncclCommCount), 0 without one */
    int32_t partition;              /* BOS_PARTITION_* of a sharded handle                       */
    int32_t pl_factored;            /* 1: pose-landmark blocks stored factored (3 floats, fp32 J+H) */
    int32_t fold_fp32;              /* 1: the solver's landmark folds read the fp32 block array (the fp64
                                       copy skips the pose-landmark and landmark-diagonal region)  */
    int64_t layout_bytes;           /* algorithmic_bytes with this layout's output: 12 B less per
                                       pose-landmark block when pl_factored                       */
} bos_system_info;

void bos_default_options(bos_options* opt);
const char* bos_last_error(void);
int bos_abi_version(void);
int bos_device_count(void);
/* Peer access between the visible devices (no reference counterpart: the multi-GPU bench records it
 * beside its exchange decision). out[i * n + j] = 1 if device i can access device j's memory
 * (hipDeviceCanAccessPeer; 1 on the diagonal), for n = min(capacity, bos_device_count()) devices;
 * *n_out = that n. */
int bos_device_peer_access(int32_t capacity, int32_t* out, int32_t* n_out);
/* ncclGetUniqueId for world_size > 1: rank 0 creates it, the caller distributes the bytes */
int bos_nccl_unique_id(void* out, int64_t len);

/* Solver::Solver (slam/solver.hpp:30, slam/solver.cpp:5-18) */
int bos_create(const bos_problem* problem, const bos_options* options, struct bos_solver** out);
/* ~Solver */
int bos_destroy(struct bos_solver* s);
/* Solver::set_kernel_threshold / set_damping_factor (slam/solver.hpp:33-34) */
int bos_set_kernel_threshold(struct bos_solver* s, double kt);
int bos_set_damping_factor(struct bos_solver* s, double df);
/* Solver::step (slam/solver.hpp:36, slam/solver.cpp:27-97): one synchronous GN iteration.
 * BOS_ERR_SOLVER (state untouched by the failed iteration) if the GPU factorization could not
 * complete (a dataflow dependency wait timed out); a non-positive pivot is only reported in
 * stats->solver_info, as the reference reports and continues. */
int bos_step(struct bos_solver* s, bos_step_stats* stats);
/* bos_step repeated n times with one host synchronisation at the end (UI batch of 50,
 * executables/bearing_only_slam.cpp:95-98); stats of the last iteration */
int bos_step_n(struct bos_solver* s, int n, bos_step_stats* last);
/* The J+H build alone (slam/solver.cpp:28-69) — H and b stay on the device */
int bos_linearize(struct bos_solver* s, bos_step_stats* stats);
/* Enqueue the J+H build on the handle's stream without synchronising (benchmarking) */
int bos_linearize_async(struct bos_solver* s);
int bos_synchronize(struct bos_solver* s);
/* triangulate_landmarks (slam/triangulation.cpp:65-74, per landmark triangulate_one_landmark
 * :21-62): every landmark re-estimated on the device from the current poses and its bearings
 * (column-pivoted least squares, the basic solution for single-observation landmarks), synchronous.
 * bos_create does the same when bos_problem.landmark_xy is NULL (the reference triangulates before
 * constructing the Solver, executables/bearing_only_slam.cpp). The _async form only enqueues it. */
int bos_triangulate(struct bos_solver* s);
int bos_triangulate_async(struct bos_solver* s);
int bos_system_info_get(const struct bos_solver* s, bos_system_info* info);
/*
 * Export the last linearization in the reference's dof order (poses 3*stix, landmarks
 * 3*NP + 2*stix, slam/solver_jacobians.cpp:70-71): the lower triangle of H with the fixed pose's
 * rows/cols removed (H_nofixed, slam/solver.cpp:72, indices still in full N numbering) as COO
 * (capacity = nnz_lower), and the full b[N] (slam/solver.cpp:45,61).
 */
int bos_export_system(const struct bos_solver* s, int64_t capacity, int32_t* rows, int32_t* cols, double* vals,
                      double* b);
/* On sharded handles (world_size > 1, or a communicator) bos_linearize is BOS_ERR_UNSUPPORTED (a
 * rank builds only part of H); bos_export_system and bos_get_last_dx are supported with
 * BOS_PARTITION_OBSERVATIONS after a step (every rank holds the all-reduced system and the whole
 * dx) and BOS_ERR_UNSUPPORTED with BOS_PARTITION_SUBTREE (a rank holds H and x of its own, top and
 * boundary nodes only). */
/*
 * Multi-GPU (one process per GPU, world_size > 1, BOS_SOLVER_SCHUR / _SUPERNODAL). The sparse
 * Cholesky's assembly tree is cut into per-rank subtrees below a replicated top; each rank builds
 * the part of H its fronts read (its own and the top nodes' J+H lanes), factors its subtrees, and
 * two all-gathers per iteration move the subtree roots' update matrices (exchange 1) and the
 * boundary solution (exchange 2). With a communicator bos_step does everything. Without one
 * (external exchange) the caller runs, per iteration:
 *   bos_step_phase(s, 0); all-gather of every rank's exchange-1 buffer (bos_exchange_download /
 *   bos_exchange_upload, rank order); bos_step_phase(s, 1); the same for exchange 2;
 *   bos_step_phase(s, 2, stats)   (synchronous, like bos_step).
 * After a step a rank's state is current on the nodes it owns, the top and the boundary nodes
 * (bos_node_owner: owning rank per node, -1 top, -2 fixed pose); merge per owner for the full state.
 *
 * BOS_PARTITION_OBSERVATIONS (the north star's form): phase 0 is rank r's range of J+H lanes, the one
 * exchange is an all-reduce (sum) of every rank's exchange-1 buffer (its chi^2 partials and its
 * (H, b) values, zero outside its range; bos_exchange_upload then takes the element-wise SUM, one
 * rank's size, not the concatenation), phase 1 runs the solve and the box-plus of every node and
 * returns the stats (phase 2 does not exist). Every rank then holds the whole state.
 */
int bos_step_phase(struct bos_solver* s, int32_t phase, bos_step_stats* stats);
int bos_exchange_size(const struct bos_solver* s, int32_t which, int64_t* doubles_per_rank);
int bos_exchange_download(struct bos_solver* s, int32_t which, double* send);
int bos_exchange_upload(struct bos_solver* s, int32_t which, const double* recv_all_ranks);
int bos_node_owner(const struct bos_solver* s, int32_t* owner);
/*
 * Direct peer exchange (BOS_PARTITION_SUBTREE, round 4): instead of the two ncclAllGather calls,
 * every rank writes its exchange buffers straight into every rank's receive mailbox (uncached device
 * memory, mapped into the other ranks' processes by HIP IPC: over xGMI between GPUs) and raises a
 * per-sender flag there; the receiving rank's next kernel waits for every sender's flag of the
 * current iteration (bounded: a missing peer aborts the step with BOS_ERR_SOLVER instead of
 * hanging). Two small launches per exchange, no collective library, and the whole iteration stays
 * one graph. bos_exchange_p2p_handle writes this rank's mailbox handle (BOS_P2P_HANDLE_BYTES bytes);
 * the caller gathers every rank's (rank order, e.g. torch.distributed.all_gather_object) and passes
 * them to bos_exchange_p2p_connect, after which bos_step uses the direct exchange (a communicator
 * is then not needed; world_size 1 exchanges with itself). All ranks must step in lockstep (each
 * bos_step / bos_step_n iteration on every rank). BOS_ERR_UNSUPPORTED if the mailbox cannot be
 * exported (no uncached IPC memory) or on other partitions; callers then keep RCCL.
 */
#define BOS_P2P_HANDLE_BYTES 64
int bos_exchange_p2p_handle(struct bos_solver* s, void* handle);
int bos_exchange_p2p_connect(struct bos_solver* s, const void* handles);
/* Timing contract of the direct exchange. A rank's step waits on the device for the other ranks'
 * pushes (two waits per iteration); a wait gives up after `seconds` (default 2 s, so host-side gaps
 * of one rank between its bos_step calls — the first step's graph captures, logging, a pause —
 * stay far inside it) and then marks the step aborted: every later exchange wait of that step
 * returns at once, the box-plus is skipped and bos_step returns BOS_ERR_SOLVER. A local solver
 * stall (a dataflow dependency wait that timed out) aborts the step too but does not shorten the
 * exchange waits, so that rank still receives its peers' current exchange 2. An abort raised before
 * exchange 2 travels in exchange 2's header, so every rank skips that update together and reports
 * BOS_ERR_SOLVER for the same step; a wait on exchange 2 itself that times out skips the update on
 * the ranks that timed out only, so after any BOS_ERR_SOLVER from a sharded step the caller must
 * bring all ranks back to one state (bos_set_state on every rank) or destroy the handles. Once connected, bos_step_phase and
 * bos_exchange_download / _upload return BOS_ERR_INVALID (the exchange is the handle's own). Every
 * rank must finish stepping (its last bos_step returned on every rank, e.g. a barrier) before any
 * rank calls bos_destroy: the peers' pushes write into this rank's mailbox. */
int bos_set_exchange_timeout(struct bos_solver* s, double seconds);

/* State read/write in stix order (State::poses / landmarks, framework/state.hpp:47-48) */
int bos_get_state(const struct bos_solver* s, double* pose_xyt, double* landmark_xy);
int bos_set_state(struct bos_solver* s, const double* pose_xyt, const double* landmark_xy);
/* The dx of the last bos_step in the reference's dof order (slam/solver.cpp:88-94) */
int bos_get_last_dx(const struct bos_solver* s, double* dx);

/* Marginal covariances of the current estimate: the diagonal blocks of (H_nf)^-1, H_nf being
 * exactly the matrix bos_linearize builds at the handle's current state with its current kernel
 * threshold and damping factor (fixed pose removed). H includes the damping term: call
 * bos_set_damping_factor(0) first for the plain Gauss-Newton information matrix; with zero damping
 * a landmark seen by a single bearing makes H singular (the reference dataset has three: 69, 112
 * and 114).
 * pose_cov [NP * 9] (3 x 3 per pose) and landmark_cov [NL * 4] (2 x 2 per landmark): host
 * pointers, row-major, stix order; either may be NULL; the fixed pose's block is zeros.
 * *solver_info (may be NULL): the count of non-positive pivots of the factorization; when it is not
 * zero the blocks are not meaningful (the call still returns BOS_OK, as bos_step does).
 * Synchronous. Runs the J+H build, the multifrontal factorization and a selected-inverse pass over
 * the same assembly tree (no n x n inverse is formed) as individual launches on the handle's stream.
 * The state is not touched and a following bos_step gives the results it would have given without
 * the call; the call counts as a bos_linearize for bos_export_system. After it bos_get_last_dx is
 * unspecified until the next step (here: BOS_ERR_INVALID, as before the first step).
 * BOS_ERR_UNSUPPORTED on BOS_SOLVER_DENSE_CHOL / BOS_SOLVER_ROCSOLVER_RF handles and on sharded
 * handles (world_size > 1, a communicator, or external / direct exchange); BOS_ERR_DEVICE (with the
 * byte count in bos_last_error) when the pass's buffers cannot be allocated: the handle stays usable. */
int bos_marginals(struct bos_solver* s, double* pose_cov, double* landmark_cov, int32_t* solver_info);
/* Edge covariances of the current estimate: for every bearing and odometry edge of the problem, the
 * cross-covariance block of its two nodes and the covariance of its predicted measurement, computed on
 * the device in the same pass as the diagonal blocks of bos_marginals. H_nf, the damping, the kernel
 * threshold, the state handling, the synchronous behaviour, *solver_info and the clearing of the pivot
 * word are exactly those of bos_marginals; so are the "counts as a bos_linearize" rule and
 * bos_get_last_dx afterwards. pose_cov and landmark_cov are bit for bit what bos_marginals returns at
 * the same state. Host pointers, edge (measurement) order, row-major:
 *   bearing_cross [M_b * 6]  Sigma(pose dofs, landmark dofs), 3 x 2
 *   odom_cross    [M_o * 9]  Sigma(src dofs, dst dofs), 3 x 3
 *   bearing_var   [M_b]      J Sigma_joint J^T, J the 1 x 5 bearing Jacobian
 *   odom_cov      [M_o * 9]  J Sigma_joint J^T, J the 3 x 6 odometry Jacobian
 * Any output may be NULL: it is neither downloaded nor computed (with all four edge outputs NULL the
 * call is bos_marginals). Sigma_joint of an edge with nodes (a, b) is [[S_aa, S_ab], [S_ab^T, S_bb]].
 * The fixed pose's diagonal block and every cross block that involves it are exactly zero: a bearing
 * taken from the fixed pose has bearing_var = J_l S_ll J_l^T, an odometry edge that touches it uses the
 * free pose's columns only. An odometry self-loop (src == dst) has odom_cross = S_aa and all four blocks
 * of its Sigma_joint equal to S_aa. Duplicate edges each get their own slot, bit-identical between
 * duplicates of one orientation; a reversed duplicate (dst, src) gets the transposed cross block.
 * J is bearing_error_jacobian<double> / odometry_error_jacobian<double> (csrc/host/bos_math.hpp) at the
 * fp64 master state with cos / sin computed in fp64, on every handle, fp32 ones included (as bos_cost);
 * neither depends on the measurement. odom_cov is evaluated on its lower triangle and mirrored (each
 * block is bit-symmetric), bearing_var is one fixed-order sum; two calls give identical bits.
 * The cross blocks are pieces of the selected inverse the pass forms anyway (H lies inside L's
 * pattern): each front writes those of its edges into a pair buffer, and one kernel projects every
 * edge. The buffers are allocated at the first call that asks for an edge output; a handle that never
 * does pays nothing.
 * BOS_ERR_UNSUPPORTED on BOS_SOLVER_DENSE_CHOL / BOS_SOLVER_ROCSOLVER_RF handles and on sharded handles;
 * BOS_ERR_DEVICE (with the byte count in bos_last_error) when the feature's buffers cannot be
 * allocated: the handle stays usable and bos_marginals still works. */
int bos_edge_covariances(struct bos_solver* s, double* bearing_cross, double* odom_cross, double* bearing_var,
                         double* odom_cov, double* pose_cov, double* landmark_cov, int32_t* solver_info);
/* Pair covariances of the current estimate: the joint covariance of n_pairs arbitrary node pairs, whether
 * the problem has an edge between them or not (loop-closure candidates, a bearing that may belong to a
 * landmark the pose never observed, two landmarks that may be one). Node ids use the numbering of
 * bos_node_owner: pose stix u is u, landmark stix l is NP + l. An id outside [0, NP + NL) gives
 * BOS_ERR_INVALID; a mixed pair must be written (pose, landmark), the opposite order gives BOS_ERR_INVALID.
 * Every output is [9 * n_pairs] doubles (host pointers): pair q's block row-major in the first rows * cols
 * of its nine entries, the rest exactly 0. Any output may be NULL: it is neither computed nor downloaded.
 * n_pairs == 0 returns BOS_OK and touches nothing.
 *   cross      Sigma(a, b): 3 x 3, 3 x 2 or 2 x 2
 *   projected  pose-pose: the 3 x 3 J Sigma_joint J^T of the odometry prediction a -> b; pose-landmark:
 *              entry 0 holds the variance of the predicted bearing; landmark-landmark: the 2 x 2
 *              covariance of l_a - l_b = S_aa + S_bb - S_ab - S_ab^T (lower triangle, mirrored)
 *   cov_a      Sigma(a, a)
 *   cov_b      Sigma(b, b)
 * With H_nf = L L^T, Sigma(a, b) = (L^-1 E_a)^T (L^-1 E_b), and L^-1 E_a is non-zero only on the supernodes
 * between a's and the root of the assembly tree: each distinct node of the call gets one sparse forward
 * solve along its root path (one wavefront), each pair the products over the dofs its two paths share.
 * cov_a / cov_b come from the same product (lower triangle evaluated and mirrored: bit-symmetric); they
 * are not promised bit-equal to bos_marginals, whose summation differs. The Jacobians, the state they are
 * evaluated at (fp64 master state, fp64 cos / sin on every handle) and the projection's arithmetic are
 * those of bos_edge_covariances.
 * H_nf, the damping, the kernel threshold, the state handling, the synchronous behaviour, *solver_info,
 * the clearing of the pivot word, the "counts as a bos_linearize" rule and bos_get_last_dx afterwards are
 * exactly those of bos_marginals.
 * Exact rules: the fixed pose's diagonal block and every cross block that involves it are exactly zero
 * (the projection then uses the other node's columns only); a pair (a, a) has cross == cov_a == cov_b;
 * duplicate queries return identical bits; (b, a) returns the exact transpose of (a, b); two calls give
 * identical bits; a query's result depends neither on the other pairs of the call nor on how the call is
 * split into batches (a call whose path-solve buffer would pass 64 MiB runs in batches).
 * The buffers are allocated at the first call; a handle that never calls pays nothing.
 * BOS_ERR_SOLVER on a stalled factorization; BOS_ERR_UNSUPPORTED on BOS_SOLVER_DENSE_CHOL /
 * BOS_SOLVER_ROCSOLVER_RF handles, on sharded handles and when a node's dofs straddle two supernodes;
 * BOS_ERR_DEVICE (with the byte count in bos_last_error) when the feature's buffers cannot be allocated:
 * the handle stays usable. */
int bos_pair_covariances(struct bos_solver* s, int64_t n_pairs, const int32_t* node_a, const int32_t* node_b, double* cross,
                         double* projected, double* cov_a, double* cov_b, int32_t* solver_info);
/* Node covariances of the current estimate: the covariance of each of n_nodes query nodes against every
 * node, the block column Sigma(:, a) = H_nf^-1 E_a (which old poses could close a loop with the current
 * one, which landmarks a new bearing could belong to). Node ids as for bos_pair_covariances: pose stix u is
 * u, landmark stix l is NP + l; an id outside [0, NP + NL) gives BOS_ERR_INVALID and touches nothing.
 * n_nodes == 0 returns BOS_OK and touches nothing. Outputs are host pointers, row-major; any may be NULL:
 * it is neither computed nor downloaded. With i the query index, a = nodes[i], d_a = 3 or 2, each block
 * fills the first rows * cols entries of its slot, the rest of the slot is exactly 0:
 *   cross_pose          [n_nodes][NP][9]  Sigma(a, pose u), d_a x 3: rows a's dofs, columns the target's
 *   cross_landmark      [n_nodes][NL][6]  Sigma(a, landmark l), d_a x 2
 *   projected_pose      [n_nodes][NP][9]  a pose: the 3 x 3 J Sigma_joint J^T of the odometry prediction
 *                                         a -> u; a landmark: entry 0 is the variance of the predicted
 *                                         bearing of landmark a from pose u
 *   projected_landmark  [n_nodes][NL][4]  a pose: entry 0 is the variance of the predicted bearing of
 *                                         landmark l from pose a; a landmark: the 2 x 2 covariance of
 *                                         l_a - l_l
 *   pose_cov, landmark_cov                as in bos_marginals, bit for bit what it returns at this state
 * With H_nf = L L^T the column is L^-T (L^-1 E_a): the root-path solve of bos_pair_covariances for the one
 * node, then one backward substitution over every front of the assembly tree with d_a right-hand sides,
 * which reads L once; per query node one launch per tree level and front class, then one thread per target
 * node. The cross block of Sigma_joint comes from the column (transposed for a landmark query against a
 * pose), both diagonal blocks from the selected inverse of bos_marginals: a call that asks for a projected
 * output or for pose_cov / landmark_cov runs that pass on the same factorization, a call that asks for cross
 * blocks only does not. The Jacobians, the state they are evaluated at (fp64 master state, fp64 cos / sin
 * on every handle) and the projection's arithmetic are those of bos_edge_covariances / bos_pair_covariances.
 * H_nf, the damping, the kernel threshold, the state handling, the synchronous behaviour, *solver_info,
 * the clearing of the pivot word, the "counts as a bos_linearize" rule and bos_get_last_dx afterwards are
 * exactly those of bos_marginals.
 * Exact rules: with a the fixed pose every cross block is exactly zero (the projections then use the
 * target's columns only); the block of the fixed pose as target is exactly zero for every a (its
 * projection uses a's columns only); the own block (u == a) is evaluated like every other one: it is not
 * promised bit-symmetric, nor bit-equal to bos_marginals, but the projected entry for u == a uses the
 * marginals' S_aa for all four blocks (the self-loop rule of bos_edge_covariances), so the
 * landmark-landmark entry is exactly 0; two calls give identical bits; a query's bits do not depend on
 * the other nodes of the call, and a repeated id returns identical bits.
 * The buffers (X, one node's output blocks, the index arrays) are allocated at the first call; a handle
 * that never calls pays nothing.
 * BOS_ERR_SOLVER on a stalled factorization; BOS_ERR_UNSUPPORTED on BOS_SOLVER_DENSE_CHOL /
 * BOS_SOLVER_ROCSOLVER_RF handles, on sharded handles, when a front exceeds the path solve's LDS and when a
 * node's dofs straddle two supernodes (the limits of bos_pair_covariances); BOS_ERR_DEVICE (with the byte
 * count in bos_last_error) when the feature's buffers cannot be allocated: the handle stays usable. */
int bos_node_covariances(struct bos_solver* s, int32_t n_nodes, const int32_t* nodes, double* cross_pose,
                         double* cross_landmark, double* projected_pose, double* projected_landmark, double* pose_cov,
                         double* landmark_cov, int32_t* solver_info);
/* Bearing association at the current estimate: n_bearings new bearings, bearing q measured as z[q] from
 * pose stix pose[q] with information omega[q] (omega NULL: 1 for every bearing), each gated against every
 * landmark of the problem on the device. For bearing q, a = pose[q] and landmark stix l:
 *   e   = bearing_error<double> (csrc/host/bos_math.hpp) = normalized_angle(predicted bearing of l from a - z[q]),
 *         at the fp64 master state with cos / sin computed in fp64, on every handle, fp32 ones included (as
 *         bos_cost); z may be any finite value, it is not wrapped first
 *   var = the variance of the predicted bearing of l from a: exactly the number bos_node_covariances puts in
 *         projected_landmark[.][l][0] for the query node a, by the same device code and with its fixed-pose
 *         rule (from the fixed pose it is J_l S_ll J_l^T)
 *   S   = var + 1.0 / omega[q]
 *   nis = (e * e) / S, evaluated in this order without FP contraction: a caller reproduces its bits from e
 *         and S with IEEE arithmetic
 * Outputs (host pointers; any may be NULL: it is neither computed nor downloaded), k in 1 .. BOS_ASSOC_MAX_K:
 *   cand_landmark   [n_bearings][k]  landmark stix, -1 where nothing is listed
 *   cand_nis        [n_bearings][k]  +inf where nothing is listed; bit for bit nis_all[q][cand_landmark[q][j]]
 *   cand_innovation [n_bearings][k]  e of the listed landmark, 0 where nothing is listed
 *   cand_var        [n_bearings][k]  S of the listed landmark, 0 where nothing is listed
 *   n_inside        [n_bearings]     landmarks with nis <= gate: all of them, not min(., k)
 *   nis_all         [n_bearings][NL] the whole row
 * The listed candidates are the min(k, n_inside) smallest NIS among the landmarks with nis <= gate, ascending
 * by (nis, landmark stix): equal NIS go to the lower stix first. A nis that is not finite (a landmark that
 * sits on the pose) is never listed and never counted; nis_all still holds what was computed. Landmarks the
 * pose already observes are not excluded: the caller knows its edges. gate may be +inf.
 * n_bearings == 0 returns BOS_OK and touches nothing; with NL == 0 every count is 0 and every list is
 * padding. BOS_ERR_INVALID, with nothing touched, for a pose outside [0, NP), a z that is not finite, an
 * omega that is not finite and positive, a gate that is NaN or <= 0 and k outside 1 .. BOS_ASSOC_MAX_K.
 * The bearings are grouped by pose. Per distinct pose: the column solve and gather of bos_node_covariances
 * for projected_landmark alone, read in place on the device; then, per chunk of that pose's bearings (a
 * chunk's NIS rows stay within 64 MiB), one kernel with a thread per landmark and bearing and two selection
 * launches (per tile of landmarks and bearing, then per bearing); per chunk k entries and a count per
 * bearing are downloaded, the rows only for nis_all.
 * H_nf, the damping, the kernel threshold, the state handling, the synchronous behaviour, *solver_info,
 * the clearing of the pivot word, the "counts as a bos_linearize" rule and bos_get_last_dx afterwards are
 * exactly those of bos_marginals.
 * Exact rules: two calls give identical bits; a bearing's results depend neither on the other bearings of
 * the call, nor on their order, nor on how the call is split into chunks; a repeated (pose, z, omega)
 * returns identical bits.
 * The buffers are allocated at the first call (with those of bos_node_covariances, if it has not run); a
 * handle that never calls pays nothing.
 * BOS_ERR_SOLVER, BOS_ERR_UNSUPPORTED and BOS_ERR_DEVICE on exactly the conditions of bos_node_covariances:
 * the handle stays usable. */
#define BOS_ASSOC_MAX_K 8
int bos_associate_bearings(struct bos_solver* s, int32_t n_bearings, const int32_t* pose, const double* z,
                           const double* omega, double gate, int32_t k, int32_t* cand_landmark, double* cand_nis,
                           double* cand_innovation, double* cand_var, int32_t* n_inside, double* nis_all,
                           int32_t* solver_info);
/* Landmark matching at the current estimate (are two landmarks really one?): each of n_queries query
 * landmarks, stix landmark[q], gated against every other landmark on the device by the squared Mahalanobis
 * distance of their difference. For query a = landmark[q] and target landmark stix l != a:
 *   d  = (l_a.x - l_l.x, l_a.y - l_l.y) at the fp64 master state
 *   C  = the 2 x 2 covariance of l_a - l_l: exactly the four numbers bos_node_covariances puts in
 *        projected_landmark[.][l][0..3] for the query node NP + a, by the same device code, read in place;
 *        only its lower triangle c00 = C[0], c10 = C[2], c11 = C[3] is used
 *   d2 = d^T C^-1 d through the LDL^T of C, evaluated in this order without FP contraction:
 *        D0 = c00, t = c10 / D0, D1 = c11 - t * c10, y1 = d1 - t * d0, d2 = (d0 * d0) / D0 + (y1 * y1) / D1;
 *        NaN when D0 or D1 is not finite and > 0. A caller reproduces its bits from d and C.
 * The entry l == a is NaN by definition (its C is exactly 0 by the node call's self rule).
 * Outputs (host pointers; any may be NULL: it is neither computed nor downloaded), k in 1 .. BOS_MATCH_MAX_K:
 *   cand_landmark [n_queries][k]     landmark stix, -1 where nothing is listed
 *   cand_d2       [n_queries][k]     +inf where nothing is listed; bit for bit d2_all[q][cand_landmark[q][j]]
 *   cand_diff     [n_queries][k][2]  d of the listed landmark, 0 where nothing is listed
 *   cand_cov      [n_queries][k][4]  C of the listed landmark, 0 where nothing is listed
 *   n_inside      [n_queries]        landmarks with d2 <= gate: all of them, not min(., k)
 *   d2_all        [n_queries][NL]    the whole row
 * Order and gate are those of bos_associate_bearings: the min(k, n_inside) smallest d2 among the landmarks
 * with d2 <= gate, ascending by (d2, stix), equal d2 to the lower stix first; a d2 that is not finite is
 * never listed and never counted. gate may be +inf.
 * n_queries == 0 returns BOS_OK and touches nothing. BOS_ERR_INVALID, with nothing touched, for a landmark
 * outside [0, NL), a gate that is NaN or <= 0 and k outside 1 .. BOS_MATCH_MAX_K. On a handle whose only
 * node is the fixed pose every list is padding, every count 0 and a row NaN.
 * Per distinct landmark: the column solve and gather of bos_node_covariances for projected_landmark alone,
 * one kernel with a thread per target and the two selection launches of bos_associate_bearings; k entries
 * and a count are downloaded, the row only for d2_all; a repeated query is copied on the host.
 * H_nf, the damping, the kernel threshold, the state handling, the synchronous behaviour, *solver_info,
 * the clearing of the pivot word, the "counts as a bos_linearize" rule and bos_get_last_dx afterwards are
 * exactly those of bos_marginals.
 * Exact rules: two calls give identical bits; a query's results depend neither on the other queries of the
 * call nor on their order; a repeated query returns identical bits.
 * The buffers (shared with bos_match_poses) are allocated at the first call of either, with those of
 * bos_node_covariances if it has not run; a handle that never calls pays nothing.
 * BOS_ERR_SOLVER, BOS_ERR_UNSUPPORTED and BOS_ERR_DEVICE on exactly the conditions of bos_node_covariances:
 * the handle stays usable. */
#define BOS_MATCH_MAX_K BOS_ASSOC_MAX_K
int bos_match_landmarks(struct bos_solver* s, int32_t n_queries, const int32_t* landmark, double gate, int32_t k,
                        int32_t* cand_landmark, double* cand_d2, double* cand_diff, double* cand_cov, int32_t* n_inside,
                        double* d2_all, int32_t* solver_info);
/* Pose matching at the current estimate (which old poses could close a loop with this one?): n_meas
 * relative-pose measurements, measurement q = z[q] = (x, y, theta) in the frame of pose stix pose[q] with
 * the 3 x 3 information omega[q] (row-major; omega NULL: the identity for every measurement), each gated
 * against every pose on the device by its normalised innovation squared. For a = pose[q] and target pose u:
 *   e   = the error of odometry_error_jacobian<double> (csrc/host/bos_math.hpp) for source a, destination u
 *         and measurement z[q], at the fp64 master state with cos / sin computed in fp64 on every handle
 *         (as bos_cost); z may be any finite value, it is not wrapped first
 *   P   = the 3 x 3 projected_pose[.][u] of bos_node_covariances for the query node a, by the same device
 *         code and with its fixed-pose and self rules, read in place; only its lower triangle is used
 *   R   = omega[q]^-1, formed once per measurement on the host (bos_match_information_inverse, bos_host.h)
 *   S   = P + R, entry-wise on the lower triangle
 *   nis = e^T S^-1 e through the LDL^T of S, evaluated in this order without FP contraction:
 *         D0 = s00, l10 = s10 / D0, l20 = s20 / D0, D1 = s11 - l10 * s10, t21 = s21 - l20 * s10,
 *         l21 = t21 / D1, D2 = (s22 - l20 * s20) - l21 * t21,
 *         y0 = e0, y1 = e1 - l10 * y0, y2 = (e2 - l20 * y0) - l21 * y1,
 *         nis = ((y0 * y0) / D0 + (y1 * y1) / D1) + (y2 * y2) / D2;
 *         NaN when a pivot is not finite and > 0. A caller reproduces its bits from e and S.
 * u == a is evaluated like every other target: the caller knows its query.
 * Outputs (host pointers; any may be NULL), k in 1 .. BOS_MATCH_MAX_K:
 *   cand_pose       [n_meas][k]     pose stix, -1 where nothing is listed
 *   cand_nis        [n_meas][k]     +inf where nothing is listed; bit for bit nis_all[q][cand_pose[q][j]]
 *   cand_innovation [n_meas][k][3]  e of the listed pose, 0 where nothing is listed
 *   cand_cov        [n_meas][k][9]  S of the listed pose, its lower triangle mirrored; 0 where nothing is listed
 *   n_inside        [n_meas]        poses with nis <= gate: all of them
 *   nis_all         [n_meas][NP]    the whole row
 * Order, gate and padding as for bos_match_landmarks. n_meas == 0 returns BOS_OK and touches nothing.
 * BOS_ERR_INVALID, with nothing touched, for a pose outside [0, NP), a z that is not finite, an omega that
 * is not finite, not bit-symmetric or whose LDL^T has a pivot <= 0, a gate that is NaN or <= 0 and k outside
 * 1 .. BOS_MATCH_MAX_K.
 * The measurements are grouped by pose. Per distinct pose: the column solve and gather of
 * bos_node_covariances for projected_pose alone; then, per chunk of that pose's measurements (a chunk's
 * rows stay within 64 MiB), one kernel with a thread per target and measurement and the two selection
 * launches. Everything else - the system, *solver_info, the exact rules (a measurement's results depend
 * neither on the other measurements, nor on their order, nor on the chunks), the buffers, the errors - as
 * for bos_match_landmarks. */
int bos_match_poses(struct bos_solver* s, int32_t n_meas, const int32_t* pose, const double* z, const double* omega,
                    double gate, int32_t k, int32_t* cand_pose, double* cand_nis, double* cand_innovation, double* cand_cov,
                    int32_t* n_inside, double* nis_all, int32_t* solver_info);
/* Joint compatibility at the current estimate (Neira & Tardos' JCBB test): the joint NIS
 *   d2 = e^T (J Sigma J^T + R)^-1 e
 * over the stacked innovation of a hypothesis, for n_hyp hypotheses in one call. Hypothesis h consists of the
 * pairings hyp_start[h] .. hyp_start[h + 1] - 1 (hyp_start has n_hyp + 1 entries, hyp_start[0] == 0, never
 * decreasing); m_h is its size (at most BOS_JOINT_MAX_M, 0 allowed) and n_pair = hyp_start[n_hyp]. Pairing i
 * means: the bearing z[i], taken from pose stix pose[i] with information omega[i] (omega NULL: 1 everywhere),
 * is assigned to landmark stix landmark[i]. Per hypothesis, i and j its local indices:
 *   e_i   bearing_error<double> at the fp64 master state, fp64 cos / sin on every handle: the code and the
 *         conventions of bos_associate_bearings (z is not wrapped first)
 *   J_i   the 1 x 5 bearing_error_jacobian<double> over [pose dofs | landmark dofs], as in bos_pair_covariances
 *   S_ii  edge_bearing_var(Sigma_pp, Sigma_ll, Sigma_pl, J_i) + 1.0 / omega_i: bit for bit the projected[0]
 *         bos_pair_covariances returns for the pair (pose_i, NP + landmark_i) at this state, plus
 *         1.0 / omega_i (the same device code on the same blocks)
 *   S_ij  (i > j) J_i C_ij J_j^T, C_ij the 5 x 5 matrix of the four blocks Sigma(p_i, p_j), Sigma(p_i, l_j),
 *         Sigma(l_i, p_j), Sigma(l_i, l_j). Each block is exactly what bos_pair_covariances computes for that
 *         node pair (the path solve, then the product over the common tail), read transposed where the pair
 *         call would need the opposite order; a block that involves the fixed pose is exactly zero; a block
 *         between a node and itself is its cov_a. Evaluation: t = C_ij J_j^T (5 entries, each an ascending
 *         sum), then J_i t ascending, without FP contraction (csrc/host/joint.hpp joint_S_offdiag). S_ji is
 *         the same value: S is bit-symmetric.
 * LDL^T and the prefix NIS: right-looking, one IEEE operation at a time, without FP contraction. A is the
 * working copy of S, y of e. For k = 0 .. m - 1: D_k = A_kk; for i > k: l_ik = A_ik / D_k; for i > k and
 * k < j <= i: A_ij = A_ij - l_ik * A_jk (A_jk the unscaled value); for i > k: y_i = y_i - l_ik * y_k;
 * prefix_k = prefix_{k-1} + (y_k * y_k) / D_k, prefix_{-1} = 0. From the first k whose D_k is not finite and
 * > 0 that prefix and all later ones are NaN. A caller reproduces every bit from the returned e and S.
 * Outputs (host pointers; any may be NULL: it is neither computed nor downloaded):
 *   prefix_nis     [n_pair]  entry i of hypothesis h: the joint NIS of its pairings 0 .. i (one call
 *                            evaluates a whole branch of the interpretation tree)
 *   joint_nis      [n_hyp]   the last prefix of h; 0 for an empty hypothesis
 *   innovation     [n_pair]  e
 *   innovation_cov           hypothesis h's m_h x m_h block, row-major, at offset sum over g < h of m_g^2
 *   solver_info              as in bos_marginals
 * Exact rules: two calls give identical bits; a hypothesis's bits depend neither on the other hypotheses of
 * the call, nor on their order, nor on the batch it lands in; a repeated hypothesis returns identical bits;
 * the hypothesis made of the first k pairings of h returns h's prefix_nis[0 .. k - 1], h's leading k x k
 * block of S and h's first k entries of e, bit for bit. A hypothesis may repeat a pose, a landmark or a whole
 * pairing: R keeps S positive definite.
 * n_hyp == 0 returns BOS_OK and touches nothing. BOS_ERR_INVALID, with nothing touched: hyp_start[0] != 0 or
 * a decreasing hyp_start, m_h > BOS_JOINT_MAX_M, a pose outside [0, NP) or a landmark outside [0, NL), a z
 * that is not finite, an omega that is not finite and positive.
 * Per batch of whole consecutive hypotheses (Y slices limited to the pair call's 64 MiB; one hypothesis
 * always runs) the host reduces the pairings to the distinct free nodes and the needed node pairs to the
 * distinct ones; the device runs the pair call's path solve and products, then one wavefront per hypothesis
 * that assembles S in LDS, factors it and sums the prefixes. Nothing but the outputs is downloaded.
 * H_nf, the damping, the kernel threshold, the state handling, the synchronous behaviour, the clearing of
 * the pivot word, the "counts as a bos_linearize" rule and bos_get_last_dx afterwards are exactly those of
 * bos_marginals. BOS_ERR_SOLVER, BOS_ERR_UNSUPPORTED and BOS_ERR_DEVICE fire on exactly the conditions of
 * bos_pair_covariances: the handle stays usable. The buffers are allocated at the first call; a handle that
 * never calls pays nothing. */
#define BOS_JOINT_MAX_M 32
int bos_joint_compatibility(struct bos_solver* s, int32_t n_hyp, const int32_t* hyp_start, const int32_t* pose,
                            const int32_t* landmark, const double* z, const double* omega, double* prefix_nis,
                            double* joint_nis, double* innovation, double* innovation_cov, int32_t* solver_info);
/* Joint-compatibility branch and bound at the current estimate (Neira & Tardos' JCBB): per frame of new
 * bearings, the search over the interpretation tree that bos_joint_compatibility evaluates one branch of, on
 * the device; nothing but the winning assignment comes back. n_frames frames in one call.
 * Frame f consists of the bearings frame_start[f] .. frame_start[f + 1] - 1 (frame_start has n_frames + 1
 * entries, frame_start[0] == 0, never decreasing); m_f is their number (at most BOS_JCBB_MAX_BEARINGS, 0
 * allowed) and n_bearings = frame_start[n_frames]. Bearing b has the pose stix pose[b], the measurement z[b],
 * the information omega[b] (omega NULL: 1 everywhere) and the candidate list
 * cand_landmark[cand_start[b] .. cand_start[b + 1]) of c_b >= 0 landmark stix in the caller's order (the order
 * bos_associate_bearings returns is the intended one); cand_start has n_bearings + 1 entries, cand_start[0] == 0,
 * never decreasing, and n_pairings = cand_start[n_bearings]. The frame's pairings are all its (bearing,
 * candidate) pairs in (bearing, list position) order; their number P_f is at most BOS_JOINT_MAX_M.
 * All-pairings system: e_all [P_f] and S_all [P_f x P_f] are exactly the innovation and innovation_cov that
 * bos_joint_compatibility returns for the hypothesis made of the frame's pairings in that order, bit for bit
 * (the same host preparation, the same device code per entry).
 * Hypothesis: it assigns to each bearing one of its candidates or nothing (-1); no landmark is assigned to two
 * bearings of the frame. Its pairings are taken in bearing order; its S and e are the corresponding principal
 * submatrix of S_all and subvector of e_all; its prefix NIS values are those of bos_joint_compatibility's
 * recurrence on that submatrix, bit for bit (evaluated row by row: for a fixed entry the subtractions stay in
 * ascending k, csrc/host/jcbb.hpp).
 * Admissible: a hypothesis of n pairings is admissible iff for every j = 1 .. n its j-th prefix NIS is finite
 * and <= gate[j - 1]. gate has BOS_JOINT_MAX_M entries, chi^2 quantiles by degrees of freedom, each finite and
 * > 0, or +inf. The empty hypothesis is admissible.
 * Result of a frame: the admissible hypothesis with 1. the most pairings; 2. among those the smallest joint NIS
 * (last prefix); 3. among those the lexicographically smallest choice vector, a bearing's choice being its list
 * position and "nothing" ranking after every position. A total order: the result does not depend on the order
 * of the search.
 * The search cuts a node whose prefix NIS fails its gate or whose pivot is not finite and positive, with its
 * subtree (prefix NIS never decreases in floating point: this is the definition, not a heuristic); a node whose
 * pairings so far plus the later bearings that have a candidate are strictly fewer than the best count found;
 * and, at equal potential, a node whose prefix NIS already exceeds the best NIS known at that count.
 * Node budget: a frame's search visits at most max_nodes tree nodes (a node: a choice whose row was evaluated,
 * or a step "nothing"); 0 means 2^22, values above 2^26 are clamped. complete[f] = 1 when the search ended by
 * itself: the result is then the one defined above. Otherwise complete[f] = 0 and the returned hypothesis is
 * admissible with a count of pairings that was found; it is not promised optimal.
 * Outputs (host pointers; any may be NULL: it is neither computed nor downloaded):
 *   assignment     [n_bearings]  the landmark stix assigned to the bearing, or -1
 *   n_paired       [n_frames]    the result's pairings
 *   joint_nis      [n_frames]    its joint NIS; 0 for no pairing
 *   prefix_nis     [n_bearings]  the joint NIS of the result's pairings among the frame's bearings 0 .. b
 *   complete       [n_frames]
 *   innovation     [n_pairings]  e_all
 *   innovation_cov               frame f's P_f x P_f block S_all, row-major, at offset sum over g < f of P_g^2
 *   solver_info                  as in bos_marginals
 * Exact rules, for frames with complete == 1: two calls give identical bits; a frame's results depend neither
 * on the other frames of the call, nor on their order, nor on the batch it lands in; a repeated frame returns
 * identical bits; joint_nis[f] and prefix_nis at the paired bearings are bit for bit what
 * bos_joint_compatibility returns for the result's pairings as one hypothesis at the same state; innovation and
 * innovation_cov are bit for bit those of the all-pairings hypothesis.
 * n_frames == 0 returns BOS_OK and touches nothing. BOS_ERR_INVALID, with nothing touched: frame_start[0] or
 * cand_start[0] != 0, a decreasing frame_start or cand_start, m_f > BOS_JCBB_MAX_BEARINGS, P_f >
 * BOS_JOINT_MAX_M, a pose outside [0, NP) or a landmark outside [0, NL), a landmark listed twice for one
 * bearing, a z that is not finite, an omega that is not finite and positive, a gate entry that is NaN or <= 0,
 * max_nodes < 0.
 * Per batch of whole consecutive frames (bos_joint_compatibility's batches of the all-pairings hypotheses) the
 * device runs the pair call's path solve and products, then one wavefront per frame that assembles S_all in
 * LDS and searches it in place. Everything else - H_nf, the damping, the kernel threshold, the state handling,
 * the synchronous behaviour, the clearing of the pivot word, the "counts as a bos_linearize" rule,
 * bos_get_last_dx afterwards, BOS_ERR_SOLVER, BOS_ERR_UNSUPPORTED and BOS_ERR_DEVICE - is exactly as for
 * bos_joint_compatibility. The buffers are allocated at the first call; a handle that never calls pays
 * nothing. */
#define BOS_JCBB_MAX_BEARINGS 32
int bos_jcbb(struct bos_solver* s, int32_t n_frames, const int32_t* frame_start, const int32_t* pose, const double* z,
             const double* omega, const int32_t* cand_start, const int32_t* cand_landmark, const double* gate, int64_t max_nodes,
             int32_t* assignment, int32_t* n_paired, double* joint_nis, double* prefix_nis, int32_t* complete, double* innovation,
             double* innovation_cov, int32_t* solver_info);
/* Edge consistency at the current estimate (Baarda's data snooping): every bearing and odometry edge that IS
 * in the graph is tested against the estimate it helped to produce, and the k worst of each kind are listed on
 * the device. H is sum J^T Omega J + lambda I and the robust kernel scales the right-hand side only, so with
 * R = Omega^-1 and P = J Sigma_joint J^T (bos_edge_covariances' bearing_var / odom_cov) the residual of an edge
 * at the optimum has the covariance T = R - P, positive semi-definite in exact arithmetic for every
 * lambda >= 0. Per edge:
 *   w2         = e^T T^-1 e, the normalised residual squared: chi^2 with 1 (bearing) or 3 (odometry) degrees of
 *                freedom for a consistent edge
 *   chi2       = e^T Omega e, the edge's term of bos_step_stats.chi2
 *   redundancy = 1 - tr(Omega P) / d, d = 1 or 3; over all edges sum tr(Omega P) = n - lambda tr(Sigma), n of
 *                bos_system_info and the trace over the blocks of bos_marginals
 * Bearing edge i (pose p, landmark l, information omega, 1 where the problem gave none), every line one IEEE
 * operation at a time, without FP contraction:
 *   e    = bearing_error<double> (csrc/host/bos_math.hpp) at the fp64 master state with cos / sin computed in
 *          fp64, on every handle, fp32 ones included (as bos_cost and bos_associate_bearings)
 *   chi2 = (e * omega) * e
 *   var  = bit for bit the bearing_var[i] bos_edge_covariances returns at this state, with its fixed-pose rule
 *          (the same kernel's output, read in place)
 *   R = 1.0 / omega,  T = R - var,  w2 = (e * e) / T, NaN when T is not finite and > 0
 *   redundancy = 1.0 - omega * var
 * Odometry edge j (Omega is read as bos_create keeps it: the upper triangle u = (00, 01, 02, 11, 12, 22) of
 * odom_omega[j], mirrored):
 *   e    = the error of odometry_error_jacobian<double> at the fp64 master state, fp64 cos / sin
 *   chi2 = (e0 * Oe0 + e1 * Oe1) + e2 * Oe2 with Oe0 = (u00 * e0 + u01 * e1) + u02 * e2, Oe1 = (u01 * e0 +
 *          u11 * e1) + u12 * e2, Oe2 = (u02 * e0 + u12 * e1) + u22 * e2: the order of bos_cost's pass
 *   P    = bit for bit odom_cov[j] of bos_edge_covariances at this state, read in place
 *   R    = Omega^-1, formed once per edge on the host at the feature's first call by the code of
 *          bos_match_information_inverse (bos_host.h); an Omega it refuses (not finite, a pivot of its LDL^T not
 *          positive) gives an R of NaNs, hence w2 NaN
 *   T    = R - P entry-wise on the lower triangle
 *   w2   = e^T T^-1 e through the LDL^T of T: exactly the sequence written out for bos_match_poses with T in
 *          the place of S (the same function, csrc/host/match.hpp match_pose_nis); NaN when a pivot is not finite
 *          and > 0
 *   redundancy = 1.0 - t / 3.0, t the sum of Omega_ab * P_ab over a, b in row-major order, starting from 0.0
 * An odometry self-loop (src == dst) contributes nothing to H: its w2 and redundancy are NaN by definition, its
 * chi2 is evaluated like every other edge's.
 * Lists, per kind, k in 1 .. BOS_EDGE_CHECK_MAX_K: the min(k, n_over) LARGEST w2 among the edges whose w2 is
 * finite and >= the kind's gate, descending by w2, equal w2 to the lower edge index first; n_over counts all
 * edges that qualify, not min(., k). A gate is finite and >= 0; 0 lists every finite score.
 * Outputs (host pointers; any may be NULL: it is neither computed nor downloaded; edge = measurement order):
 *   cand_bearing            [k]     bearing index, -1 where nothing is listed
 *   cand_bearing_w2         [k]     -inf where nothing is listed; bit for bit bearing_w2[cand_bearing[j]]
 *   cand_bearing_innovation [k]     e of the listed bearing, 0 where nothing is listed
 *   cand_bearing_resvar     [k]     T of the listed bearing, 0 where nothing is listed
 *   n_over_bearing          [1]
 *   cand_odom, cand_odom_w2 [k]     likewise, indices among the odometry edges
 *   cand_odom_innovation    [k][3]  e
 *   cand_odom_rescov        [k][9]  T, row-major, its lower triangle mirrored
 *   n_over_odom             [1]
 *   bearing_w2, bearing_chi2, bearing_redundancy  [M_b]  the whole rows
 *   odom_w2, odom_chi2, odom_redundancy           [M_o]
 * A caller reproduces a listed w2 from the listed e and T with IEEE arithmetic.
 * BOS_ERR_INVALID, with nothing touched, for a gate that is NaN, negative or infinite and for k outside
 * 1 .. BOS_EDGE_CHECK_MAX_K. A kind without edges (M_b == 0 or M_o == 0) has lists of padding and a count of 0.
 * On a handle whose only node is the fixed pose (no landmark, hence no bearing, and every odometry edge a
 * self-loop) P is zero everywhere: the lists are padding, the counts 0, w2 and redundancy NaN, and chi2 is
 * evaluated on the host by the same code; *solver_info is 0.
 * One pass: the selected inverse with the cross blocks' emission and the projection kernel of
 * bos_edge_covariances into its buffers, one kernel with a thread per edge that reads bearing_var / odom_cov
 * in place and the fp64 measurements of bos_cost, then per kind the two selection launches of
 * bos_associate_bearings over the row of -w2. By default the lists alone are downloaded (1 872 bytes).
 * Exact rules: two calls give identical bits; duplicate edges of one orientation return identical bits; a
 * self-loop is never listed and never counted.
 * H_nf, the damping, the kernel threshold, the state handling, the synchronous behaviour, *solver_info, the
 * clearing of the pivot word, the "counts as a bos_linearize" rule and bos_get_last_dx afterwards are exactly
 * those of bos_edge_covariances. BOS_ERR_SOLVER on a stalled factorization; BOS_ERR_UNSUPPORTED and
 * BOS_ERR_DEVICE fire on exactly the conditions of bos_edge_covariances: the handle stays usable. The buffers
 * (with those of bos_edge_covariances and of bos_cost, if they have not run) are allocated at the first call
 * that asks for an output; a handle that never calls pays nothing. */
#define BOS_EDGE_CHECK_MAX_K BOS_ASSOC_MAX_K
int bos_edge_consistency(struct bos_solver* s, double gate_bearing, double gate_odom, int32_t k, int32_t* cand_bearing,
                         double* cand_bearing_w2, double* cand_bearing_innovation, double* cand_bearing_resvar,
                         int32_t* n_over_bearing, int32_t* cand_odom, double* cand_odom_w2, double* cand_odom_innovation,
                         double* cand_odom_rescov, int32_t* n_over_odom, double* bearing_w2, double* bearing_chi2,
                         double* bearing_redundancy, double* odom_w2, double* odom_chi2, double* odom_redundancy,
                         int32_t* solver_info);
/*
 * Levenberg-Marquardt with on-device step control (DESIGN.md §4 "Levenberg-Marquardt"). The objective is
 *   F(x) = sum over all edges of h(rho), rho = e^T Omega e, h(rho) = rho for rho <= kt and
 *   2 sqrt(kt rho) - kt beyond (Huber in squared form): the function whose half gradient the robust
 *   J+H build computes; with a kernel threshold past every rho it is the chi2 of bos_step_stats.
 * One iteration at state x with damping lambda: H = H0 + lambda I and b built at x (an iteration with
 * lambda = d is the linear system of a bos_step with damping factor d), H x_s = b solved (dx = -x_s),
 * predicted = dx^T (lambda dx - b), trial state x [+] dx, gain = (F - F') / predicted. The step is
 * accepted iff the factorization met no non-positive pivot, predicted > 0, F' is finite and gain > 0:
 * then lambda <- lambda max(1/3, 1 - (2 gain - 1)^3), nu <- 2; otherwise the state is rolled back,
 * lambda <- lambda nu, nu <- 2 nu. lambda stays in [lambda_min, lambda_max]. Stop tests, in this
 * order: 1 max |dx| <= dx_tol (an accepted step is kept, a rejected one is not), 2 accepted and
 * F - F' <= f_tol F, 4 rejected with lambda already at lambda_max, 3 max_iterations reached.
 * lambda, the gain, the decision and the rollback are device code: check_every iterations are
 * enqueued between two host reads of the status; after a stop the remaining iterations of a batch
 * change nothing (rejected, not counted).
 */
typedef struct bos_lm_options {
    double lambda0;        /* > 0: restart with this lambda and nu = 2; 0: continue from the handle's
                              last lambda/nu (first call: the handle's damping factor) */
    double lambda_min, lambda_max;   /* defaults 1e-12, 1e12 */
    double dx_tol, f_tol;            /* defaults 1e-6, 1e-12; 0 disables a test */
    int32_t max_iterations;          /* default 50; 1 .. 4096 */
    int32_t check_every;             /* iterations enqueued between host reads of the status, default 4 */
} bos_lm_options;
typedef struct bos_lm_iteration { double cost, cost_trial, predicted, gain, lambda, max_abs_dx;
                                  int32_t solver_info, accepted; } bos_lm_iteration;
typedef struct bos_lm_result { int32_t iterations, accepted, rejected, reason;
                               double cost_initial, cost_final, lambda_final; } bos_lm_result;
void bos_lm_default_options(bos_lm_options* opt);
/* F, the plain chi2 and the count of edges with rho > kt at the handle's current state and kernel
 * threshold; any output may be NULL. Evaluated in fp64 from the master state on every handle (fp32
 * ones included); no H is built, the last linearization stays as it is. Synchronous. Any one-GPU
 * handle (every solver); BOS_ERR_UNSUPPORTED on sharded handles. */
int bos_cost(struct bos_solver* s, double* cost, double* chi2, int32_t* n_robust);
/* Runs LM iterations until a stop test fires (result->reason, 1-4 above; options NULL: the
 * defaults). Synchronous. On return the state is the last accepted iterate. trace (may be NULL)
 * receives one record per counted iteration, the first min(iterations, trace_capacity) of them.
 * Afterwards bos_export_system gives the damped system of the last iteration that ran on the device
 * (the last counted one unless a batch went on past a stop: those re-linearise at the final state),
 * bos_get_last_dx returns BOS_ERR_INVALID until the next bos_step, and a following bos_step behaves
 * as if the state had been set with bos_set_state (its T caches are the box-plus kernel's, as after
 * a bos_step: on an fp32 handle their cos / sin can differ from bos_set_state's host-computed ones
 * by an ulp of fp32). The kernel threshold is the handle's; its damping
 * factor is not changed. A stalled factorization returns BOS_ERR_SOLVER with the state at the last
 * accepted iterate. BOS_ERR_UNSUPPORTED on BOS_SOLVER_DENSE_CHOL / BOS_SOLVER_ROCSOLVER_RF handles
 * and on sharded handles; BOS_ERR_DEVICE when the feature's buffers cannot be allocated: the handle
 * stays usable. */
int bos_optimize(struct bos_solver* s, const bos_lm_options* options, bos_lm_result* result,
                 bos_lm_iteration* trace, int32_t trace_capacity);
/*
 * Unary prior factors: a Gaussian prior (mean, information Omega) on single poses and single landmarks, added to
 * every H and b the handle builds (DESIGN.md §4 "Priors"). Each call REPLACES the handle's whole prior set;
 * n_pose == 0 && n_landmark == 0 clears it. The caller's arrays are copied. pose / landmark are node indices
 * (at most one prior per node and kind), pose_mean [n][3] = (x, y, theta), pose_omega [n][9] and
 * landmark_omega [n][4] row-major (the upper triangle is what is kept), landmark_mean [n][2].
 * Every line is one IEEE operation at a time, without FP contraction (csrc/host/prior.hpp, exported as
 * bos_prior_terms in bos_host.h). Pose prior at pose (x, y, theta), mean m, u = (00, 01, 02, 11, 12, 22) of Omega;
 * the perturbation is left-multiplicative, so J = [[1, 0, -y], [0, 1, x], [0, 0, 1]]:
 *   e0 = x - m0, e1 = y - m1, e2 = normalized_angle(theta - m2)
 *   Oe0 = (u00 e0 + u01 e1) + u02 e2, Oe1 = (u01 e0 + u11 e1) + u12 e2, Oe2 = (u02 e0 + u12 e1) + u22 e2
 *   rho = (e0 Oe0 + e1 Oe1) + e2 Oe2
 *   g = J^T Omega e:  g0 = Oe0, g1 = Oe1, g2 = ((-y) Oe0 + x Oe1) + Oe2
 *   q = Omega (-y, x, 1)^T:  q0 = ((-y) u00 + x u01) + u02, q1 = ((-y) u01 + x u11) + u12, q2 = ((-y) u02 + x u12) + u22
 *   A = J^T Omega J, lower triangle (00, 10, 11, 20, 21, 22) = (u00, u01, u11, q0, q1, ((-y) q0 + x q1) + q2)
 * Landmark prior at l, mean m, u = (00, 01, 11), J = I:
 *   e = l - m,  g0 = u00 e0 + u01 e1, g1 = u01 e0 + u11 e1,  rho = e0 g0 + e1 g1,  A = (u00, u01, u11)
 * Priors are not robustified (h(rho) = rho) and b accumulates J^T Omega e like every edge (H x_s = b, dx = -x_s).
 * The J+H build is followed by one kernel, a thread per prior, that forms A and g in the handle's precision
 * from the state caches the build reads and adds them to the node's diagonal block and b segment; a handle
 * without priors launches exactly what it launched before. Addition order: bos_step, bos_linearize and the
 * covariance calls build H = (sum over edges + damping) + A; bos_optimize builds (sum over edges + A) + lambda,
 * its lambda being added after the prior kernel. So on a handle with priors "an LM iteration with lambda = d is
 * the linear system of a bos_step with damping factor d" holds to rounding, not in its bits.
 * bos_step_stats.chi2, bos_cost's cost and chi2 and bos_optimize's F include the sum of rho over the priors (the
 * step's in the handle's precision, reduced in a fixed order; bos_cost's in fp64 from the master state);
 * n_robust does not count priors. Every covariance and gate call (bos_marginals, bos_edge_covariances,
 * bos_pair_covariances, bos_node_covariances, bos_associate_bearings, bos_match_*, bos_joint_compatibility,
 * bos_jcbb, bos_edge_consistency) sees H with the priors; nothing else about those calls changes. Priors are not
 * rows of bos_edge_consistency, and on a handle with priors the trace identity of its comment reads
 *   sum over edges tr(Omega P) + sum over priors tr(Omega_k J_k Sigma_kk J_k^T) = n - lambda tr(Sigma).
 * Priors survive bos_set_state, bos_triangulate and bos_optimize. The call drops the captured step graphs and
 * the captured LM iteration; the next step captures them again with the new set.
 * BOS_ERR_INVALID, with nothing touched, for: an index outside [0, num_poses) / [0, num_landmarks); a node
 * listed twice within its kind; the fixed pose; a mean that is not finite; an Omega that is not finite, not
 * bit-symmetric or has a negative diagonal entry. A semidefinite Omega (heading only, position only) is
 * allowed; an indefinite one is the caller's risk and shows in solver_info. Every one-GPU handle (all four
 * solvers, both precisions); BOS_ERR_UNSUPPORTED on sharded handles. BOS_ERR_DEVICE (bos_last_error names the
 * byte count) when the buffers cannot be allocated: the handle stays usable and keeps its previous set.
 */
int bos_set_priors(struct bos_solver* s, int32_t n_pose, const int32_t* pose, const double* pose_mean,
                   const double* pose_omega, int32_t n_landmark, const int32_t* landmark, const double* landmark_mean,
                   const double* landmark_omega);

/* Diagnostics: the phase boundaries of the last completed step, realtime clock (100 MHz ticks),
 * as the step's own kernels stamped them: [0] J+H start, [1] J+H end / solve start, [2] solve end,
 * [3] step end; subtree-sharded handles: [4] phase 0 done (own subtrees factored, exchange 1
 * starts), [5] exchange 1 received (replicated top starts), [6] phase 1 done (top factored and
 * solved, own subtrees solved backward; exchange 2 starts), [7] exchange 2 received (box-plus
 * starts). bench.py reports them per rank. */
int bos_last_step_stamps(const struct bos_solver* s, uint64_t stamps[8]);

#ifdef __cplusplus
}
#endif
#endif /* BOS_H_ */
