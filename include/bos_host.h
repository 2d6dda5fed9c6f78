/*
 * bos_host.h — host-side utilities of libbos.so (no GPU needed): the reference's g2o loader and
 * landmark triangulation, the synthetic world generator, and plan inspection for tests.
 *
 *   bos_dataset_load_g2o   <- parse_g2o           (utils/g2o_utils.hpp:29, g2o_utils.cpp:10-146)
 *                            + default fixed pose (executables/bearing_only_slam.cpp:63-65)
 *                            + triangulate_landmarks (slam/triangulation.hpp:8, triangulation.cpp:65-74)
 *   bos_dataset_write_g2o  <- (no reference counterpart: the checkpoint artefact of SURVEY.md §5)
 */
#ifndef BOS_HOST_H_
#define BOS_HOST_H_

#include "bos.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bos_dataset bos_dataset;

/* Parse a g2o file, default the fixed pose to the first pose and (if triangulate) append the
 * triangulated landmarks in ascending-id order. verbose prints the reference's warnings. */
int bos_dataset_load_g2o(const char* path, int triangulate, int verbose, bos_dataset** out);
/* Synthetic world: initial guess = dead-reckoned odometry chain, landmarks
 * triangulated from it; ground truth available through bos_dataset_ground_truth. */
int bos_dataset_synthetic(int32_t num_poses, int32_t num_landmarks, int32_t bearings_per_pose, uint64_t seed,
                          bos_dataset** out);
/* Problem view (pointers owned by the dataset, valid until bos_dataset_free). */
int bos_dataset_problem(const bos_dataset* ds, bos_problem* view);
const int32_t* bos_dataset_pose_ids(const bos_dataset* ds);
const int32_t* bos_dataset_landmark_ids(const bos_dataset* ds);
int32_t bos_dataset_fixed_pose_id(const bos_dataset* ds);
float bos_dataset_bound(const bos_dataset* ds);
/* Ground truth of a synthetic dataset in stix order; BOS_ERR_INVALID for loaded files. */
int bos_dataset_ground_truth(const bos_dataset* ds, const double** pose_xyt, const double** landmark_xy);
/* Write the dataset as g2o; pose_xyt / landmark_xy override the state (NULL = dataset state). */
int bos_dataset_write_g2o(const bos_dataset* ds, const char* path, const double* pose_xyt, const double* landmark_xy,
                          int with_landmarks);
void bos_dataset_free(bos_dataset* ds);

/* Solver::normalized_angle (slam/solver.hpp:50, slam/solver_jacobians.cpp:325-333): the wrap into
 * [-pi, pi) the kernels use (bos_math.hpp), compared in double as the reference does. An |a| past
 * ~1e15 (or an infinite one), on which the reference's loops never end, gives NaN. */
double bos_normalized_angle_f64(double a);
float bos_normalized_angle_f32(float a);

typedef struct bos_plan_info {
    int64_t n;
    int64_t nnz_lower;
    int64_t nnz_factor;
    int64_t num_block_values;       /* block array of H (J+H kernel layout)                      */
    int64_t lanes_per_pose;
    double flops_temporal;
    double flops_nested_dissection;
    char ordering[32];
    int64_t mf_supernodes;          /* multifrontal: supernodes / tree levels / largest front */
    int64_t mf_levels;
    int64_t mf_max_front;
    double mf_flops;
    int64_t mf_update_bytes;
    int64_t mf_fits;                /* Schur: every front fits the fast kernels (m <= 64, m <= 48 from level 2 up) */
    int64_t mf_max_front_upper;     /* Schur: largest front from tree level 2 up                  */
    int64_t mf_balance_pct;         /* Schur: separator balance of the plan kept (40 = first try)   */
    /* multi-GPU shard of rank `rank` (multifrontal solvers; one GPU: everything own, no top) */
    int64_t shard_own_fronts;       /* fronts of this rank's subtrees                             */
    int64_t shard_top_fronts;       /* fronts of the replicated top                               */
    int64_t shard_roots;            /* this rank's subtree roots below the top (exchange 1)       */
    int64_t shard_ex1_doubles;      /* exchange 1 buffer per rank (doubles)                        */
    int64_t shard_ex2_doubles;      /* exchange 2 buffer per rank (doubles)                        */
    int64_t shard_pose_lanes;       /* J+H pose lane groups (own, padding, top)                    */
    int64_t shard_own_pose_lanes;
    int64_t shard_lm_lanes;
    int64_t shard_update_nodes;     /* nodes the box-plus updates (own, top, boundary)             */
    int64_t mf_fold_fp32;           /* the folds alone read the pose-landmark / landmark-diagonal
                                       region (mf_fold_reads_fp32): an fp32 build's folds read it
                                       from the fp32 array (bos_system_info.fold_fp32)             */
    int64_t lm_lanes_consecutive;   /* J+H landmark lanes whose poses are consecutive (p0, p0 + 1,
                                       ...): they read no pose-index records                      */
    int64_t pose_odometry_chain;    /* poses whose odometry entries are exactly edges p - 1 = (p - 1,
                                       p) and p = (p, p + 1): the J+H derives them from p          */
} bos_plan_info;

/* Build the static plan on the host (what bos_create does before touching the GPU) with the
 * planning fields of `options` (NULL = bos_default_options): solver (BOS_SOLVER_*: it selects the
 * ordering), partition, lanes_per_pose, schur_leaf; its rank / world_size are ignored (the
 * arguments below give them).
 * If ref_rows/ref_cols/owned are given (capacity >= nnz_lower) they receive, for every stored
 * entry of the lower triangle of H_nf, its (row, col) in the reference dof numbering
 * (row >= col) and whether rank `rank` of `world` computes it (its J+H lanes write the block);
 * b_owned (n + 3 entries, indexed by reference dof) marks the b entries its lanes write;
 * perm_to_ref (n + 3 entries) maps the permuted dof order used on the device to reference dofs. */
int bos_plan_inspect(const bos_problem* problem, const bos_options* options, int32_t rank, int32_t world, int64_t capacity, int32_t* ref_rows,
                     int32_t* ref_cols, uint8_t* owned, uint8_t* b_owned, int32_t* perm_to_ref, bos_plan_info* info);

/* Test hook: the GPU multifrontal algorithm re-run on the host with the plan's tree and maps
 * (options->solver BOS_SOLVER_SUPERNODAL or _SCHUR; vals in the plan's CSR order, rhs/x in its permuted
 * dof order). Not used by any solve. */
int bos_plan_mf_selftest(const bos_problem* problem, const bos_options* options, const double* vals, const double* rhs, double* x);

/* Test hook: the marginal covariances bos_marginals computes, on the host: the host multifrontal
 * factorization of H_nf (vals in the plan's CSR order, as for bos_plan_mf_selftest) followed by the
 * selected-inverse recursion over the plan's tree. pose_cov [NP * 9] and landmark_cov [NL * 4],
 * row-major, stix order; the fixed pose's block is zero. options->solver BOS_SOLVER_SUPERNODAL or
 * _SCHUR; schur_leaf is honoured. */
int bos_plan_mf_marginals(const bos_problem* problem, const bos_options* options, const double* vals, double* pose_cov,
                          double* landmark_cov);

/* Test hook: what bos_edge_covariances computes, in its literal host form: the host factorization and
 * selected inverse of bos_plan_mf_marginals, every edge's cross block emitted through the plan's cross
 * records (csrc/host/plan.hpp selinv_cross_records), and the projection J Sigma_joint J^T by the very
 * code the device kernel runs (csrc/host/edge_cov.hpp), J evaluated at the problem's state
 * (problem->pose_xyt, problem->landmark_xy: both required). Outputs as for bos_edge_covariances; any
 * may be NULL. No device is used. */
int bos_plan_mf_edge_covariances(const bos_problem* problem, const bos_options* options, const double* vals,
                                 double* bearing_cross, double* odom_cross, double* bearing_var, double* odom_cov,
                                 double* pose_cov, double* landmark_cov);

/* Test hook: what bos_edge_consistency computes, in its literal host form: bearing_var / odom_cov of
 * bos_plan_mf_edge_covariances (the host selected inverse and the plan's cross records), then e, T, w2, chi2
 * and the redundancy of every edge by the code the device kernel runs (csrc/host/edge_check.hpp), at the
 * problem's state, Omega read by its upper triangle as bos_create keeps it, and the lists by a plain stable
 * sort (descending w2, equal w2 to the lower edge first). Arguments, outputs and rules as for
 * bos_edge_consistency (without solver_info); any output may be NULL. No device is used. */
int bos_plan_mf_edge_consistency(const bos_problem* problem, const bos_options* options, const double* vals, double gate_bearing,
                                 double gate_odom, int32_t k, int32_t* cand_bearing, double* cand_bearing_w2,
                                 double* cand_bearing_innovation, double* cand_bearing_resvar, int32_t* n_over_bearing,
                                 int32_t* cand_odom, double* cand_odom_w2, double* cand_odom_innovation, double* cand_odom_rescov,
                                 int32_t* n_over_odom, double* bearing_w2, double* bearing_chi2, double* bearing_redundancy,
                                 double* odom_w2, double* odom_chi2, double* odom_redundancy);

/* Test hook: what bos_pair_covariances computes, in its literal host form over the host factorization of
 * H_nf (vals as for bos_plan_mf_marginals): the same root-path walk per distinct node, the products
 * summed in row order, and the projection by the code the device kernel runs (csrc/host/pair_cov.hpp,
 * csrc/host/edge_cov.hpp), J evaluated at the problem's state. Ids, outputs and rules as for
 * bos_pair_covariances; any output may be NULL. No device is used. */
int bos_plan_mf_pair_covariances(const bos_problem* problem, const bos_options* options, const double* vals, int64_t n_pairs,
                                 const int32_t* node_a, const int32_t* node_b, double* cross, double* projected, double* cov_a,
                                 double* cov_b);

/* Test hook: what bos_node_covariances computes, in its literal host form over the host factorization of
 * H_nf (vals as for bos_plan_mf_marginals): per query node the root-path solve of
 * bos_plan_mf_pair_covariances, its rows scattered into the zeroed X, the backward substitution over every
 * front (levels from the root's down, then the folded landmarks; a pivot's sum from the front's last row
 * up), the host selected inverse for the diagonal blocks, and the gather and projection by the code the
 * device kernel runs (csrc/host/node_cov.hpp, csrc/host/edge_cov.hpp), J evaluated at the problem's state.
 * Ids, outputs and rules as for bos_node_covariances; any output may be NULL. No device is used. */
int bos_plan_mf_node_covariances(const bos_problem* problem, const bos_options* options, const double* vals, int32_t n_nodes,
                                 const int32_t* nodes, double* cross_pose, double* cross_landmark, double* projected_pose,
                                 double* projected_landmark, double* pose_cov, double* landmark_cov);

/* Test hook: what bos_associate_bearings computes, in its literal host form: per distinct pose the column of
 * bos_plan_mf_node_covariances for projected_landmark, then e, S and nis by the code the device kernels run
 * (csrc/host/associate.hpp), at the problem's state, and the selection by a plain sort over (nis, stix).
 * Arguments, outputs and rules as for bos_associate_bearings; any output may be NULL. No device is used. */
int bos_plan_mf_associate_bearings(const bos_problem* problem, const bos_options* options, const double* vals,
                                   int32_t n_bearings, const int32_t* pose, const double* z, const double* omega, double gate,
                                   int32_t k, int32_t* cand_landmark, double* cand_nis, double* cand_innovation,
                                   double* cand_var, int32_t* n_inside, double* nis_all);
/* Test constant: the landmarks one workgroup of bos_associate_bearings' first selection stage takes (a
 * world needs more than that to have a second tile). */
int32_t bos_associate_tile(void);

/* Test hooks: what bos_match_landmarks / bos_match_poses compute, in their literal host form: per distinct
 * query node the column of bos_plan_mf_node_covariances for projected_landmark / projected_pose, then the
 * differences, errors and scores by the code the device kernels run (csrc/host/match.hpp), at the problem's
 * state, and the selection by a plain sort over (score, stix). Arguments, outputs and rules as for the two
 * calls; any output may be NULL. No device is used. */
int bos_plan_mf_match_landmarks(const bos_problem* problem, const bos_options* options, const double* vals, int32_t n_queries,
                                const int32_t* landmark, double gate, int32_t k, int32_t* cand_landmark, double* cand_d2,
                                double* cand_diff, double* cand_cov, int32_t* n_inside, double* d2_all);
int bos_plan_mf_match_poses(const bos_problem* problem, const bos_options* options, const double* vals, int32_t n_meas,
                            const int32_t* pose, const double* z, const double* omega, double gate, int32_t k,
                            int32_t* cand_pose, double* cand_nis, double* cand_innovation, double* cand_cov, int32_t* n_inside,
                            double* nis_all);
/* Test hook: what bos_joint_compatibility computes, in its literal host form (csrc/host/joint.hpp): the host
 * factorization, one root-path solve per distinct node and the products in row order as in
 * bos_plan_mf_pair_covariances, then per hypothesis e, J, the entries of S through its block table, the
 * serial LDL^T recurrence and the prefixes, all by the functions the device kernel runs, at the problem's
 * state. Arguments, outputs and rules as for the call; any output may be NULL. max_batch > 0 closes a batch
 * at that many hypotheses (bos_debug_set_joint_batch). No device is used. */
int bos_plan_mf_joint_compatibility(const bos_problem* problem, const bos_options* options, const double* vals, int32_t n_hyp,
                                    const int32_t* hyp_start, const int32_t* pose, const int32_t* landmark, const double* z,
                                    const double* omega, int64_t max_batch, double* prefix_nis, double* joint_nis,
                                    double* innovation, double* innovation_cov);
/* Test hook: the serial search of bos_jcbb (csrc/host/jcbb.hpp jcbb_search) on a given all-pairings system: one
 * frame of m bearings with the candidate lists cand_start [m + 1] (cand_start[0] == 0) / cand_landmark [P],
 * S_all [P x P] row-major and e_all [P], gate [BOS_JOINT_MAX_M], max_nodes as for the call. no_bound != 0
 * switches the count and NIS bound off (the gate cut is the definition and stays). Outputs (any may be NULL):
 * assignment [m], *n_paired, *joint_nis, prefix_nis [m], *complete, *nodes (the nodes visited). The exact
 * oracle of the kernel's search on the kernel's own S. BOS_ERR_INVALID as for the call's lists, gates and
 * max_nodes (landmarks only need to be >= 0). No device is used. */
int bos_jcbb_search_host(int32_t m, const int32_t* cand_start, const int32_t* cand_landmark, const double* S_all, const double* e_all,
                         const double* gate, int64_t max_nodes, int32_t no_bound, int32_t* assignment, int32_t* n_paired,
                         double* joint_nis, double* prefix_nis, int32_t* complete, int64_t* nodes);
/* Test hook: what bos_jcbb computes, in its literal host form: the frames' all-pairings hypotheses through the
 * code of bos_plan_mf_joint_compatibility (max_batch as there), then the serial search per frame, at the
 * problem's state. Arguments, outputs and rules as for the call; any output may be NULL; nodes [n_frames]: the
 * nodes visited. No device is used. */
int bos_plan_mf_jcbb(const bos_problem* problem, const bos_options* options, const double* vals, int32_t n_frames,
                     const int32_t* frame_start, const int32_t* pose, const double* z, const double* omega, const int32_t* cand_start,
                     const int32_t* cand_landmark, const double* gate, int64_t max_nodes, int64_t max_batch, int32_t* assignment,
                     int32_t* n_paired, double* joint_nis, double* prefix_nis, int32_t* complete, double* innovation,
                     double* innovation_cov, int64_t* nodes);
/* R = omega^-1 as bos_match_poses forms it, bit for bit (csrc/host/match.hpp): the LDL^T of omega (row-major
 * 3 x 3), the lower triangle of L^-T D^-1 L^-1 evaluated and mirrored. BOS_ERR_INVALID, R untouched, when
 * omega is not finite, not bit-symmetric or has a pivot that is not positive. */
int bos_match_information_inverse(const double omega[9], double R[9]);

/* The root paths of node pairs, from the plan alone (no values, no device): out[5 * n_pairs] = per pair
 * the supernode of a, the supernode of b (-1: the fixed pose), the lowest common ancestor of the two (-1:
 * none, the nodes hang under two roots; -2: the pair involves the fixed pose), the dofs c the two paths
 * share (the pivots of the LCA and its ancestors; 0 without one) and the longer of the two paths, in
 * dofs. Ids as for bos_pair_covariances. */
int bos_plan_pair_paths(const bos_problem* problem, const bos_options* options, int64_t n_pairs, const int32_t* node_a,
                        const int32_t* node_b, int32_t* out);

/* The fronts of the plan's multifrontal tree, from the plan alone (no values, no device):
 * fronts[BOS_PLAN_FRONT_COLS * nsuper] = per supernode: k (own dofs), r (update rows), tree level
 * (leaves 0; -1 for a folded landmark, which is in no level), parent (-1 for a root), children
 * (folded ones included), folded children, 1 when the supernode itself is folded, and the selected
 * inverse's records of the front (csrc/host/plan.hpp selinv_records / selinv_cross_records): whole
 * nodes (diagonal blocks), cross records that read S_RJ, cross records that evaluate S_JJ, and how
 * many of either are transposed. fronts NULL with capacity 0: only *nsuper is returned. options as
 * for bos_plan_mf_selftest. */
enum { BOS_PLAN_FRONT_COLS = 11 };
int bos_plan_mf_fronts(const bos_problem* problem, const bos_options* options, int64_t capacity, int32_t* fronts,
                       int32_t* nsuper);

/* Owner of every node (NP poses, then NL landmarks) when the multifrontal solve is sharded over
 * `world` ranks: the rank, -1 for the replicated top, -2 for the fixed pose. */
int bos_plan_node_owner(const bos_problem* problem, const bos_options* options, int32_t world, int32_t* owner);

/* Test hook: the sharded GN solve (plan.hpp Shard) simulated on the host for all `world` ranks,
 * both exchanges included: per-rank plans, each rank's J+H outputs only, subtree factorization,
 * exchange 1, replicated top, backward, exchange 2. BOS_OK when the merged solution x (permuted
 * order, n) equals the one-rank solution bit for bit, the ranks agree on the top, every observation's
 * chi^2 is counted by one rank and every node a rank's J+H reads is kept current by its box-plus.
 * vals / rhs as for bos_plan_mf_selftest. */
int bos_plan_shard_selftest(const bos_problem* problem, const bos_options* options, int32_t world, const double* vals,
                            const double* rhs, double* x);

/* CPU baseline of bench.py (the build's own C++ CPU backend on the host's cores):
 * one GN iteration per bos_cpu_gn_step — J+H over the plan's lanes (fp64), the multifrontal
 * factorization and solves of the plan's tree with each level's fronts in parallel, box-plus — on
 * `threads` threads. A separate object: bos_create / bos_step never use it (no CPU fallback). */
typedef struct bos_cpu_gn bos_cpu_gn;
int bos_cpu_gn_create(const bos_problem* problem, int32_t solver, int32_t threads, bos_cpu_gn** out);
int bos_cpu_gn_step(bos_cpu_gn* c, double* chi2);
int bos_cpu_gn_get_state(const bos_cpu_gn* c, double* pose_xyt, double* landmark_xy);
void bos_cpu_gn_destroy(bos_cpu_gn* c);
/* The CPU twin of bos_cost / bos_optimize (include/bos.h) on the same object: the same objective,
 * iteration, options, result and trace, decided by the same rule code as the device's (kernel
 * threshold 1 and first lambda 0.01 unless set below). */
int bos_cpu_gn_set_kernel_threshold(bos_cpu_gn* c, double kt);
int bos_cpu_gn_cost(bos_cpu_gn* c, double* cost, double* chi2, int32_t* n_robust);
int bos_cpu_gn_optimize(bos_cpu_gn* c, const bos_lm_options* options, bos_lm_result* result, bos_lm_iteration* trace,
                        int32_t trace_capacity);
/* The CPU twin of bos_set_priors (include/bos.h): the same arguments, checks and "replace" semantics; the
 * object's step, cost and optimize then include the priors in fp64 through the same functions
 * (csrc/host/prior.hpp), added in the device's order (after the J+H build, before an LM iteration's lambda). */
int bos_cpu_gn_set_priors(bos_cpu_gn* c, int32_t n_pose, const int32_t* pose, const double* pose_mean, const double* pose_omega,
                          int32_t n_landmark, const int32_t* landmark, const double* landmark_mean,
                          const double* landmark_omega);
/* Test hook: the terms of one prior in fp64 by the functions the prior kernel, the cost pass and the CPU twin
 * call (csrc/host/prior.hpp; the formulas are written out at bos_set_priors). kind 0: a pose prior,
 * node_state = (x, y, theta), mean[3], omega[9] row-major, A[6] = (00, 10, 11, 20, 21, 22), g[3]. kind 1: a
 * landmark prior, node_state = (x, y), mean[2], omega[4], A[3] = (00, 10, 11), g[2]. Only the upper triangle
 * of omega is read. *rho = e^T Omega e. */
int bos_prior_terms(int32_t kind, const double* node_state, const double* mean, const double* omega, double* A, double* g,
                    double* rho);

/* The LM step control's state between two iterations (the device keeps one per handle). */
typedef struct bos_lm_state { double lambda, nu, cost; int32_t iteration, accepted, rejected, done, reason; } bos_lm_state;
/* Test hook: the accept / reject rule, damping update and stop tests of one LM iteration, the very
 * function the device decision kernel and the CPU twin call (csrc/host/lm_rule.hpp). Updates *state,
 * fills *record (may be NULL) and returns 1 when the iteration counted, 0 when state->done was
 * already set (nothing changes, the step is rejected), < 0 on a null argument. */
int bos_lm_rule_apply(bos_lm_state* state, const bos_lm_options* options, double cost_trial, double predicted,
                      double max_abs_dx, int32_t solver_info, bos_lm_iteration* record);

/* Benchmark helpers (bench.py; HIP events on the handle's stream, no torch):
 * bos_time_linearize: n J+H builds. flush_caches = 0: back to back, the average per build;
 * flush_caches = 1: 512 MiB (of two alternating buffers) are read before each build so its inputs
 * come from HBM (as inside a GN step); each build timed alone by its own pair of events.
 * bos_time_triangulate: n device triangulations back to back (re-estimates the landmarks).
 * bos_time_steps: n GN iterations, each exactly a bos_step call (launch, wait, status read and
 * checked), timed on the host clock in a C loop: the synchronous rate a C++ caller of the drop-in
 * (the reference's driver, executables/bearing_only_slam.cpp:95-98) sees, without a binding's
 * per-call overhead. */
int bos_time_linearize(struct bos_solver* s, int32_t n, int32_t flush_caches, double* ms_per_build);
int bos_time_triangulate(struct bos_solver* s, int32_t n, double* ms_per_call);
int bos_time_steps(struct bos_solver* s, int32_t n, double* ms_per_step);

/* Measurement helper (tools/marginals_time.py): the last bos_marginals call's split, ms[4] = J+H
 * build, factorization, selected inverse (HIP events on the handle's stream) and download of the
 * blocks (host clock); *sigma_bytes (may be NULL) = bytes of the Sigma-front buffer (0 before the
 * first call). */
int bos_marginals_timing(const struct bos_solver* s, double ms[4], int64_t* sigma_bytes);
/* Measurement helper (tools/edge_cov_time.py): the last bos_edge_covariances call's split, ms[5] = J+H
 * build, factorization, selected inverse with the cross blocks' emission, projection kernel (HIP
 * events) and download of the outputs (host clock); *edge_bytes (may be NULL) = bytes of the feature's
 * device buffers (0 before the first call). */
int bos_edge_covariances_timing(const struct bos_solver* s, double ms[5], int64_t* edge_bytes);
/* Measurement helper (tools/edge_consistency_time.py): the last bos_edge_consistency call's split, ms[7] = host
 * preparation (host clock; R and the arena at the first call), J+H build, factorization, selected inverse with
 * the cross blocks' emission, projection + scoring kernels, the selections (HIP events) and download of the
 * outputs (host clock); *bytes (may be NULL) = bytes of the feature's own arena (0 before the first call; the
 * edge call's buffers, which it reads, are bos_edge_covariances_timing's). */
int bos_edge_consistency_timing(const struct bos_solver* s, double ms[7], int64_t* bytes);
/* Measurement helper (tools/pair_cov_time.py): the last bos_pair_covariances call's split, ms[6] = host
 * preparation and upload (host clock), J+H build, factorization, path solve, product and projection (HIP
 * events, summed over the call's batches) and download of the outputs (host clock); *bytes (may be NULL)
 * = bytes of the feature's device buffers (0 before the first call). */
int bos_pair_covariances_timing(const struct bos_solver* s, double ms[6], int64_t* bytes);
/* Measurement helper (tools/node_cov_time.py): the last bos_node_covariances call's split, ms[7] = host
 * preparation and upload (host clock; the plan data and the arena at the first call), J+H build,
 * factorization, selected inverse (0 when the call did not run it), column solve (path solve, scatter and
 * backward sweep), gather + projection (HIP events, the last two summed over the call's nodes) and download
 * of the outputs (host clock); *bytes (may be NULL) = bytes of the feature's device buffers (0 before the
 * first call). */
int bos_node_covariances_timing(const struct bos_solver* s, double ms[7], int64_t* bytes);
/* Measurement helper (tools/associate_time.py): the last bos_associate_bearings call's split, ms[8] = host
 * preparation (host clock; the plan data and the buffers at the first call), J+H build, factorization,
 * selected inverse, column solve and gather (summed over the call's distinct poses), NIS kernel, selection
 * (HIP events, the last two summed over the call's chunks) and download of the outputs (host clock); *bytes
 * (may be NULL) = bytes of the feature's own device buffers (0 before the first call; the column's are
 * bos_node_covariances_timing's). */
int bos_associate_bearings_timing(const struct bos_solver* s, double ms[8], int64_t* bytes);
/* Test knob: bos_associate_bearings closes a chunk at max_bearings bearings of one pose instead of at its
 * byte budget alone; 0 restores the budget. */
int bos_debug_set_associate_chunk(struct bos_solver* s, int64_t max_bearings);
/* Measurement helper (tools/match_time.py): the split of the last bos_match_landmarks or bos_match_poses
 * call, whichever ran last, in the slots of bos_associate_bearings_timing: ms[8] = host preparation, J+H
 * build, factorization, selected inverse, column solve and gather (summed over the call's distinct nodes),
 * score kernel, selection (summed over the call's chunks) and download; *bytes (may be NULL) = bytes of the
 * feature's own device buffers (0 before the first call). */
int bos_match_timing(const struct bos_solver* s, double ms[8], int64_t* bytes);
/* Test knob: bos_match_poses closes a chunk at max_rows measurements of one pose instead of at its byte
 * budget alone; 0 restores the budget. (A landmark query is one row: it is a chunk of its own.) */
int bos_debug_set_match_chunk(struct bos_solver* s, int64_t max_rows);
/* Measurement helper (tools/joint_time.py): the split of the last bos_joint_compatibility call: ms[7] = host
 * preparation and upload, J+H build, factorization, path solve, products, NIS kernel (the last three summed
 * over the call's batches) and download; *bytes (may be NULL) = bytes of the device buffers the call uses
 * (its own and the pair call's arena; 0 before the first call of either). */
int bos_joint_compatibility_timing(const struct bos_solver* s, double ms[7], int64_t* bytes);
/* Test knob: bos_joint_compatibility closes a batch at max_hypotheses hypotheses instead of at its budgets
 * alone; 0 restores the budgets. */
int bos_debug_set_joint_batch(struct bos_solver* s, int64_t max_hypotheses);
/* Measurement helper (tools/jcbb_time.py): the split of the last bos_jcbb call in the slots of
 * bos_joint_compatibility_timing: ms[7] = host preparation and upload, J+H build, factorization, path solve,
 * products, assembly + search kernel (the last three summed over the call's batches) and download; *bytes (may
 * be NULL) = bytes of the device buffers the call uses (its own and the pair call's arena). nodes (may be
 * NULL, else capacity entries): the nodes the last call's search visited per frame, for its first
 * min(capacity, n_frames) frames; *n_frames (may be NULL): the frames of that call. */
int bos_jcbb_timing(const struct bos_solver* s, double ms[7], int64_t* bytes, int64_t capacity, int64_t* nodes, int32_t* n_frames);
/* Test knob: bos_jcbb closes a batch at max_frames frames instead of at its budgets alone; 0 restores the
 * budgets. */
int bos_debug_set_jcbb_batch(struct bos_solver* s, int64_t max_frames);
/* Test knob: bos_pair_covariances closes a batch at max_distinct_nodes distinct nodes (at least one pair
 * per batch) instead of at its byte budget alone; 0 restores the budget. */
int bos_debug_set_pair_batch(struct bos_solver* s, int64_t max_distinct_nodes);
/* Measurement helper (tools/lm_time.py): n launches of bos_cost's kernel back to back between two
 * HIP events on the handle's stream: *ms_per_pass. */
int bos_time_cost(struct bos_solver* s, int32_t n, double* ms_per_pass);

/* The C++ façade proj02::Solver (prb-project-bearing-only-slam_amd/csrc/host/solver.hpp, the
 * reference's class API, slam/solver.hpp:21-92) driven as the reference's executable drives it
 * (executables/bearing_only_slam.cpp:93-99: solver.step() in a loop, then one read of solver.state
 * to draw it). The façade is built from `problem` (ids = stix); one untimed step, then n
 * Solver::step() calls timed on the host clock: *ms_per_step. *ms_state_read: the one read of
 * solver.state after them (its lazy download of the device state). *mismatches: doubles of
 * solver.state whose bits differ from bos_get_state of the façade's handle. *ms_per_step_capi: n
 * bos_step calls on the same handle right after (bos_time_steps). Optional outputs may be NULL. */
int bos_time_facade_steps(const bos_problem* problem, const bos_options* options, int32_t n, double* ms_per_step,
                          double* ms_state_read, double* ms_per_step_capi, int64_t* mismatches);
/* Test hook: n steps of the façade beside n bos_step calls of a second handle created from the same
 * problem, solver.state read every 7 steps and written once (a landmark moved, a pose turned:
 * through the façade's public state, by bos_get_state / bos_set_state on the other handle) at n / 2.
 * *mismatches = doubles of solver.state that differ in their bits from the device states at the
 * reads and at the end (0 expected). */
int bos_debug_facade_selftest(const bos_problem* problem, const bos_options* options, int32_t n, int64_t* mismatches);

/* Test hook (process-wide, default 0 = product behaviour; not part of the drop-in boundary): the
 * line-by-line g2o parser instead of the chunked one (the tests prove them identical). */
void bos_debug_set_g2o_parser(int32_t line_by_line);
/* Test hook: the next bos_step's factor dataflow launch skips its first front, so a dependency
 * wait times out — bos_step must then fail with BOS_ERR_SOLVER and leave the state untouched.
 * BOS_ERR_UNSUPPORTED when the handle's solver has no dataflow launch. */
int bos_debug_inject_stall(struct bos_solver* s);
/* Test hook: run the one-GPU GN step as individual launches (enable = 0) instead of the captured
 * hipGraph replay (1, default). The same kernels in the same order either way. */
int bos_debug_set_step_graph(struct bos_solver* s, int32_t enable);
/* Diagnostics: one GN step (individual launches) whose multifrontal dataflow launches stamp every
 * front they process: stamps[16 * nsuper] = factor stamps [nsuper][8] (start, folded, assembled,
 * children ready, extend-added, factored, written, published), then backward stamps [nsuper][8]
 * (start, staged, parent ready, solved, published; 0 = not in a flow launch); realtime clock,
 * 100 MHz. meta[4 * nsuper] = tree level (-1 folded), k, r, folded children. */
int bos_debug_solver_stamps(struct bos_solver* s, int64_t capacity, uint64_t* stamps, int32_t* meta);

/* Diagnostics: the kernel route every front of the multifrontal tree takes in this handle's launch
 * sequence. One value per launch site of the factorization (mf_factor_t) and of the backward
 * substitution (mf_solve) in hip/multifrontal.hip (the kernels they launch are in hip/mf_level.hpp,
 * mf_blk.hpp, mf_wave.hpp and mf_backward.hpp); the launch sites themselves note it, with the
 * front list they launch, the first time the sequence is enqueued (a replayed graph enqueues it
 * once, at capture). Nothing is launched or changed by the call. */
enum {
    BOS_ROUTE_NONE = -1,          /* no launch of this handle processes the front (another rank's)   */
    BOS_ROUTE_F_REG16 = 0,        /* mf_factor_reg<16>, main stream                                   */
    BOS_ROUTE_F_REG16_SIDE = 1,   /* mf_factor_reg<16> behind the class-64 launch on the side stream */
    BOS_ROUTE_F_PAN48 = 2,        /* class-48 launch (17-48 rows): mf_factor_pan<48>                  */
    BOS_ROUTE_F_PAN64 = 3,        /* class-64 launch (49-64 rows): mf_factor_pan<64>, main stream     */
    BOS_ROUTE_F_PAN64_SIDE = 4,   /* the same on the side stream                                     */
    BOS_ROUTE_F_BLK = 5,          /* mf_factor_blk (65-128 rows), main stream                         */
    BOS_ROUTE_F_BLK_SIDE2 = 6,    /* mf_factor_blk on the second side stream                          */
    BOS_ROUTE_F_MIXB_BLK = 7,     /* mf_factor_mixb, a blocked front                                  */
    BOS_ROUTE_F_MIXB_WAVE = 8,    /* mf_factor_mixb, a wave front                                     */
    BOS_ROUTE_F_LEVEL = 9,        /* mf_factor_level + mf_forward_level (above 128 rows)              */
    BOS_ROUTE_F_FLOW = 10,        /* mf_factor_flow (dataflow launch over the top of the tree)        */
    BOS_ROUTE_F_FOLDED = 11,      /* a landmark folded into its parent front by the parent's kernel   */
    BOS_ROUTE_F_COUNT = 12
};
enum {
    BOS_ROUTE_B_FLOW = 0,         /* mf_backward_flow  */
    BOS_ROUTE_B_WAVE = 1,         /* mf_backward_wave  */
    BOS_ROUTE_B_LEVEL = 2,        /* mf_backward_level */
    BOS_ROUTE_B_FOLD = 3,         /* mf_backward_fold  */
    BOS_ROUTE_B_COUNT = 4
};
/* routes[4 * nsuper] = per front: factor route, backward route, k (columns), r (update rows); fronts
 * in the plan's supernode order; *nsuper (may be NULL) = their number. routes NULL with capacity 0:
 * only *nsuper is returned. BOS_ERR_UNSUPPORTED for a handle without the multifrontal solver,
 * BOS_ERR_INVALID before the handle's first bos_step (the sequence has not been enqueued yet) or
 * when capacity < 4 * nsuper. */
int bos_debug_solver_routes(struct bos_solver* s, int64_t capacity, int32_t* routes, int32_t* nsuper);

/* Diagnostics: what the selected inverse's launch plan (hip/selinv.hip selinv_build) decided for every
 * front, from the plan this handle built at its first bos_marginals / bos_edge_covariances call. The
 * class is noted where selinv_build chooses the front's thread count and its workspace slice; nothing
 * is launched or changed by the call. */
enum {
    BOS_SELINV_WAVE_LDS = 0,       /* one wavefront, the working set in LDS (m <= 64; folded landmarks too) */
    BOS_SELINV_BLK_LDS_MFMA = 1,   /* 256 threads, the working set in LDS, G Z on f64 MFMA tiles (65-128)  */
    BOS_SELINV_BLK_WORKSPACE = 2,  /* 256 threads, Li / Z / S_RJ in the global workspace, G read in place   */
    BOS_SELINV_CLASS_COUNT = 3
};
enum { BOS_SELINV_COLS = 10 };
/* fronts[BOS_SELINV_COLS * nsuper] = per front, in the plan's supernode order: class, index of its
 * launch in the pass, k, r, 1 when it is a folded landmark (in fold_list), 1 when it stores a Sigma
 * front for its children, its diagonal-block records (whole nodes), and, once the cross records exist
 * (after the first bos_edge_covariances; -1 before), its cross records that read S_RJ, those that
 * evaluate S_JJ, and how many of either are transposed. node_front[NP + NL] (may be NULL) = the front
 * whose records write each node's block (poses, then landmarks; -1 for the fixed pose); edge_front
 * [Mb + Mo] (may be NULL) = the front whose cross record emits each edge's cross block (bearings, then
 * odometry; -1 when the edge involves the fixed pose or the cross records do not exist yet). fronts
 * NULL with capacity 0: only *nsuper is returned. BOS_ERR_UNSUPPORTED for a handle without the
 * multifrontal solver, BOS_ERR_INVALID before the first bos_marginals / bos_edge_covariances call or when
 * capacity < BOS_SELINV_COLS * nsuper. */
int bos_debug_selinv_fronts(struct bos_solver* s, int64_t capacity, int32_t* fronts, int32_t* nsuper, int32_t* node_front,
                            int32_t* edge_front);

/* Diagnostics: one J+H launch with per-wave timeline stamps, 8 x uint64 per wave: block, wave in
 * block, kind (0 pose lanes / 1 landmark lanes), t_start, t_loop, t_loop_end, t_end (realtime clock,
 * 100 MHz ticks), hw_id | xcc_id << 32. capacity in waves; *n_waves = waves of the launch;
 * flush_caches = 1: 512 MiB read before the launch (inputs from HBM, as in a GN step). Not part
 * of the drop-in boundary; the product launches never carry stamps. */
int bos_debug_linearize_timeline(struct bos_solver* s, int64_t capacity, uint64_t* stamps, int64_t* n_waves,
                                 int32_t flush_caches);

#ifdef __cplusplus
}
#endif
#endif /* BOS_HOST_H_ */
