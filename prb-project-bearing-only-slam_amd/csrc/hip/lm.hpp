// Device side of bos_cost / bos_optimize (hip/lm.hip): the fp64 objective, the damping added to the
// block array's diagonal, the model's predicted reduction, the state backup / rollback and the
// one-workgroup decision that applies host/lm_rule.hpp. Every kernel is a plain grid launch: no
// waits between workgroups, no atomics, every reduction in a fixed order.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "../host/lm_rule.hpp"

namespace bos {
namespace dev {

constexpr int kLmBlock = 256;
// workgroups of a partial-sum pass at most (each thread then strides over several items), and the
// width of the one-workgroup decision that sums the partials: one or two loads per thread and array
constexpr int kLmMaxParts = 1024;
constexpr int kLmDecideBlock = 1024;

// The LM loop's state on the device (one per handle); the host writes it before a bos_optimize call
// and reads its host-mapped copy after each batch of iterations.
struct LmControl {
    bos_lm_state st;
    bos_lm_options opt;
    double cost_eval, chi2;   // the last cost pass: F and the plain chi^2 ...
    double cost_start;        // F at the start of the bos_optimize call (mode 1 of the decision kernel)
    int32_t n_robust;         // ... and its count of edges with rho > kt
    int32_t restore;          // the last decision: 1 = rejected, the restore kernel copies the backup back
    int32_t aborted;          // a factorization stalled (kStepAbort): the loop is frozen, the call fails
    int32_t trace_cap;        // records the trace buffer holds
    int32_t seq;              // decisions taken so far; written to the host copy last
    int32_t pad;
};

// F, chi^2 and the robust count at the master state: the edges dealt to the threads in a fixed
// stride, bearings [0, Mb) in measurement order then odometry edges [Mb, Mb + Mo) (self-loops
// contribute nothing here: they are constants the caller adds), then the pose priors and the landmark
// priors (bos_set_priors; not robustified: F and chi^2 both gain rho), one partial of each per workgroup.
struct CostParams {
    int NP, NL, Mb, Mo;
    const double* pose;       // [NP][3]
    const double* lm;         // [NL][2]
    const int32_t* b_pose;    // [Mb]
    const int32_t* b_lm;      // [Mb]
    const double* b_z;        // [Mb]
    const double* b_w;        // [Mb] or null: 1
    const int32_t* o_src;     // [Mo]
    const int32_t* o_dst;     // [Mo]
    const double* o_z;        // [Mo][3]
    const double* o_om;       // [Mo][6] upper triangle (00, 01, 02, 11, 12, 22)
    // priors (host/prior.hpp), fp64: node of each (pose priors, then landmark priors), mean[3] + upper
    // triangle[6] per pose prior, mean[2] + upper triangle[3] per landmark prior
    int n_pose_priors = 0, n_lm_priors = 0;
    const int32_t* pr_idx = nullptr;
    const double* pr_pose = nullptr;
    const double* pr_lm = nullptr;
    double kt;
    double* part_F;           // [n_parts]
    double* part_chi;         // [n_parts]
    int32_t* part_nrob;       // [n_parts]
    int n_parts;              // workgroups: lm_cost_parts(Mb, Mo, priors)
};
inline int lm_parts(int64_t items) {
    const int64_t b = (items + kLmBlock - 1) / kLmBlock;
    return (int)(b < kLmMaxParts ? b : kLmMaxParts);
}
inline int lm_cost_parts(int64_t Mb, int64_t Mo, int64_t priors = 0) { return lm_parts(Mb + Mo + priors); }
hipError_t launch_lm_cost(const CostParams& p, hipStream_t s);

// Word copies of up to five arrays in one launch (the state and its T caches).
struct CopySet {
    uint32_t* dst[5];
    const uint32_t* src[5];
    int64_t words[5];
};

// hval[6 p + {0, 2, 5}] += (T)lambda for the pose of every J+H lane group, hval[off_ldiag + 3 l +
// {0, 2}] += (T)lambda for the landmark of every landmark lane: the blocks the J+H build writes. The
// same launch makes the state backup (the state does not change before the trial box-plus).
template <typename T>
hipError_t launch_lm_damping(T* hval, int64_t nval, int64_t off_ldiag, const int32_t* lane_pose, int n_groups, int NP,
                             const int32_t* lane_lm, int n_lm_lanes, int NL, const LmControl* ctl, const CopySet& backup,
                             hipStream_t s);

// Partials of x^T x and x^T b over the n solved dofs (x in elimination order, b in the reference
// numbering through elim_ref, nb entries): predicted = lambda x^T x + x^T b.
inline int lm_model_parts(int64_t n) { return lm_parts(n); }
template <typename T>
hipError_t launch_lm_model(const double* x, const T* b, const int32_t* elim_ref, int64_t n, int64_t nb, double* part_xx,
                           double* part_xb, hipStream_t s);

// The rollback: the copies are made when flag->restore is 1 (flag null: always).
hipError_t launch_lm_copy(const CopySet& c, const LmControl* flag, hipStream_t s);

struct DecideParams {
    const double* part_F;
    const double* part_chi;
    const int32_t* part_nrob;
    int n_cost;
    double F_const, chi_const;   // the odometry self-loops' constant terms
    int32_t nrob_const;
    const double* part_xx;
    const double* part_xb;
    int n_model;
    const double* max_part;      // box-plus max |dx| partials
    int n_max;
    int32_t* info;               // the solver's status word: read, then zeroed for the next factorization
    int lambda_fp32;             // the system was damped with (float)lambda
    LmControl* ctl;
    LmControl* mirror;           // host-mapped copy, or null
    bos_lm_iteration* trace;
    // 0: one LM iteration's decision; 1: the objective of the current state becomes st.cost (the start
    // of a bos_optimize call); 2: the objective alone (bos_cost)
    int mode;
};
hipError_t launch_lm_decide(const DecideParams& p, hipStream_t s);

}  // namespace dev
}  // namespace bos
