// Levenberg-Marquardt step control (include/bos.h bos_optimize): the objective's per-edge term, the
// accept / reject rule with its damping update, and the stop tests. One copy, plain C++ without
// intrinsics, called by the device decision kernel (hip/lm.hip), the CPU twin (host/cpu_baseline.cpp)
// and the host export bos_lm_rule_apply (tests), so the three cannot drift apart.
#pragma once

#include <cstdint>

#include "../../../include/bos.h"
#include "../../../include/bos_host.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define BOS_LM_HD __host__ __device__ inline
#else
#define BOS_LM_HD inline
#endif

namespace bos {

// stop reasons (bos_lm_result.reason, bos_lm_state.reason); 0 = still running
constexpr int32_t kLmStopDx = 1;         // max |dx| <= dx_tol
constexpr int32_t kLmStopCost = 2;       // accepted and F - F' <= f_tol F
constexpr int32_t kLmStopIterations = 3; // max_iterations reached
constexpr int32_t kLmStopLambda = 4;     // rejected with lambda already at lambda_max

// h(rho) of the objective F = sum h(rho_i): the function whose half gradient the robust J+H builds
// (e scaled by sqrt(kt / rho) beyond kt, H unscaled). sq = sqrt(kt * rho), computed by the caller.
BOS_LM_HD double lm_huber(double rho, double kt, double sq) { return rho <= kt ? rho : 2.0 * sq - kt; }

// One iteration's decision. s: the state before the iteration (lambda = the damping the system was
// built with, cost = F at the current iterate); cost_trial = F at x [+] dx, predicted = dx^T (lambda
// dx - b), max_dx = max |dx|, solver_info = the factorization's count of non-positive pivots.
// Returns true when the iteration counts (a record was written to *rec, which may be null); false
// once s.done is set: the state is then frozen, nothing is counted, the step is rejected.
// rec->accepted tells the caller whether to keep the trial state.
BOS_LM_HD bool lm_rule_apply(bos_lm_state& s, const bos_lm_options& o, double cost_trial, double predicted, double max_dx,
                             int32_t solver_info, bos_lm_iteration* rec) {
    if (s.done) {
        if (rec) rec->accepted = 0;
        return false;
    }
    const double F = s.cost, lambda_used = s.lambda;
    const bool finite = cost_trial - cost_trial == 0.0;   // false for +-inf and NaN
    const bool model_ok = solver_info == 0 && predicted > 0.0 && finite;
    const double gain = model_ok ? (F - cost_trial) / predicted : 0.0;
    const bool accept = model_ok && gain > 0.0;
    const bool at_max = s.lambda >= o.lambda_max;
    if (accept) {
        const double t = 2.0 * gain - 1.0;
        double f = 1.0 - t * t * t;
        if (f < 1.0 / 3.0) f = 1.0 / 3.0;
        s.lambda *= f;
        s.nu = 2.0;
        s.cost = cost_trial;
        s.accepted += 1;
    } else {
        s.lambda *= s.nu;
        s.nu *= 2.0;
        s.rejected += 1;
    }
    if (s.lambda < o.lambda_min) s.lambda = o.lambda_min;
    if (s.lambda > o.lambda_max) s.lambda = o.lambda_max;
    s.iteration += 1;
    if (o.dx_tol > 0.0 && max_dx <= o.dx_tol) s.reason = kLmStopDx;
    else if (accept && o.f_tol > 0.0 && F - cost_trial <= o.f_tol * F) s.reason = kLmStopCost;
    else if (!accept && at_max) s.reason = kLmStopLambda;
    else if (s.iteration >= o.max_iterations) s.reason = kLmStopIterations;
    s.done = s.reason != 0;
    if (rec) {
        rec->cost = F;
        rec->cost_trial = cost_trial;
        rec->predicted = predicted;
        rec->gain = gain;
        rec->lambda = lambda_used;
        rec->max_abs_dx = max_dx;
        rec->solver_info = solver_info;
        rec->accepted = accept ? 1 : 0;
    }
    return true;
}

BOS_LM_HD void lm_default_options(bos_lm_options& o) {
    o.lambda0 = 0.0;
    o.lambda_min = 1e-12;
    o.lambda_max = 1e12;
    o.dx_tol = 1e-6;
    o.f_tol = 1e-12;
    o.max_iterations = 50;
    o.check_every = 4;
}

}  // namespace bos
