// CPU baseline of bench.py ("the build's own C++ CPU backend"):
// one Gauss-Newton iteration of the reference's Solver::step (slam/solver.cpp:27-97) on the host's
// cores, with the same static plan as the GPU path —
//   * J+H: every pose lane and landmark lane of the plan (host/plan.hpp BlockLayout) evaluated in
//     parallel over poses / landmarks, written into the same block array (fp64),
//   * sparse Cholesky: the multifrontal algorithm of hip/multifrontal.hip on the host (host/host_mf.hpp),
//     the fronts of each tree level in parallel,
//   * box-plus in parallel.
// Timed by bench.py only; bos_create / bos_step never use it (the product has no CPU fallback).
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "../../../include/bos_host.h"
#include "bos_math.hpp"
#include "error.hpp"
#include "host_mf.hpp"
#include "lm_rule.hpp"
#include "plan.hpp"
#include "prior.hpp"
#include "prior_set.hpp"

struct bos_cpu_gn {
    bos::Plan plan;
    std::unique_ptr<bos::Pool> pool;
    std::unique_ptr<bos::HostMf> mf;
    int NP = 0, NL = 0;
    std::vector<double> pose, lm, b;
    std::vector<int32_t> b_pose, b_lm, o_src, o_dst;
    std::vector<double> b_z, b_w, o_z, o_om;   // o_om: upper triangle (00, 01, 02, 11, 12, 22)
    double kt = 1.0, damping = 0.01;
    bos::PriorSet priors;   // bos_cpu_gn_set_priors
    // bos_cpu_gn_optimize: the last call's final lambda / nu (lambda0 = 0 continues from them)
    bool lm_started = false;
    double lm_lambda = 0.0, lm_nu = 2.0;
};

namespace {

int cfail(int code, const std::string& m) { return bos::set_error(code, m); }

// J+H of one pose lane group (all of its lanes) and of one landmark lane, as hip/kernels.hip
// pose_lanes / landmark_lane compute them (fp64)
void jh_pose(bos_cpu_gn* c, int grp, double& chi) {
    const bos::Plan& P = c->plan;
    const bos::BlockLayout& B = P.blk;
    const int p = B.lane_pose[grp];
    if (p < 0) return;
    const double X = c->pose[3 * p], Y = c->pose[3 * p + 1], th = c->pose[3 * p + 2];
    const double cs = std::cos(th), ss = std::sin(th);
    double h[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    double* hv = c->mf->hval.data();
    for (int sub = 0; sub < B.lpp; ++sub) {
        const int lane = grp * B.lpp + sub;
        const int n = B.pose_lanes.cnt[lane];
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int j = 0; j < n; ++j) {
            const int32_t sl = B.pose_lanes.slot(lane, j);
            const int k = B.pose_lanes.obs[sl];
            const int l = c->b_lm[k];
            double J[5];
            double e = bos::bearing_error_jacobian<double>(X, Y, cs, ss, c->lm[2 * l], c->lm[2 * l + 1], c->b_z[k], J);
            const double w = c->b_w.empty() ? 1.0 : c->b_w[k];
            const double rho = e * w * e;
            chi += rho;
            if (rho > c->kt) e *= std::sqrt(c->kt / rho);
            const double w0 = J[0] * w, w1 = J[1] * w, w2 = J[2] * w;
            h[0] += w0 * J[0]; h[1] += w1 * J[0]; h[2] += w1 * J[1];
            h[3] += w2 * J[0]; h[4] += w2 * J[1]; h[5] += w2 * J[2];
            g[0] += w0 * e; g[1] += w1 * e; g[2] += w2 * e;
            const double o[6] = {w0 * J[3], w0 * J[4], w1 * J[3], w1 * J[4], w2 * J[3], w2 * J[4]};
            for (int q = 0; q < 6; ++q) acc[q] += o[q];
            const bool last = j + 1 == n ||
                              c->b_lm[B.pose_lanes.obs[B.pose_lanes.slot(lane, j + 1)]] != l;
            if (last) {
                double* dst = hv + B.off_pl + 6 * (int64_t)sl;
                for (int q = 0; q < 6; ++q) { dst[q] = acc[q]; acc[q] = 0.0; }
            }
        }
    }
    double acc6[6] = {0, 0, 0, 0, 0, 0};
    for (int x = B.po_ptr[p]; x < B.po_ptr[p + 1]; ++x) {
        const int e = B.po_ent[x], k = e >> 1;
        const bool dst = e & 1;
        const int s = c->o_src[k], d = c->o_dst[k];
        const double* zs = c->o_z.data() + 3 * (size_t)k;
        const double* u = c->o_om.data() + 6 * (size_t)k;
        double E[3], J[18];
        bos::odometry_error_jacobian<double>(c->pose[3 * s], c->pose[3 * s + 1], c->pose[3 * s + 2],
                                             std::cos(c->pose[3 * s + 2]), std::sin(c->pose[3 * s + 2]), c->pose[3 * d],
                                             c->pose[3 * d + 1], c->pose[3 * d + 2], zs[0], zs[1], zs[2], E, J);
        const double Om[3][3] = {{u[0], u[1], u[2]}, {u[1], u[3], u[4]}, {u[2], u[4], u[5]}};
        double Oe[3];
        for (int i = 0; i < 3; ++i) Oe[i] = Om[i][0] * E[0] + Om[i][1] * E[1] + Om[i][2] * E[2];
        const double rho = E[0] * Oe[0] + E[1] * Oe[1] + E[2] * Oe[2];
        if (rho > c->kt) {
            const double sc = std::sqrt(c->kt / rho);
            for (int i = 0; i < 3; ++i) Oe[i] *= sc;
        }
        if (!dst) chi += rho;
        // H_ss = J_s^T Omega J_s (J_d = -J_s), b_s = J_s^T Omega e
        double Hs[3][3], bs[3];
        for (int a = 0; a < 3; ++a) {
            for (int b2 = 0; b2 < 3; ++b2) {
                double v = 0.0;
                for (int i = 0; i < 3; ++i)
                    for (int jj = 0; jj < 3; ++jj) v += J[6 * i + a] * Om[i][jj] * J[6 * jj + b2];
                Hs[a][b2] = v;
            }
            bs[a] = J[a] * Oe[0] + J[6 + a] * Oe[1] + J[12 + a] * Oe[2];
        }
        const double hl[6] = {Hs[0][0], Hs[1][0], Hs[1][1], Hs[2][0], Hs[2][1], Hs[2][2]};
        for (int q = 0; q < 6; ++q) h[q] += hl[q];
        for (int q = 0; q < 3; ++q) g[q] += dst ? -bs[q] : bs[q];
        const int blk = B.po_blk[x];
        if (blk >= 0) {
            for (int q = 0; q < 6; ++q) acc6[q] -= hl[q];
            if (x + 1 == B.po_ptr[p + 1] || B.po_blk[x + 1] != blk) {
                double* dstp = hv + B.off_pp + 6 * (int64_t)blk;
                for (int q = 0; q < 6; ++q) { dstp[q] = acc6[q]; acc6[q] = 0.0; }
            }
        }
    }
    double* hp = hv + 6 * (int64_t)p;
    const double lam = c->damping;
    hp[0] = h[0] + lam; hp[1] = h[1]; hp[2] = h[2] + lam; hp[3] = h[3]; hp[4] = h[4]; hp[5] = h[5] + lam;
    for (int q = 0; q < 3; ++q) c->b[3 * (size_t)p + q] = g[q];
}

void jh_landmark(bos_cpu_gn* c, int lane) {
    const bos::BlockLayout& B = c->plan.blk;
    const int l = B.lm_lane_lm[lane];
    const double lx = c->lm[2 * l], ly = c->lm[2 * l + 1];
    double h[3] = {0, 0, 0}, g[2] = {0, 0};
    for (int j = 0; j < B.lm_lanes.cnt[lane]; ++j) {
        const int k = B.lm_lanes.obs[B.lm_lanes.slot(lane, j)];
        const int p = c->b_pose[k];
        const double th = c->pose[3 * p + 2];
        double J[5];
        double e = bos::bearing_error_jacobian<double>(c->pose[3 * p], c->pose[3 * p + 1], std::cos(th), std::sin(th), lx,
                                                       ly, c->b_z[k], J);
        const double w = c->b_w.empty() ? 1.0 : c->b_w[k];
        const double rho = e * w * e;
        if (rho > c->kt) e *= std::sqrt(c->kt / rho);
        const double w3 = J[3] * w, w4 = J[4] * w;
        h[0] += w3 * J[3]; h[1] += w4 * J[3]; h[2] += w4 * J[4];
        g[0] += w3 * e; g[1] += w4 * e;
    }
    double* hp = c->mf->hval.data() + B.off_ldiag + 3 * (int64_t)l;
    hp[0] = h[0] + c->damping; hp[1] = h[1]; hp[2] = h[2] + c->damping;
    c->b[3 * (size_t)c->NP + 2 * (size_t)l] = g[0];
    c->b[3 * (size_t)c->NP + 2 * (size_t)l + 1] = g[1];
}

}  // namespace

extern "C" {

int bos_cpu_gn_create(const bos_problem* pb, int32_t solver, int32_t threads, bos_cpu_gn** out) {
    if (!pb || !out) return cfail(BOS_ERR_INVALID, "null argument");
    if (solver != BOS_SOLVER_SCHUR && solver != BOS_SOLVER_SUPERNODAL)
        return cfail(BOS_ERR_INVALID, "the CPU baseline runs the multifrontal solvers");
    *out = nullptr;
    std::unique_ptr<bos_cpu_gn> c(new bos_cpu_gn());
    bos::ProblemIndex pi;
    pi.NP = pb->num_poses; pi.NL = pb->num_landmarks; pi.Mb = pb->num_bearings; pi.Mo = pb->num_odometry;
    pi.fixed = pb->fixed_pose;
    pi.b_pose = pb->bearing_pose; pi.b_lm = pb->bearing_landmark; pi.o_src = pb->odom_src; pi.o_dst = pb->odom_dst;
    pi.b_omega = pb->bearing_omega; pi.o_omega = pb->odom_omega;
    std::string err;
    const int rc = bos::build_plan(pi, 0, 1, solver == BOS_SOLVER_SCHUR ? bos::kFactorSchur : bos::kFactorMultifrontal,
                                   c->plan, err);
    if (rc) return cfail(rc, err);
    c->NP = pi.NP;
    c->NL = pi.NL;
    c->pose.assign(pb->pose_xyt, pb->pose_xyt + 3 * (size_t)pi.NP);
    for (int i = 0; i < pi.NP; ++i) c->pose[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(c->pose[3 * i + 2]));
    if (!pb->landmark_xy && pi.NL) return cfail(BOS_ERR_INVALID, "the CPU baseline needs landmark positions");
    c->lm.assign(pb->landmark_xy, pb->landmark_xy + 2 * (size_t)pi.NL);
    c->b.assign(3 * (size_t)pi.NP + 2 * (size_t)pi.NL, 0.0);
    c->b_pose.assign(pi.b_pose, pi.b_pose + pi.Mb);
    c->b_lm.assign(pi.b_lm, pi.b_lm + pi.Mb);
    c->b_z.assign(pb->bearing_z, pb->bearing_z + pi.Mb);
    if (pb->bearing_omega) c->b_w.assign(pb->bearing_omega, pb->bearing_omega + pi.Mb);
    c->o_src.assign(pi.o_src, pi.o_src + pi.Mo);
    c->o_dst.assign(pi.o_dst, pi.o_dst + pi.Mo);
    c->o_z.assign(pb->odom_z, pb->odom_z + 3 * (size_t)pi.Mo);
    c->o_om.resize(6 * (size_t)pi.Mo);
    for (int k = 0; k < pi.Mo; ++k) {
        const double* m = pb->odom_omega + 9 * (size_t)k;
        const double u[6] = {m[0], m[1], m[2], m[4], m[5], m[8]};
        std::memcpy(&c->o_om[6 * (size_t)k], u, sizeof(u));
    }
    c->pool.reset(new bos::Pool(std::max(1, threads)));
    c->mf.reset(new bos::HostMf(c->plan, c->pool.get()));
    *out = c.release();
    return BOS_OK;
}

}  // extern "C"

namespace {

// J+H into the block array and b; returns chi^2
double cpu_build(bos_cpu_gn* c) {
    const bos::Plan& P = c->plan;
    bos::Pool& pool = *c->pool;
    const int G = (int)P.blk.lane_pose.size(), NLL = (int)P.blk.lm_lane_lm.size();
    // J+H (self-loops: chi^2 only, their Jacobian is zero; see host/plan.cpp build_layout)
    std::vector<double> chi_part(G, 0.0);
    pool.parallel_for(G, [&](int64_t i) { jh_pose(c, (int)i, chi_part[i]); });
    pool.parallel_for(NLL, [&](int64_t i) { jh_landmark(c, (int)i); });
    double chi = 0.0;
    for (double v : chi_part) chi += v;
    // the priors onto the diagonal blocks and b just written (host/prior.hpp), as the device's prior kernel
    double* hv = c->mf->hval.data();
    const bos::PriorSet& R = c->priors;
    for (size_t i = 0; i < R.pose.size(); ++i) {
        const int p = R.pose[i];
        const double* r = &R.pose_rec[9 * i];
        double A[6], g[3];
        chi += bos::prior_pose_terms<double>(c->pose[3 * (size_t)p], c->pose[3 * (size_t)p + 1], c->pose[3 * (size_t)p + 2], r, r + 3, A, g);
        for (int q = 0; q < 6; ++q) hv[6 * (int64_t)p + q] += A[q];
        for (int q = 0; q < 3; ++q) c->b[3 * (size_t)p + q] += g[q];
    }
    for (size_t i = 0; i < R.lm.size(); ++i) {
        const int l = R.lm[i];
        const double* r = &R.lm_rec[5 * i];
        double A[3], g[2];
        chi += bos::prior_landmark_terms<double>(c->lm[2 * (size_t)l], c->lm[2 * (size_t)l + 1], r, r + 2, A, g);
        for (int q = 0; q < 3; ++q) hv[P.blk.off_ldiag + 3 * (int64_t)l + q] += A[q];
        for (int q = 0; q < 2; ++q) c->b[3 * (size_t)c->NP + 2 * (size_t)l + q] += g[q];
    }
    for (int k = 0; k < (int)c->o_src.size(); ++k)
        if (c->o_src[k] == c->o_dst[k]) {
            const double* z = &c->o_z[3 * (size_t)k];
            const double* u = &c->o_om[6 * (size_t)k];
            const double e[3] = {-z[0], -z[1], bos::normalized_angle<double>(-z[2])};
            const double Oe[3] = {u[0] * e[0] + u[1] * e[1] + u[2] * e[2], u[1] * e[0] + u[3] * e[1] + u[4] * e[2],
                                  u[2] * e[0] + u[4] * e[1] + u[5] * e[2]};
            chi += e[0] * Oe[0] + e[1] * Oe[1] + e[2] * Oe[2];
        }
    return chi;
}

// permuted dof -> reference dof
std::vector<int32_t> cpu_ref_dof(const bos_cpu_gn* c) {
    const bos::Plan& P = c->plan;
    std::vector<int32_t> ref(P.n);
    for (int u = 0; u < c->NP + c->NL; ++u) {
        if (u == P.fixed) continue;
        const int sz = u < c->NP ? 3 : 2;
        const int r0 = u < c->NP ? 3 * u : 3 * c->NP + 2 * (u - c->NP);
        for (int d = 0; d < sz; ++d) ref[P.node_dof[u] + d] = r0 + d;
    }
    return ref;
}

// solve H_nf x = b_nf (rhs in elimination order), dx = -x; returns the count of non-positive pivots
int cpu_solve(bos_cpu_gn* c, const std::vector<int32_t>& ref) {
    bos::HostMf& M = *c->mf;
    for (int64_t i = 0; i < c->plan.n; ++i) M.x[i] = c->b[ref[i]];
    auto all = [](int) { return true; };
    M.nonpos = 0;
    M.factor(all);
    M.forward(all);
    M.backward(all);
    return M.nonpos;
}

// box-plus (framework/state.cpp:69-80); returns max |dx| (NaN if the update is not finite)
double cpu_update(bos_cpu_gn* c) {
    const bos::Plan& P = c->plan;
    bos::HostMf& M = *c->mf;
    double m = 0.0;
    for (int64_t i = 0; i < P.n; ++i) {
        const double a = std::fabs(M.x[i]);
        m = (a != a || m != m) ? a + m : std::max(m, a);
    }
    c->pool->parallel_for(c->NP + c->NL, [&](int64_t u) {
        if (u == P.fixed) return;
        const int d = P.node_dof[u];
        if (u < c->NP) {
            double* p = &c->pose[3 * u];
            bos::boxplus_pose<double>(p[0], p[1], p[2], -M.x[d], -M.x[d + 1], -M.x[d + 2]);
        } else {
            double* l = &c->lm[2 * (u - c->NP)];
            l[0] += -M.x[d];
            l[1] += -M.x[d + 1];
        }
    });
    return m;
}

// F, chi^2 and the robust count at the current state: every bearing and odometry edge once, self-loops
// included (bos.h bos_cost)
void cpu_cost(const bos_cpu_gn* c, double& F, double& chi, int32_t& nrob) {
    F = chi = 0.0;
    nrob = 0;
    auto add = [&](double rho) {
        chi += rho;
        if (rho > c->kt) ++nrob;
        F += bos::lm_huber(rho, c->kt, rho > c->kt ? std::sqrt(c->kt * rho) : 0.0);
    };
    for (size_t k = 0; k < c->b_z.size(); ++k) {
        const double* p = &c->pose[3 * (size_t)c->b_pose[k]];
        const double* l = &c->lm[2 * (size_t)c->b_lm[k]];
        double gx, gy;
        const double e = bos::bearing_error<double>(p[0], p[1], std::cos(p[2]), std::sin(p[2]), l[0], l[1], c->b_z[k], gx, gy);
        const double w = c->b_w.empty() ? 1.0 : c->b_w[k];
        add(e * w * e);
    }
    for (size_t k = 0; k < c->o_src.size(); ++k) {
        const double* s = &c->pose[3 * (size_t)c->o_src[k]];
        const double* d = &c->pose[3 * (size_t)c->o_dst[k]];
        const double* z = &c->o_z[3 * k];
        const double* u = &c->o_om[6 * k];
        double e[3], J[18];
        if (c->o_src[k] == c->o_dst[k]) {
            e[0] = -z[0]; e[1] = -z[1]; e[2] = bos::normalized_angle<double>(-z[2]);
        } else {
            bos::odometry_error_jacobian<double>(s[0], s[1], s[2], std::cos(s[2]), std::sin(s[2]), d[0], d[1], d[2], z[0], z[1],
                                                 z[2], e, J);
        }
        const double Oe[3] = {u[0] * e[0] + u[1] * e[1] + u[2] * e[2], u[1] * e[0] + u[3] * e[1] + u[4] * e[2],
                              u[2] * e[0] + u[4] * e[1] + u[5] * e[2]};
        add(e[0] * Oe[0] + e[1] * Oe[1] + e[2] * Oe[2]);
    }
    // priors are not robustified: F and chi^2 both gain rho
    const bos::PriorSet& R = c->priors;
    for (size_t i = 0; i < R.pose.size(); ++i) {
        const double* p = &c->pose[3 * (size_t)R.pose[i]];
        const double rho = bos::prior_pose_rho<double>(p[0], p[1], p[2], &R.pose_rec[9 * i], &R.pose_rec[9 * i + 3]);
        chi += rho;
        F += rho;
    }
    for (size_t i = 0; i < R.lm.size(); ++i) {
        const double* l = &c->lm[2 * (size_t)R.lm[i]];
        const double rho = bos::prior_landmark_rho<double>(l[0], l[1], &R.lm_rec[5 * i], &R.lm_rec[5 * i + 2]);
        chi += rho;
        F += rho;
    }
}

}  // namespace

extern "C" {

int bos_cpu_gn_step(bos_cpu_gn* c, double* chi2) {
    if (!c) return cfail(BOS_ERR_INVALID, "null handle");
    const double chi = cpu_build(c);
    if (chi2) *chi2 = chi;
    cpu_solve(c, cpu_ref_dof(c));
    cpu_update(c);
    return BOS_OK;
}

int bos_cpu_gn_set_kernel_threshold(bos_cpu_gn* c, double kt) {
    if (!c) return cfail(BOS_ERR_INVALID, "null handle");
    c->kt = kt;
    return BOS_OK;
}

int bos_cpu_gn_set_priors(bos_cpu_gn* c, int32_t n_pose, const int32_t* pose, const double* pose_mean, const double* pose_omega,
                          int32_t n_landmark, const int32_t* landmark, const double* landmark_mean,
                          const double* landmark_omega) {
    if (!c) return cfail(BOS_ERR_INVALID, "null handle");
    const std::string err = bos::prior_set_build(c->NP, c->NL, c->plan.fixed, n_pose, pose, pose_mean, pose_omega, n_landmark,
                                                 landmark, landmark_mean, landmark_omega, c->priors);
    if (!err.empty()) return cfail(BOS_ERR_INVALID, "bos_cpu_gn_set_priors: " + err);
    return BOS_OK;
}

int bos_cpu_gn_cost(bos_cpu_gn* c, double* cost, double* chi2, int32_t* n_robust) {
    if (!c) return cfail(BOS_ERR_INVALID, "null handle");
    double F, chi;
    int32_t nrob;
    cpu_cost(c, F, chi, nrob);
    if (cost) *cost = F;
    if (chi2) *chi2 = chi;
    if (n_robust) *n_robust = nrob;
    return BOS_OK;
}

int bos_cpu_gn_optimize(bos_cpu_gn* c, const bos_lm_options* options, bos_lm_result* result, bos_lm_iteration* trace,
                        int32_t trace_capacity) {
    if (!c) return cfail(BOS_ERR_INVALID, "null handle");
    bos_lm_options o;
    bos::lm_default_options(o);
    if (options) o = *options;
    if (o.max_iterations < 1 || o.max_iterations > 4096) return cfail(BOS_ERR_INVALID, "max_iterations must be 1 .. 4096");
    if (!(o.lambda0 >= 0.0) || !(o.lambda_min > 0.0) || !(o.lambda_max >= o.lambda_min) || !(o.dx_tol >= 0.0) || !(o.f_tol >= 0.0))
        return cfail(BOS_ERR_INVALID, "bad lambda0 / lambda_min / lambda_max / dx_tol / f_tol");
    if (trace_capacity < 0 || (trace_capacity > 0 && !trace)) return cfail(BOS_ERR_INVALID, "trace_capacity without a trace");
    const bos::Plan& P = c->plan;
    const bos::BlockLayout& B = P.blk;
    bos_lm_state st;
    std::memset(&st, 0, sizeof(st));
    st.lambda = o.lambda0 > 0.0 ? o.lambda0 : (c->lm_started ? c->lm_lambda : c->damping);
    st.nu = o.lambda0 > 0.0 || !c->lm_started ? 2.0 : c->lm_nu;
    double chi;
    int32_t nrob;
    cpu_cost(c, st.cost, chi, nrob);
    const double cost_initial = st.cost;
    const std::vector<int32_t> ref = cpu_ref_dof(c);
    const double damping = c->damping;
    while (!st.done) {
        // H0 and b without damping, then lambda on the diagonal of the blocks the J+H wrote
        c->damping = 0.0;
        cpu_build(c);
        c->damping = damping;
        double* hv = c->mf->hval.data();
        for (int32_t p : B.lane_pose)
            if (p >= 0) { hv[6 * (int64_t)p] += st.lambda; hv[6 * (int64_t)p + 2] += st.lambda; hv[6 * (int64_t)p + 5] += st.lambda; }
        for (int32_t l : B.lm_lane_lm) { hv[B.off_ldiag + 3 * (int64_t)l] += st.lambda; hv[B.off_ldiag + 3 * (int64_t)l + 2] += st.lambda; }
        const int info = cpu_solve(c, ref);
        double xx = 0.0, xb = 0.0;
        for (int64_t i = 0; i < P.n; ++i) {
            xx += c->mf->x[i] * c->mf->x[i];
            xb += c->mf->x[i] * c->b[ref[i]];
        }
        const double pred = st.lambda * xx + xb;
        const std::vector<double> pose0 = c->pose, lm0 = c->lm;
        const double max_dx = cpu_update(c);
        double F;
        cpu_cost(c, F, chi, nrob);
        bos_lm_iteration rec;
        const int32_t slot = st.iteration;
        bos::lm_rule_apply(st, o, F, pred, max_dx, info, &rec);
        if (!rec.accepted) { c->pose = pose0; c->lm = lm0; }
        if (trace && slot < trace_capacity) trace[slot] = rec;
    }
    c->lm_started = true;
    c->lm_lambda = st.lambda;
    c->lm_nu = st.nu;
    if (result) {
        result->iterations = st.iteration;
        result->accepted = st.accepted;
        result->rejected = st.rejected;
        result->reason = st.reason;
        result->cost_initial = cost_initial;
        result->cost_final = st.cost;
        result->lambda_final = st.lambda;
    }
    return BOS_OK;
}

int bos_lm_rule_apply(bos_lm_state* state, const bos_lm_options* options, double cost_trial, double predicted,
                      double max_abs_dx, int32_t solver_info, bos_lm_iteration* record) {
    if (!state || !options) return cfail(BOS_ERR_INVALID, "null argument");
    return bos::lm_rule_apply(*state, *options, cost_trial, predicted, max_abs_dx, solver_info, record) ? 1 : 0;
}

int bos_cpu_gn_get_state(const bos_cpu_gn* c, double* pose_xyt, double* landmark_xy) {
    if (!c) return cfail(BOS_ERR_INVALID, "null handle");
    if (pose_xyt) std::memcpy(pose_xyt, c->pose.data(), c->pose.size() * sizeof(double));
    if (landmark_xy) std::memcpy(landmark_xy, c->lm.data(), c->lm.size() * sizeof(double));
    return BOS_OK;
}

void bos_cpu_gn_destroy(bos_cpu_gn* c) { delete c; }

}  // extern "C"
