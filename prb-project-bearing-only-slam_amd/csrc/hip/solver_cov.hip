// Covariances from the multifrontal factor on the C ABI handle (solver_handle.hpp): marginals, edge, pair
// and node covariances and the bearing association, node matching, joint compatibility and JCBB built on them
// (hip/selinv.hpp, hip/pair_cov.hpp, hip/node_cov.hpp, hip/associate.hpp, hip/match.hpp, hip/joint.hpp, hip/jcbb.hpp).
#include <algorithm>
#include <chrono>

#include "solver_handle.hpp"

using namespace bos::capi;

namespace {

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
    if (rc) return fail(rc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
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

// bos_marginals (edge = nullptr) and bos_edge_covariances (edge[4] = bearing_cross, odom_cross,
// bearing_var, odom_cov; with all four null the pass is the marginals' own)
int covariance_pass(bos_solver* s, const char* name, double* const* edge, double* pose_cov, double* landmark_cov,
                    int32_t* solver_info) {
    int rc;
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
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
    if (src) return fail(src == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
    if (info & bos::dev::kMfStall)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out");
    const auto t0 = std::chrono::steady_clock::now();
    if (pose_cov) HIP_TRY(hipMemcpy(pose_cov, out, np9 * sizeof(double), hipMemcpyDeviceToHost));
    if (landmark_cov && nl4) HIP_TRY(hipMemcpy(landmark_cov, out + np9, nl4 * sizeof(double), hipMemcpyDeviceToHost));
    if (any_edge) {
        const double* dev[4] = {er.bearing_cross, er.odom_cross, er.bearing_var, er.odom_cov};
        for (int i = 0; i < 4; ++i)
            if (want[i]) HIP_TRY(hipMemcpy(edge[i], dev[i], ecount[i] * sizeof(double), hipMemcpyDeviceToHost));
    }
    const double dl = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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

// What a matching call returns (host pointers, any of them null): the lists' doubles per entry are dd
// (detail) and dc (covariance), the device's strides kMatchDetailStride / kMatchCovStride
struct MatchOutputs {
    int32_t* cand_ix;
    double *cand_score, *cand_detail, *cand_cov;
    int32_t* n_inside;
    double* all;
    int dd, dc;
};

// bos_match_landmarks (zr null; node: the landmarks) and bos_match_poses (zr: [n][kMatchRowDoubles], z and
// the lower triangle of R; node: the poses), their arguments checked. Rows are grouped by query node, the
// nodes in the order of their first row: one column per node. A landmark's column gives one score row,
// copied to every query of that landmark; a pose's measurements are its rows, in chunks.
int match_pass(bos_solver* s, const char* name, int32_t n, const int32_t* node, const double* zr, double gate, int32_t k,
               const MatchOutputs& o, int32_t* solver_info) {
    int rc;
    const bool poses = zr != nullptr;
    const size_t N = (size_t)(poses ? s->NP : s->NL), K = (size_t)k;
    const bool select = o.cand_ix || o.cand_score || o.cand_detail || o.cand_cov || o.n_inside;
    const bool rows_wanted = select || o.all;
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    for (double& m : s->match_ms) m = 0.0;
    // a query's slots as they stay where nothing is listed
    auto pad = [&](int32_t q) {
        for (size_t j = 0; j < K; ++j) {
            if (o.cand_ix) o.cand_ix[q * K + j] = -1;
            if (o.cand_score) o.cand_score[q * K + j] = HUGE_VAL;
            if (o.cand_detail) std::fill_n(o.cand_detail + (q * K + j) * o.dd, o.dd, 0.0);
            if (o.cand_cov) std::fill_n(o.cand_cov + (q * K + j) * o.dc, o.dc, 0.0);
        }
        if (o.n_inside) o.n_inside[q] = 0;
    };
    if (s->plan.n == 0) {   // the fixed pose alone: there is no system to take a covariance from, no score
        for (int32_t q = 0; q < n; ++q) pad(q);
        if (o.all) std::fill_n(o.all, (size_t)n * N, bos::match_nan());
        return BOS_OK;
    }
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    const auto t_prep = Clock::now();
    std::vector<int32_t> group_of(N, -1), nodes;
    std::vector<std::vector<int32_t>> members;
    for (int32_t q = 0; q < n && rows_wanted; ++q) {
        int32_t& g = group_of[node[q]];
        if (g < 0) {
            g = (int32_t)nodes.size();
            nodes.push_back(node[q]);
            members.emplace_back();
        }
        members[g].push_back(q);
    }
    const int widest = std::max(s->NP, s->NL);   // one set of buffers serves both calls
    int chunk_rows = bos::dev::match_budget_rows(widest);
    if (s->match_chunk > 0) chunk_rows = (int)std::min<int64_t>(chunk_rows, s->match_chunk);
    if (rows_wanted) {
        std::string err;
        if ((rc = node_cov_setup(s, name))) return rc;
        size_t largest = 1;
        for (const std::vector<int32_t>& m : members) largest = std::max(largest, poses ? m.size() : (size_t)1);
        if (!s->match) s->match = bos::dev::match_create();
        if (bos::dev::match_reserve(s->match, widest, (int)std::min<size_t>(largest, (size_t)chunk_rows), err))
            return fail(BOS_ERR_DEVICE, err);
    }
    s->match_ms[0] = ms_since(t_prep);
    // the factorization's word, read and cleared before anything reads the panels
    int32_t info = 0;
    if ((rc = enqueue_factorization(s, &info))) return rc;
    s->match_ms[1] = elapsed(s->ev[0], s->ev[1]);
    s->match_ms[2] = elapsed(s->ev[1], s->ev[2]);
    if (info & bos::dev::kMfStall)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out");
    if (!rows_wanted) {   // nothing asked for
        if (solver_info) *solver_info = info;
        return BOS_OK;
    }
    const double* sig = nullptr;
    {   // the marginals' own pass on this factorization: the diagonal blocks of the projection
        std::string err;
        const int src = bos::dev::mf_selected_inverse(s->mf, s->plan, &sig, s->stream, err);
        hipError_t e = hipEventRecord(s->ev[3], s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        HIP_TRY(e);
        if (src) return fail(src == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        s->match_ms[3] = elapsed(s->ev[2], s->ev[3]);
    }
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    const bool want[4] = {false, false, poses, !poses};
    std::vector<double> dbuf;
    std::vector<int32_t> ibuf;
    std::vector<std::pair<int32_t, int32_t>> dst;   // (the chunk's row, the query that receives it)
    for (size_t g = 0; g < nodes.size(); ++g) {
        const int a = nodes[g], a_node = poses ? a : s->NP + a;
        const std::vector<int32_t>& mem = members[g];
        std::string err;
        bos::dev::NodeCovDev col;
        HIP_TRY(hipEventRecord(s->ev[4], s->stream));
        int prc = bos::dev::node_cov_enqueue(s->node, view, a_node, a_node == s->plan.fixed, want, sig, s->d_pose, s->d_lm, s->stream, nullptr,
                                             &col, err);
        if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        const size_t rows_of_node = poses ? mem.size() : 1;
        for (size_t c0 = 0; c0 < rows_of_node; c0 += (size_t)chunk_rows) {
            const size_t rows = std::min(rows_of_node - c0, (size_t)chunk_rows);
            bos::dev::MatchDev res;
            dst.clear();
            if (poses) {
                dbuf.resize(rows * bos::dev::kMatchRowDoubles);
                for (size_t i = 0; i < rows; ++i) {
                    std::copy_n(zr + (size_t)mem[c0 + i] * bos::dev::kMatchRowDoubles, bos::dev::kMatchRowDoubles,
                                dbuf.begin() + i * bos::dev::kMatchRowDoubles);
                    dst.emplace_back((int32_t)i, mem[c0 + i]);
                }
                prc = bos::dev::match_pose_enqueue(s->match, s->NP, a, (int)rows, dbuf.data(), gate, select, col.projected_pose, s->d_pose,
                                                   s->stream, s->ev[5], s->ev[6], &res, err);
            } else {
                for (int32_t q : mem) dst.emplace_back(0, q);
                prc = bos::dev::match_landmark_enqueue(s->match, s->NL, a, gate, select, col.projected_landmark, s->d_lm, s->stream,
                                                       s->ev[5], s->ev[6], &res, err);
            }
            hipError_t e = hipEventRecord(s->ev[7], s->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
            HIP_TRY(e);
            if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
            if (c0 == 0) s->match_ms[4] += elapsed(s->ev[4], s->ev[5]);
            s->match_ms[5] += elapsed(s->ev[5], s->ev[6]);
            s->match_ms[6] += elapsed(s->ev[6], s->ev[7]);
            // the chunk's small outputs once each, then a row's k entries to the queries that receive it
            const auto t_dl = Clock::now();
            const size_t RK = rows * bos::kMatchMaxK;
            double* const douts[3] = {o.cand_score, o.cand_detail, o.cand_cov};
            const double* const ddev[3] = {res.cand_score, res.cand_detail, res.cand_cov};
            const size_t width[3] = {1, (size_t)o.dd, (size_t)o.dc};
            const size_t stride[3] = {1, (size_t)bos::dev::kMatchDetailStride, (size_t)bos::dev::kMatchCovStride};
            for (int v = 0; v < 3; ++v) {
                if (!douts[v]) continue;
                dbuf.resize(RK * stride[v]);
                HIP_TRY(hipMemcpy(dbuf.data(), ddev[v], RK * stride[v] * sizeof(double), hipMemcpyDeviceToHost));
                for (const auto& rq : dst)
                    for (size_t j = 0; j < K; ++j)
                        std::copy_n(dbuf.begin() + ((size_t)rq.first * bos::kMatchMaxK + j) * stride[v], width[v],
                                    douts[v] + ((size_t)rq.second * K + j) * width[v]);
            }
            ibuf.resize(RK);
            if (o.cand_ix) {
                HIP_TRY(hipMemcpy(ibuf.data(), res.cand_ix, RK * sizeof(int32_t), hipMemcpyDeviceToHost));
                for (const auto& rq : dst) std::copy_n(ibuf.begin() + (size_t)rq.first * bos::kMatchMaxK, K, o.cand_ix + (size_t)rq.second * K);
            }
            if (o.n_inside) {
                HIP_TRY(hipMemcpy(ibuf.data(), res.n_inside, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
                for (const auto& rq : dst) o.n_inside[rq.second] = ibuf[rq.first];
            }
            for (size_t i = 0; i < dst.size() && o.all; ++i) {
                double* to = o.all + (size_t)dst[i].second * N;
                if (i > 0 && dst[i].first == dst[i - 1].first) std::copy_n(o.all + (size_t)dst[i - 1].second * N, N, to);
                else HIP_TRY(hipMemcpy(to, res.score + (size_t)dst[i].first * N, N * sizeof(double), hipMemcpyDeviceToHost));
            }
            s->match_ms[7] += ms_since(t_dl);
        }
    }
    if (solver_info) *solver_info = info;
    return BOS_OK;
}

}  // namespace

extern "C" {

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
    for (int i = 0; i < 5; ++i) ms[i] = s->edge_ms[i];
    if (edge_bytes) *edge_bytes = s->mf ? bos::dev::mf_edge_cov_bytes(s->mf) : 0;
    return BOS_OK;
}

int bos_marginals_timing(const bos_solver* s, double ms[4], int64_t* sigma_bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    for (int i = 0; i < 4; ++i) ms[i] = s->marg_ms[i];
    if (sigma_bytes) *sigma_bytes = s->mf ? bos::dev::mf_selinv_sigma_bytes(s->mf) : 0;
    return BOS_OK;
}

int bos_pair_covariances(bos_solver* s, int64_t n_pairs, const int32_t* node_a, const int32_t* node_b, double* cross,
                         double* projected, double* cov_a, double* cov_b, int32_t* solver_info) {
    const char* name = "bos_pair_covariances";
    int rc;
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!node_a || !node_b))) return fail(BOS_ERR_INVALID, std::string(name) + ": bad argument");
    if (n_pairs == 0) return BOS_OK;
    if (!bos::pair_ids_valid(s->NP, s->NL, n_pairs, node_a, node_b))
        return fail(BOS_ERR_INVALID, std::string(name) + ": a node id outside [0, NP + NL), or a mixed pair not written (pose, landmark)");
    double* const outs[4] = {cross, projected, cov_a, cov_b};
    bool want[4];
    for (int i = 0; i < 4; ++i) want[i] = outs[i] != nullptr;
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    for (double& m : s->pair_ms) m = 0.0;
    if (s->plan.n == 0) {   // the fixed pose alone
        for (int i = 0; i < 4; ++i)
            if (want[i]) std::fill(outs[i], outs[i] + 9 * n_pairs, 0.0);
        return BOS_OK;
    }
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    auto t_prep = Clock::now();
    if ((rc = pair_paths_setup(s, name))) return rc;
    if (!s->pair) s->pair = bos::dev::pair_cov_create();
    s->pair_ms[0] += ms_since(t_prep);
    // the factorization's word, read and cleared before anything reads the panels
    int32_t info = 0;
    if ((rc = enqueue_factorization(s, &info))) return rc;
    s->pair_ms[1] = elapsed(s->ev[0], s->ev[1]);
    s->pair_ms[2] = elapsed(s->ev[1], s->ev[2]);
    if (info & bos::dev::kMfStall)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out");
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    const int64_t max_nodes = s->pair_batch_nodes > 0 ? std::max<int64_t>(s->pair_batch_nodes, 2) : INT32_MAX;
    std::vector<int32_t> slot_of((size_t)s->NP + s->NL, -1);
    bos::PairBatchHost B;
    for (int64_t q0 = 0; q0 < n_pairs; q0 += B.nq) {
        t_prep = Clock::now();
        bos::pair_batch_build(s->plan, s->pair_paths, n_pairs, node_a, node_b, q0, max_nodes,
                              bos::dev::kPairYBudgetBytes / (int64_t)sizeof(double), bos::dev::kPairMaxQueries, slot_of, B);
        bos::dev::PairCovBatch b;
        b.n_nodes = (int32_t)B.n_node.size(); b.n_queries = B.nq; b.y_count = B.y_count;
        b.y_off = B.y_off.data(); b.n_sn = B.n_sn.data(); b.n_loc = B.n_loc.data(); b.n_d = B.n_d.data(); b.n_len = B.n_len.data();
        b.q_a = node_a + q0; b.q_b = node_b + q0; b.q_slot_a = B.q_slot_a.data(); b.q_slot_b = B.q_slot_b.data();
        b.q_off_a = B.q_off_a.data(); b.q_off_b = B.q_off_b.data(); b.q_c = B.q_c.data();
        std::string err;
        int prc = bos::dev::pair_cov_upload(s->pair, b, want, err);
        if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        s->pair_ms[0] += ms_since(t_prep);
        bos::dev::PairCovOut res;
        HIP_TRY(hipEventRecord(s->ev[3], s->stream));
        prc = bos::dev::pair_cov_enqueue(s->pair, view, s->pair_paths.max_m, s->NP, s->d_pose, s->d_lm, s->stream, s->ev[4], &res, err);
        hipError_t e = hipEventRecord(s->ev[5], s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        HIP_TRY(e);
        if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        s->pair_ms[3] += elapsed(s->ev[3], s->ev[4]);
        s->pair_ms[4] += elapsed(s->ev[4], s->ev[5]);
        const auto t_dl = Clock::now();
        const double* dev[4] = {res.cross, res.projected, res.cov_a, res.cov_b};
        for (int i = 0; i < 4; ++i)
            if (want[i]) HIP_TRY(hipMemcpy(outs[i] + 9 * q0, dev[i], 9 * (size_t)B.nq * sizeof(double), hipMemcpyDeviceToHost));
        s->pair_ms[5] += ms_since(t_dl);
    }
    if (solver_info) *solver_info = info;
    return BOS_OK;
}

int bos_pair_covariances_timing(const bos_solver* s, double ms[6], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    for (int i = 0; i < 6; ++i) ms[i] = s->pair_ms[i];
    if (bytes) *bytes = bos::dev::pair_cov_bytes(s->pair);
    return BOS_OK;
}

extern "C++" {
namespace {
// One batch of bos_joint_compatibility and of bos_jcbb, which runs on the joint call's batches of all-pairings
// hypotheses: the batch from h0 on (joint_batch_build), the pair call's blocks uploaded, the feature's own batch
// uploaded by upload(B, err) (0, or pair_cov's codes), then between the handle's events 3 .. 6 the pair call's path
// solve and products and the feature's kernel, enqueued by enqueue(diag, cross, err), and the wait. ms: the
// feature's seven slots (0, 3, 4, 5 are added to).
template <class Upload, class Enqueue>
int joint_batch_run(bos_solver* s, const bos::dev::MfView& view, int32_t n_hyp, const int32_t* hyp_start, const int32_t* pose,
                    const int32_t* landmark, int32_t h0, int64_t max_hyp, bos::JointBatchHost& B, double* ms, Upload upload,
                    Enqueue enqueue) {
    typedef std::chrono::steady_clock Clock;
    const auto t_prep = Clock::now();
    bos::joint_batch_build(s->plan, s->pair_paths, n_hyp, hyp_start, pose, landmark, h0,
                           bos::dev::kPairYBudgetBytes / (int64_t)sizeof(double), max_hyp, bos::dev::kPairMaxQueries, s->joint_slot_of, B);
    const bos::PairBatchHost& Q = B.pairs;
    bos::dev::PairCovBatch b;
    b.n_nodes = (int32_t)Q.n_node.size(); b.n_queries = Q.nq; b.y_count = Q.y_count;
    b.y_off = Q.y_off.data(); b.n_sn = Q.n_sn.data(); b.n_loc = Q.n_loc.data(); b.n_d = Q.n_d.data(); b.n_len = Q.n_len.data();
    b.q_a = B.pair_a.data(); b.q_b = B.pair_b.data(); b.q_slot_a = Q.q_slot_a.data(); b.q_slot_b = Q.q_slot_b.data();
    b.q_off_a = Q.q_off_a.data(); b.q_off_b = Q.q_off_b.data(); b.q_c = Q.q_c.data();
    std::string err;
    int prc = bos::dev::pair_cov_upload_blocks(s->pair, b, err);
    if (!prc) prc = upload(B, err);
    if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
    ms[0] += std::chrono::duration<double, std::milli>(Clock::now() - t_prep).count();
    const double *diag = nullptr, *cross = nullptr;
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    prc = bos::dev::pair_cov_enqueue_blocks(s->pair, view, s->pair_paths.max_m, s->NP, s->stream, s->ev[4], &diag, &cross, err);
    hipError_t e = hipEventRecord(s->ev[5], s->stream);
    if (!prc && e == hipSuccess) prc = enqueue(diag, cross, err);
    if (e == hipSuccess) e = hipEventRecord(s->ev[6], s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    HIP_TRY(e);
    if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
    ms[3] += elapsed(s->ev[3], s->ev[4]);
    ms[4] += elapsed(s->ev[4], s->ev[5]);
    ms[5] += elapsed(s->ev[5], s->ev[6]);
    return BOS_OK;
}
}  // namespace
}  // extern "C++"

int bos_joint_compatibility(bos_solver* s, int32_t n_hyp, const int32_t* hyp_start, const int32_t* pose, const int32_t* landmark,
                            const double* z, const double* omega, double* prefix_nis, double* joint_nis, double* innovation,
                            double* innovation_cov, int32_t* solver_info) {
    const char* name = "bos_joint_compatibility";
    int rc;
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
    if (const char* bad = bos::joint_bad_argument(s->NP, s->NL, n_hyp, hyp_start, pose, landmark, z, omega))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_hyp == 0) return BOS_OK;
    double* const outs[4] = {prefix_nis, joint_nis, innovation, innovation_cov};
    bool want[4];
    for (int i = 0; i < 4; ++i) want[i] = outs[i] != nullptr;
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    for (double& m : s->joint_ms) m = 0.0;
    if (s->plan.n == 0) {   // the fixed pose alone: no landmark, so every hypothesis is empty
        if (joint_nis) std::fill(joint_nis, joint_nis + n_hyp, 0.0);
        return BOS_OK;
    }
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    auto t_prep = Clock::now();
    if ((rc = pair_paths_setup(s, name))) return rc;
    if (!s->pair) s->pair = bos::dev::pair_cov_create();
    if (!s->joint) s->joint = bos::dev::joint_create();
    const int32_t n_pair = hyp_start[n_hyp];
    std::vector<double> ones;
    if (!omega) ones.assign((size_t)n_pair + 1, 1.0);
    const double* om = omega ? omega : ones.data();
    s->joint_ms[0] += ms_since(t_prep);
    // the factorization's word, read and cleared before anything reads the panels
    int32_t info = 0;
    if ((rc = enqueue_factorization(s, &info))) return rc;
    s->joint_ms[1] = elapsed(s->ev[0], s->ev[1]);
    s->joint_ms[2] = elapsed(s->ev[1], s->ev[2]);
    if (info & bos::dev::kMfStall)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out");
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    const int64_t max_hyp = s->joint_batch > 0 ? s->joint_batch : bos::dev::kJointMaxHyp;
    if (s->joint_slot_of.empty()) s->joint_slot_of.assign((size_t)s->NP + s->NL, -1);   // all -1 between batches
    std::vector<int32_t> local_start;
    bos::JointBatchHost B;
    int64_t s_done = 0;
    for (int32_t h0 = 0; h0 < n_hyp; h0 += B.nh) {
        int32_t p0 = 0, np = 0;
        bos::dev::JointOut res;
        rc = joint_batch_run(
            s, view, n_hyp, hyp_start, pose, landmark, h0, max_hyp, B, s->joint_ms,
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
        s->joint_ms[6] += ms_since(t_dl);
    }
    if (solver_info) *solver_info = info;
    return BOS_OK;
}

int bos_joint_compatibility_timing(const bos_solver* s, double ms[7], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    for (int i = 0; i < 7; ++i) ms[i] = s->joint_ms[i];
    if (bytes) *bytes = bos::dev::joint_bytes(s->joint) + bos::dev::pair_cov_bytes(s->pair);
    return BOS_OK;
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
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
    if (const char* bad = bos::jcbb_bad_argument(s->NP, s->NL, n_frames, frame_start, pose, z, omega, cand_start, cand_landmark, gate,
                                                 max_nodes))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_frames == 0) return BOS_OK;
    bos::dev::JcbbWant want;
    want.assignment = assignment != nullptr; want.n_paired = n_paired != nullptr; want.joint_nis = joint_nis != nullptr;
    want.prefix_nis = prefix_nis != nullptr; want.complete = complete != nullptr; want.innovation = innovation != nullptr;
    want.cov = innovation_cov != nullptr;
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    for (double& m : s->jcbb_ms) m = 0.0;
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
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    auto t_prep = Clock::now();
    if ((rc = pair_paths_setup(s, name))) return rc;
    if (!s->pair) s->pair = bos::dev::pair_cov_create();
    if (!s->jcbb) s->jcbb = bos::dev::jcbb_create();
    bos::JcbbPairings A;   // the frames as all-pairings hypotheses
    bos::jcbb_pairings(n_frames, frame_start, pose, z, omega, cand_start, A);
    const int32_t* hyp_start = A.hyp_start.data();
    s->jcbb_ms[0] += ms_since(t_prep);
    // the factorization's word, read and cleared before anything reads the panels
    int32_t info = 0;
    if ((rc = enqueue_factorization(s, &info))) return rc;
    s->jcbb_ms[1] = elapsed(s->ev[0], s->ev[1]);
    s->jcbb_ms[2] = elapsed(s->ev[1], s->ev[2]);
    if (info & bos::dev::kMfStall)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out");
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    const int64_t max_hyp = s->jcbb_batch > 0 ? s->jcbb_batch : bos::dev::kJointMaxHyp;
    if (s->joint_slot_of.empty()) s->joint_slot_of.assign((size_t)s->NP + s->NL, -1);   // all -1 between batches
    std::vector<int32_t> local_hyp, local_bearing, local_cand;
    bos::JointBatchHost B;
    int64_t s_done = 0;
    for (int32_t h0 = 0; h0 < n_frames; h0 += B.nh) {
        int32_t p0 = 0, np = 0, b0 = 0, nb = 0;
        bos::dev::JcbbOut res;
        rc = joint_batch_run(
            s, view, n_frames, hyp_start, A.pose.data(), cand_landmark, h0, max_hyp, B, s->jcbb_ms,
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
        s->jcbb_ms[6] += ms_since(t_dl);
    }
    if (solver_info) *solver_info = info;
    return BOS_OK;
}

int bos_jcbb_timing(const bos_solver* s, double ms[7], int64_t* bytes, int64_t capacity, int64_t* nodes, int32_t* n_frames) {
    if (!s || !ms || capacity < 0 || (capacity > 0 && !nodes)) return fail(BOS_ERR_INVALID, "bos_jcbb_timing: bad argument");
    for (int i = 0; i < 7; ++i) ms[i] = s->jcbb_ms[i];
    if (bytes) *bytes = bos::dev::jcbb_bytes(s->jcbb) + bos::dev::pair_cov_bytes(s->pair);
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

int bos_node_covariances(bos_solver* s, int32_t n_nodes, const int32_t* nodes, double* cross_pose, double* cross_landmark,
                         double* projected_pose, double* projected_landmark, double* pose_cov, double* landmark_cov,
                         int32_t* solver_info) {
    const char* name = "bos_node_covariances";
    int rc;
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
    if (n_nodes < 0 || (n_nodes > 0 && !nodes)) return fail(BOS_ERR_INVALID, std::string(name) + ": bad argument");
    if (n_nodes == 0) return BOS_OK;
    if (!bos::node_ids_valid(s->NP, s->NL, n_nodes, nodes))
        return fail(BOS_ERR_INVALID, std::string(name) + ": a node id outside [0, NP + NL)");
    const size_t np9 = 9 * (size_t)s->NP, nl4 = 4 * (size_t)s->NL;
    const size_t count[4] = {np9, 6 * (size_t)s->NL, np9, nl4};
    double* const outs[4] = {cross_pose, cross_landmark, projected_pose, projected_landmark};
    bool want[4], any_node = false;
    for (int i = 0; i < 4; ++i) any_node |= want[i] = outs[i] != nullptr && count[i] > 0;
    const bool projected = want[2] || want[3], need_sig = projected || pose_cov || (landmark_cov && nl4);
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    for (double& m : s->node_ms) m = 0.0;
    if (s->plan.n == 0) {   // the fixed pose alone
        for (int i = 0; i < 4; ++i)
            if (want[i]) std::fill(outs[i], outs[i] + (size_t)n_nodes * count[i], 0.0);
        if (pose_cov) std::fill(pose_cov, pose_cov + np9, 0.0);
        return BOS_OK;
    }
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    const auto t_prep = Clock::now();
    if (any_node && (rc = node_cov_setup(s, name))) return rc;
    s->node_ms[0] = ms_since(t_prep);
    // the factorization's word, read and cleared before anything reads the panels
    int32_t info = 0;
    if ((rc = enqueue_factorization(s, &info))) return rc;
    s->node_ms[1] = elapsed(s->ev[0], s->ev[1]);
    s->node_ms[2] = elapsed(s->ev[1], s->ev[2]);
    if (info & bos::dev::kMfStall)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out");
    const double* sig = nullptr;
    if (need_sig) {   // the marginals' own pass on this factorization
        std::string err;
        const int src = bos::dev::mf_selected_inverse(s->mf, s->plan, &sig, s->stream, err);
        hipError_t e = hipEventRecord(s->ev[3], s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        HIP_TRY(e);
        if (src) return fail(src == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        s->node_ms[3] = elapsed(s->ev[2], s->ev[3]);
    }
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    for (int32_t q = 0; q < n_nodes && any_node; ++q) {
        std::string err;
        bos::dev::NodeCovDev res;
        HIP_TRY(hipEventRecord(s->ev[4], s->stream));
        const int prc = bos::dev::node_cov_enqueue(s->node, view, nodes[q], nodes[q] == s->plan.fixed, want, projected ? sig : nullptr,
                                                   s->d_pose, s->d_lm, s->stream, s->ev[5], &res, err);
        hipError_t e = hipEventRecord(s->ev[6], s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        HIP_TRY(e);
        if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        s->node_ms[4] += elapsed(s->ev[4], s->ev[5]);
        s->node_ms[5] += elapsed(s->ev[5], s->ev[6]);
        const auto t_dl = Clock::now();
        const double* dev[4] = {res.cross_pose, res.cross_landmark, res.projected_pose, res.projected_landmark};
        for (int i = 0; i < 4; ++i)
            if (want[i]) HIP_TRY(hipMemcpy(outs[i] + (size_t)q * count[i], dev[i], count[i] * sizeof(double), hipMemcpyDeviceToHost));
        s->node_ms[6] += ms_since(t_dl);
    }
    const auto t_dl = Clock::now();
    if (pose_cov) HIP_TRY(hipMemcpy(pose_cov, sig, np9 * sizeof(double), hipMemcpyDeviceToHost));
    if (landmark_cov && nl4) HIP_TRY(hipMemcpy(landmark_cov, sig + np9, nl4 * sizeof(double), hipMemcpyDeviceToHost));
    s->node_ms[6] += ms_since(t_dl);
    if (solver_info) *solver_info = info;
    return BOS_OK;
}

int bos_node_covariances_timing(const bos_solver* s, double ms[7], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    for (int i = 0; i < 7; ++i) ms[i] = s->node_ms[i];
    if (bytes) *bytes = bos::dev::node_cov_bytes(s->node);
    return BOS_OK;
}

int bos_associate_bearings(bos_solver* s, int32_t n_bearings, const int32_t* pose, const double* z, const double* omega, double gate,
                           int32_t k, int32_t* cand_landmark, double* cand_nis, double* cand_innovation, double* cand_var,
                           int32_t* n_inside, double* nis_all, int32_t* solver_info) {
    const char* name = "bos_associate_bearings";
    int rc;
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
    if (const char* bad = bos::assoc_bad_argument(s->NP, n_bearings, pose, z, omega, gate, k))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_bearings == 0) return BOS_OK;
    const size_t NL = (size_t)s->NL, K = (size_t)k;
    const bool select = cand_landmark || cand_nis || cand_innovation || cand_var || n_inside;
    const bool rows_wanted = NL > 0 && (select || nis_all);
    HIP_TRY(hipSetDevice(s->device));
    if (solver_info) *solver_info = 0;
    for (double& m : s->assoc_ms) m = 0.0;
    // a bearing's slots as they stay where nothing is listed
    auto pad = [&](int32_t q) {
        for (size_t j = 0; j < K; ++j) {
            if (cand_landmark) cand_landmark[q * K + j] = -1;
            if (cand_nis) cand_nis[q * K + j] = HUGE_VAL;
            if (cand_innovation) cand_innovation[q * K + j] = 0.0;
            if (cand_var) cand_var[q * K + j] = 0.0;
        }
        if (n_inside) n_inside[q] = 0;
    };
    if (s->plan.n == 0) {   // the fixed pose alone: no landmark
        for (int32_t q = 0; q < n_bearings; ++q) pad(q);
        return BOS_OK;
    }
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    const auto t_prep = Clock::now();
    // the bearings grouped by pose, the poses in the order of their first bearing, a pose's bearings in the call's
    std::vector<int32_t> group_of((size_t)s->NP, -1), poses;
    std::vector<std::vector<int32_t>> members;
    for (int32_t q = 0; q < n_bearings && rows_wanted; ++q) {
        int32_t& g = group_of[pose[q]];
        if (g < 0) {
            g = (int32_t)poses.size();
            poses.push_back(pose[q]);
            members.emplace_back();
        }
        members[g].push_back(q);
    }
    int chunk_rows = bos::dev::associate_budget_rows(s->NL);
    if (s->assoc_chunk > 0) chunk_rows = (int)std::min<int64_t>(chunk_rows, s->assoc_chunk);
    if (rows_wanted) {
        std::string err;
        if ((rc = node_cov_setup(s, name))) return rc;
        size_t largest = 0;
        for (const std::vector<int32_t>& m : members) largest = std::max(largest, m.size());
        if (!s->assoc) s->assoc = bos::dev::associate_create();
        if (bos::dev::associate_reserve(s->assoc, s->NL, (int)std::min<size_t>(largest, (size_t)chunk_rows), err))
            return fail(BOS_ERR_DEVICE, err);
    }
    s->assoc_ms[0] = ms_since(t_prep);
    // the factorization's word, read and cleared before anything reads the panels
    int32_t info = 0;
    if ((rc = enqueue_factorization(s, &info))) return rc;
    s->assoc_ms[1] = elapsed(s->ev[0], s->ev[1]);
    s->assoc_ms[2] = elapsed(s->ev[1], s->ev[2]);
    if (info & bos::dev::kMfStall)
        return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out");
    if (!rows_wanted) {   // no landmark, or nothing asked for
        for (int32_t q = 0; q < n_bearings; ++q) pad(q);
        if (solver_info) *solver_info = info;
        return BOS_OK;
    }
    const double* sig = nullptr;
    {   // the marginals' own pass on this factorization: the diagonal blocks of the projection
        std::string err;
        const int src = bos::dev::mf_selected_inverse(s->mf, s->plan, &sig, s->stream, err);
        hipError_t e = hipEventRecord(s->ev[3], s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        HIP_TRY(e);
        if (src) return fail(src == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        s->assoc_ms[3] = elapsed(s->ev[2], s->ev[3]);
    }
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    const bool want[4] = {false, false, false, true};
    std::vector<double> zc, oc, dbuf;
    std::vector<int32_t> ibuf;
    for (size_t g = 0; g < poses.size(); ++g) {
        const int a = poses[g];
        const std::vector<int32_t>& mem = members[g];
        std::string err;
        bos::dev::NodeCovDev col;
        HIP_TRY(hipEventRecord(s->ev[4], s->stream));
        int prc = bos::dev::node_cov_enqueue(s->node, view, a, a == s->plan.fixed, want, sig, s->d_pose, s->d_lm, s->stream, nullptr, &col, err);
        if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
        for (size_t c0 = 0; c0 < mem.size(); c0 += (size_t)chunk_rows) {
            const size_t rows = std::min(mem.size() - c0, (size_t)chunk_rows);
            zc.resize(rows);
            oc.resize(rows);
            for (size_t i = 0; i < rows; ++i) {
                zc[i] = z[mem[c0 + i]];
                oc[i] = omega ? omega[mem[c0 + i]] : 1.0;
            }
            bos::dev::AssociateDev res;
            prc = bos::dev::associate_enqueue(s->assoc, a, (int)rows, zc.data(), oc.data(), gate, select, col.projected_landmark, s->d_pose,
                                              s->d_lm, s->stream, s->ev[5], s->ev[6], &res, err);
            hipError_t e = hipEventRecord(s->ev[7], s->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
            HIP_TRY(e);
            if (prc) return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err);
            if (c0 == 0) s->assoc_ms[4] += elapsed(s->ev[4], s->ev[5]);
            s->assoc_ms[5] += elapsed(s->ev[5], s->ev[6]);
            s->assoc_ms[6] += elapsed(s->ev[6], s->ev[7]);
            // the chunk's small outputs once each, then a bearing's k entries to its place in the call's order
            const auto t_dl = Clock::now();
            const size_t RK = rows * bos::kAssocMaxK;
            double* const douts[3] = {cand_nis, cand_innovation, cand_var};
            const double* const ddev[3] = {res.cand_nis, res.cand_innovation, res.cand_var};
            dbuf.resize(RK);
            for (int o = 0; o < 3; ++o) {
                if (!douts[o]) continue;
                HIP_TRY(hipMemcpy(dbuf.data(), ddev[o], RK * sizeof(double), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < rows; ++i)
                    std::copy(dbuf.begin() + i * bos::kAssocMaxK, dbuf.begin() + i * bos::kAssocMaxK + K, douts[o] + (size_t)mem[c0 + i] * K);
            }
            ibuf.resize(RK);
            if (cand_landmark) {
                HIP_TRY(hipMemcpy(ibuf.data(), res.cand_landmark, RK * sizeof(int32_t), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < rows; ++i)
                    std::copy(ibuf.begin() + i * bos::kAssocMaxK, ibuf.begin() + i * bos::kAssocMaxK + K, cand_landmark + (size_t)mem[c0 + i] * K);
            }
            if (n_inside) {
                HIP_TRY(hipMemcpy(ibuf.data(), res.n_inside, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < rows; ++i) n_inside[mem[c0 + i]] = ibuf[i];
            }
            for (size_t i = 0; i < rows && nis_all; ++i)
                HIP_TRY(hipMemcpy(nis_all + (size_t)mem[c0 + i] * NL, res.nis + i * NL, NL * sizeof(double), hipMemcpyDeviceToHost));
            s->assoc_ms[7] += ms_since(t_dl);
        }
    }
    if (solver_info) *solver_info = info;
    return BOS_OK;
}

int bos_associate_bearings_timing(const bos_solver* s, double ms[8], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    for (int i = 0; i < 8; ++i) ms[i] = s->assoc_ms[i];
    if (bytes) *bytes = bos::dev::associate_bytes(s->assoc);
    return BOS_OK;
}

int bos_debug_set_associate_chunk(bos_solver* s, int64_t max_bearings) {
    if (!s || max_bearings < 0) return fail(BOS_ERR_INVALID, "bad argument");
    s->assoc_chunk = max_bearings;
    return BOS_OK;
}

int bos_match_landmarks(bos_solver* s, int32_t n_queries, const int32_t* landmark, double gate, int32_t k, int32_t* cand_landmark,
                        double* cand_d2, double* cand_diff, double* cand_cov, int32_t* n_inside, double* d2_all, int32_t* solver_info) {
    const char* name = "bos_match_landmarks";
    int rc;
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
    if (const char* bad = bos::match_landmarks_bad_argument(s->NL, n_queries, landmark, gate, k))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_queries == 0) return BOS_OK;
    const MatchOutputs o = {cand_landmark, cand_d2, cand_diff, cand_cov, n_inside, d2_all, 2, 4};
    return match_pass(s, name, n_queries, landmark, nullptr, gate, k, o, solver_info);
}

int bos_match_poses(bos_solver* s, int32_t n_meas, const int32_t* pose, const double* z, const double* omega, double gate, int32_t k,
                    int32_t* cand_pose, double* cand_nis, double* cand_innovation, double* cand_cov, int32_t* n_inside, double* nis_all,
                    int32_t* solver_info) {
    const char* name = "bos_match_poses";
    int rc;
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if ((rc = require_one_gpu(s, name, true, " (a rank holds part of the factor)"))) return rc;
    std::vector<double> R(9 * (size_t)std::max(n_meas, 0));
    if (const char* bad = bos::match_poses_bad_argument(s->NP, n_meas, pose, z, omega, gate, k, R.data()))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_meas == 0) return BOS_OK;
    // a measurement's row as the device reads it: z, then R's lower triangle
    std::vector<double> zr((size_t)n_meas * bos::dev::kMatchRowDoubles);
    for (int32_t q = 0; q < n_meas; ++q) {
        double* v = zr.data() + (size_t)q * bos::dev::kMatchRowDoubles;
        const double* Rq = R.data() + 9 * (size_t)q;
        std::copy_n(z + 3 * (size_t)q, 3, v);
        v[3] = Rq[0]; v[4] = Rq[3]; v[5] = Rq[4]; v[6] = Rq[6]; v[7] = Rq[7]; v[8] = Rq[8];
    }
    const MatchOutputs o = {cand_pose, cand_nis, cand_innovation, cand_cov, n_inside, nis_all, 3, 9};
    return match_pass(s, name, n_meas, pose, zr.data(), gate, k, o, solver_info);
}

int bos_match_timing(const bos_solver* s, double ms[8], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    for (int i = 0; i < 8; ++i) ms[i] = s->match_ms[i];
    if (bytes) *bytes = bos::dev::match_bytes(s->match);
    return BOS_OK;
}

int bos_debug_set_match_chunk(bos_solver* s, int64_t max_rows) {
    if (!s || max_rows < 0) return fail(BOS_ERR_INVALID, "bad argument");
    s->match_chunk = max_rows;
    return BOS_OK;
}

int bos_debug_set_pair_batch(bos_solver* s, int64_t max_distinct_nodes) {
    if (!s || max_distinct_nodes < 0) return fail(BOS_ERR_INVALID, "bad argument");
    s->pair_batch_nodes = max_distinct_nodes;
    return BOS_OK;
}

}  // extern "C"
