// The covariance calls built on the node call's columns (hip/node_cov.hpp): bos_node_covariances,
// bos_associate_bearings (hip/associate.hpp), bos_match_landmarks and bos_match_poses (hip/match.hpp), their
// timing getters and chunk knobs. The calls' frame and the column-and-chunk loop are cov_call.hpp's.
#include <cmath>

#include "cov_call.hpp"

using namespace bos::capi;

namespace {

static_assert(bos::kMatchMaxK == bos::kAssocMaxK, "one list length for the association and the matching");

// What an association or matching call returns (host pointers, any of them null): per query the k best of N
// candidates, ascending, cand[0] their scores and cand[1], cand[2] what the call lists beside them, width[v]
// doubles per entry; the count inside the gate; every candidate's score
struct ListOutputs {
    int32_t* cand_ix;
    double* cand[3];
    int32_t* n_inside;
    double* all;
    size_t width[3], K, N;
    std::vector<double> dbuf;
    std::vector<int32_t> ibuf;

    bool select() const { return cand_ix || cand[0] || cand[1] || cand[2] || n_inside; }
    // the slots of all n queries as they stay where nothing is listed
    void pad(size_t n) {
        if (cand_ix) std::fill_n(cand_ix, n * K, -1);
        if (cand[0]) std::fill_n(cand[0], n * K, HUGE_VAL);
        for (int v = 1; v < 3; ++v)
            if (cand[v]) std::fill_n(cand[v], n * K * width[v], 0.0);
        if (n_inside) std::fill_n(n_inside, n, 0);
    }
    // A chunk's device results, the lists [rows][kAssocMaxK][stride[v]], the [rows] counts and the [rows][N]
    // scores: the small ones downloaded once each, then a row's k entries to the queries that receive it
    int download(size_t rows, const std::vector<bos::RowDest>& dst, const int32_t* d_ix, const double* const d_cand[3],
                 const size_t stride[3], const int32_t* d_inside, const double* d_all) {
        const size_t RK = rows * bos::kAssocMaxK;
        for (int v = 0; v < 3; ++v) {
            if (!cand[v]) continue;
            dbuf.resize(RK * stride[v]);
            HIP_TRY(hipMemcpy(dbuf.data(), d_cand[v], RK * stride[v] * sizeof(double), hipMemcpyDeviceToHost));
            bos::scatter_lists(dbuf.data(), bos::kAssocMaxK, stride[v], dst, K, width[v], cand[v]);
        }
        ibuf.resize(RK);
        if (cand_ix) {
            HIP_TRY(hipMemcpy(ibuf.data(), d_ix, RK * sizeof(int32_t), hipMemcpyDeviceToHost));
            bos::scatter_lists(ibuf.data(), bos::kAssocMaxK, 1, dst, K, 1, cand_ix);
        }
        if (n_inside) {
            HIP_TRY(hipMemcpy(ibuf.data(), d_inside, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (const bos::RowDest& rq : dst) n_inside[rq.second] = ibuf[rq.first];
        }
        for (size_t i = 0; i < dst.size() && all; ++i) {   // a row that several queries receive is downloaded once
            double* to = all + (size_t)dst[i].second * N;
            if (i > 0 && dst[i].first == dst[i - 1].first) std::copy_n(all + (size_t)dst[i - 1].second * N, N, to);
            else HIP_TRY(hipMemcpy(to, d_all + (size_t)dst[i].first * N, N * sizeof(double), hipMemcpyDeviceToHost));
        }
        return BOS_OK;
    }
};
constexpr size_t kAssocStride[3] = {1, 1, 1};
constexpr size_t kMatchStride[3] = {1, (size_t)bos::dev::kMatchDetailStride, (size_t)bos::dev::kMatchCovStride};

// bos_match_landmarks (zr null; node: the landmarks) and bos_match_poses (zr: [n][kMatchRowDoubles], z and
// the lower triangle of R; node: the poses), their arguments checked. Rows are grouped by query node, the
// nodes in the order of their first row: one column per node. A landmark's column gives one score row,
// copied to every query of that landmark; a pose's measurements are its rows, in chunks.
int match_pass(bos_solver* s, const char* name, int32_t n, const int32_t* node, const double* zr, double gate, ListOutputs& o,
               int32_t* solver_info) {
    int rc;
    const bool poses = zr != nullptr;
    const bool select = o.select(), rows_wanted = select || o.all;
    CovCall c{s, s->match_ms, 8, solver_info};
    if ((rc = c.begin())) return rc;
    if (s->plan.n == 0) {   // the fixed pose alone: there is no system to take a covariance from, no score
        o.pad((size_t)n);
        if (o.all) std::fill_n(o.all, (size_t)n * o.N, bos::match_nan());
        return BOS_OK;
    }
    const bos::RowGroups G = bos::group_rows_by_node(rows_wanted ? n : 0, node, o.N);
    const int widest = std::max(s->NP, s->NL);   // one set of buffers serves both calls
    int chunk_rows = bos::dev::match_budget_rows(widest);
    if (s->match_chunk > 0) chunk_rows = (int)std::min<int64_t>(chunk_rows, s->match_chunk);
    if (rows_wanted) {
        std::string err;
        if ((rc = node_cov_setup(s, name))) return rc;
        size_t largest = 1;
        for (const std::vector<int32_t>& m : G.members) largest = std::max(largest, poses ? m.size() : (size_t)1);
        if (!s->match) s->match = bos::dev::match_create();
        if (bos::dev::match_reserve(s->match, widest, (int)std::min<size_t>(largest, (size_t)chunk_rows), err))
            return fail(BOS_ERR_DEVICE, err);
    }
    if ((rc = c.factor())) return rc;
    if (!rows_wanted) return c.done();   // nothing asked for
    const bool want[4] = {false, false, poses, !poses};
    std::vector<double> rows_zr;
    bos::dev::MatchDev res;
    return column_chunks(
        c, G, poses ? 0 : s->NP, !poses, want, chunk_rows,
        [&](int a, const bos::dev::NodeCovDev& col, size_t rows, const std::vector<bos::RowDest>& dst, std::string& err) {
            if (!poses)
                return bos::dev::match_landmark_enqueue(s->match, s->NL, a, gate, select, col.projected_landmark, s->d_lm, s->stream,
                                                        s->ev[5], s->ev[6], &res, err);
            rows_zr.resize(rows * bos::dev::kMatchRowDoubles);
            for (size_t i = 0; i < rows; ++i)
                std::copy_n(zr + (size_t)dst[i].second * bos::dev::kMatchRowDoubles, bos::dev::kMatchRowDoubles,
                            rows_zr.begin() + i * bos::dev::kMatchRowDoubles);
            return bos::dev::match_pose_enqueue(s->match, s->NP, a, (int)rows, rows_zr.data(), gate, select, col.projected_pose, s->d_pose,
                                                s->stream, s->ev[5], s->ev[6], &res, err);
        },
        [&](size_t rows, const std::vector<bos::RowDest>& dst) {
            const double* const cand[3] = {res.cand_score, res.cand_detail, res.cand_cov};
            return o.download(rows, dst, res.cand_ix, cand, kMatchStride, res.n_inside, res.score);
        });
}

}  // namespace

extern "C" {

int bos_node_covariances(bos_solver* s, int32_t n_nodes, const int32_t* nodes, double* cross_pose, double* cross_landmark,
                         double* projected_pose, double* projected_landmark, double* pose_cov, double* landmark_cov,
                         int32_t* solver_info) {
    const char* name = "bos_node_covariances";
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
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
    CovCall c{s, s->node_ms, 7, solver_info};
    if ((rc = c.begin())) return rc;
    if (s->plan.n == 0) {   // the fixed pose alone
        for (int i = 0; i < 4; ++i)
            if (want[i]) std::fill(outs[i], outs[i] + (size_t)n_nodes * count[i], 0.0);
        if (pose_cov) std::fill(pose_cov, pose_cov + np9, 0.0);
        return BOS_OK;
    }
    if (any_node && (rc = node_cov_setup(s, name))) return rc;
    if ((rc = c.factor())) return rc;
    const double* sig = nullptr;
    if (need_sig && (rc = c.selected_inverse(&sig))) return rc;
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    for (int32_t q = 0; q < n_nodes && any_node; ++q) {
        std::string err;
        bos::dev::NodeCovDev res;
        HIP_TRY(hipEventRecord(s->ev[4], s->stream));
        const int prc = bos::dev::node_cov_enqueue(s->node, view, nodes[q], nodes[q] == s->plan.fixed, want, projected ? sig : nullptr,
                                                   s->d_pose, s->d_lm, s->stream, s->ev[5], &res, err);
        if ((rc = c.drain(6, prc, err))) return rc;
        s->node_ms[4] += elapsed(s->ev[4], s->ev[5]);
        s->node_ms[5] += elapsed(s->ev[5], s->ev[6]);
        const auto t_dl = Clock::now();
        const double* dev[4] = {res.cross_pose, res.cross_landmark, res.projected_pose, res.projected_landmark};
        for (int i = 0; i < 4; ++i)
            if (want[i]) HIP_TRY(hipMemcpy(outs[i] + (size_t)q * count[i], dev[i], count[i] * sizeof(double), hipMemcpyDeviceToHost));
        c.host_ms(6, t_dl);
    }
    const auto t_dl = Clock::now();
    if (pose_cov) HIP_TRY(hipMemcpy(pose_cov, sig, np9 * sizeof(double), hipMemcpyDeviceToHost));
    if (landmark_cov && nl4) HIP_TRY(hipMemcpy(landmark_cov, sig + np9, nl4 * sizeof(double), hipMemcpyDeviceToHost));
    c.host_ms(6, t_dl);
    return c.done();
}

int bos_node_covariances_timing(const bos_solver* s, double ms[7], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->node_ms, 7, ms, bytes, bos::dev::node_cov_bytes(s->node));
}

int bos_associate_bearings(bos_solver* s, int32_t n_bearings, const int32_t* pose, const double* z, const double* omega, double gate,
                           int32_t k, int32_t* cand_landmark, double* cand_nis, double* cand_innovation, double* cand_var,
                           int32_t* n_inside, double* nis_all, int32_t* solver_info) {
    const char* name = "bos_associate_bearings";
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
    if (const char* bad = bos::assoc_bad_argument(s->NP, n_bearings, pose, z, omega, gate, k))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_bearings == 0) return BOS_OK;
    ListOutputs o = {cand_landmark, {cand_nis, cand_innovation, cand_var}, n_inside, nis_all, {1, 1, 1}, (size_t)k, (size_t)s->NL, {}, {}};
    const bool select = o.select(), rows_wanted = s->NL > 0 && (select || nis_all);
    CovCall c{s, s->assoc_ms, 8, solver_info};
    if ((rc = c.begin())) return rc;
    if (s->plan.n == 0) {   // the fixed pose alone: no landmark
        o.pad((size_t)n_bearings);
        return BOS_OK;
    }
    const bos::RowGroups G = bos::group_rows_by_node(rows_wanted ? n_bearings : 0, pose, (size_t)s->NP);
    int chunk_rows = bos::dev::associate_budget_rows(s->NL);
    if (s->assoc_chunk > 0) chunk_rows = (int)std::min<int64_t>(chunk_rows, s->assoc_chunk);
    if (rows_wanted) {
        std::string err;
        if ((rc = node_cov_setup(s, name))) return rc;
        size_t largest = 0;
        for (const std::vector<int32_t>& m : G.members) largest = std::max(largest, m.size());
        if (!s->assoc) s->assoc = bos::dev::associate_create();
        if (bos::dev::associate_reserve(s->assoc, s->NL, (int)std::min<size_t>(largest, (size_t)chunk_rows), err))
            return fail(BOS_ERR_DEVICE, err);
    }
    if ((rc = c.factor())) return rc;
    if (!rows_wanted) {   // no landmark, or nothing asked for
        o.pad((size_t)n_bearings);
        return c.done();
    }
    const bool want[4] = {false, false, false, true};
    std::vector<double> zc, oc;
    bos::dev::AssociateDev res;
    return column_chunks(
        c, G, 0, false, want, chunk_rows,
        [&](int a, const bos::dev::NodeCovDev& col, size_t rows, const std::vector<bos::RowDest>& dst, std::string& err) {
            zc.resize(rows);
            oc.resize(rows);
            for (size_t i = 0; i < rows; ++i) {
                zc[i] = z[dst[i].second];
                oc[i] = omega ? omega[dst[i].second] : 1.0;
            }
            return bos::dev::associate_enqueue(s->assoc, a, (int)rows, zc.data(), oc.data(), gate, select, col.projected_landmark, s->d_pose,
                                               s->d_lm, s->stream, s->ev[5], s->ev[6], &res, err);
        },
        [&](size_t rows, const std::vector<bos::RowDest>& dst) {
            const double* const cand[3] = {res.cand_nis, res.cand_innovation, res.cand_var};
            return o.download(rows, dst, res.cand_landmark, cand, kAssocStride, res.n_inside, res.nis);
        });
}

int bos_associate_bearings_timing(const bos_solver* s, double ms[8], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->assoc_ms, 8, ms, bytes, bos::dev::associate_bytes(s->assoc));
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
    if ((rc = cov_handle_check(s, name))) return rc;
    if (const char* bad = bos::match_landmarks_bad_argument(s->NL, n_queries, landmark, gate, k))
        return fail(BOS_ERR_INVALID, std::string(name) + ": " + bad);
    if (n_queries == 0) return BOS_OK;
    ListOutputs o = {cand_landmark, {cand_d2, cand_diff, cand_cov}, n_inside, d2_all, {1, 2, 4}, (size_t)k, (size_t)s->NL, {}, {}};
    return match_pass(s, name, n_queries, landmark, nullptr, gate, o, solver_info);
}

int bos_match_poses(bos_solver* s, int32_t n_meas, const int32_t* pose, const double* z, const double* omega, double gate, int32_t k,
                    int32_t* cand_pose, double* cand_nis, double* cand_innovation, double* cand_cov, int32_t* n_inside, double* nis_all,
                    int32_t* solver_info) {
    const char* name = "bos_match_poses";
    int rc;
    if ((rc = cov_handle_check(s, name))) return rc;
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
    ListOutputs o = {cand_pose, {cand_nis, cand_innovation, cand_cov}, n_inside, nis_all, {1, 3, 9}, (size_t)k, (size_t)s->NP, {}, {}};
    return match_pass(s, name, n_meas, pose, zr.data(), gate, o, solver_info);
}

int bos_match_timing(const bos_solver* s, double ms[8], int64_t* bytes) {
    if (!s || !ms) return fail(BOS_ERR_INVALID, "null argument");
    return timing_out(s->match_ms, 8, ms, bytes, bos::dev::match_bytes(s->match));
}

int bos_debug_set_match_chunk(bos_solver* s, int64_t max_rows) {
    if (!s || max_rows < 0) return fail(BOS_ERR_INVALID, "bad argument");
    s->match_chunk = max_rows;
    return BOS_OK;
}

}  // extern "C"
