// Host-side C ABI (include/bos_host.h): datasets (g2o / synthetic) and plan inspection.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/bos_host.h"
#include "associate.hpp"
#include "match.hpp"
#include "jcbb.hpp"
#include "joint.hpp"
#include "edge_check.hpp"
#include "edge_cov.hpp"
#include "node_cov.hpp"
#include "pair_cov.hpp"
#include "g2o_utils.hpp"
#include "host_mf.hpp"
#include "plan.hpp"
#include "prior.hpp"
#include "synthetic.hpp"
#include "triangulation.hpp"

#include "error.hpp"

namespace {
int hfail(int code, const std::string& m) { return bos::set_error(code, m); }
}  // namespace

struct bos_dataset {
    proj02::State state;
    proj02::BearingObservationVector bearings;
    proj02::OdometryObservationVector odometry;
    int fixed_pose_id = -1;
    float bound = 0;
    // SoA problem view
    std::vector<double> pose_xyt, lm_xy, b_z, o_z, o_om;
    std::vector<int32_t> b_pose, b_lm, o_src, o_dst, pose_ids, lm_ids;
    int32_t fixed_stix = 0;
    bool has_gt = false;
    std::vector<double> gt_pose, gt_lm;

    int finalize() {
        const proj02::NEPoseVector& P = state.poses_vec();
        const proj02::LMPosVector& L = state.landmarks_vec();
        pose_xyt.resize(3 * P.size());
        for (size_t i = 0; i < P.size(); ++i) {
            pose_xyt[3 * i] = P[i].x; pose_xyt[3 * i + 1] = P[i].y; pose_xyt[3 * i + 2] = P[i].theta;
        }
        lm_xy.resize(2 * L.size());
        for (size_t j = 0; j < L.size(); ++j) { lm_xy[2 * j] = L[j].x; lm_xy[2 * j + 1] = L[j].y; }
        pose_ids.assign(state.pose_ids().begin(), state.pose_ids().end());
        lm_ids.assign(state.landmark_ids().begin(), state.landmark_ids().end());
        // id -> stix as flat tables when the ids are dense enough (else the State's maps); a repeated
        // id maps to its last stix, as the State's map does (state.cpp:23)
        auto flat = [](const std::vector<int32_t>& ids, std::vector<int32_t>& tab, int32_t& lo) {
            tab.clear();
            lo = 0;
            if (ids.empty()) return false;
            const auto mm = std::minmax_element(ids.begin(), ids.end());
            lo = *mm.first;
            const int64_t span = (int64_t)*mm.second - lo + 1;
            if (span > 4 * (int64_t)ids.size() + 1024) return false;
            tab.assign((size_t)span, -1);
            for (size_t i = 0; i < ids.size(); ++i) tab[(size_t)(ids[i] - lo)] = (int32_t)i;
            return true;
        };
        std::vector<int32_t> ptab, ltab;
        int32_t plo = 0, llo = 0;
        const bool pf = flat(pose_ids, ptab, plo), lf = flat(lm_ids, ltab, llo);
        auto pstix = [&](int id) -> int32_t {
            if (!pf) return state.pose_stix(id);
            const int64_t q = (int64_t)id - plo;
            if (q < 0 || q >= (int64_t)ptab.size() || ptab[(size_t)q] < 0) throw std::out_of_range("pose id");
            return ptab[(size_t)q];
        };
        auto lstix = [&](int id) -> int32_t {
            if (!lf) return state.landmark_stix(id);
            const int64_t q = (int64_t)id - llo;
            if (q < 0 || q >= (int64_t)ltab.size() || ltab[(size_t)q] < 0) throw std::out_of_range("landmark id");
            return ltab[(size_t)q];
        };
        try {
            b_pose.resize(bearings.size()); b_lm.resize(bearings.size()); b_z.resize(bearings.size());
            for (size_t k = 0; k < bearings.size(); ++k) {
                b_pose[k] = pstix(bearings[k].get_pose_id());
                b_lm[k] = lstix(bearings[k].get_lm_id());
                b_z[k] = bearings[k].get_bearing_angle();
            }
            o_src.resize(odometry.size()); o_dst.resize(odometry.size());
            o_z.resize(3 * odometry.size()); o_om.resize(9 * odometry.size());
            for (size_t k = 0; k < odometry.size(); ++k) {
                o_src[k] = pstix(odometry[k].get_source_id());
                o_dst[k] = pstix(odometry[k].get_dest_id());
                const proj02::EPose z = odometry[k].get_transformation();
                o_z[3 * k] = z.x; o_z[3 * k + 1] = z.y; o_z[3 * k + 2] = z.z;
                const proj02::Mat3 m = odometry[k].get_omega();
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) o_om[9 * k + 3 * r + c] = m(r, c);
            }
            fixed_stix = pstix(fixed_pose_id);
        } catch (const std::out_of_range&) {
            return hfail(BOS_ERR_INVALID, "an observation or FIX references an unknown id");
        }
        return BOS_OK;
    }
};

namespace {

bos::ProblemIndex index_of(const bos_problem* pb) {
    bos::ProblemIndex pi;
    pi.NP = pb->num_poses; pi.NL = pb->num_landmarks; pi.Mb = pb->num_bearings; pi.Mo = pb->num_odometry;
    pi.fixed = pb->fixed_pose;
    pi.b_pose = pb->bearing_pose; pi.b_lm = pb->bearing_landmark; pi.o_src = pb->odom_src; pi.o_dst = pb->odom_dst;
    pi.b_omega = pb->bearing_omega; pi.o_omega = pb->odom_omega;
    return pi;
}

}  // namespace

extern "C" {

int bos_dataset_load_g2o(const char* path, int triangulate, int verbose, bos_dataset** out) {
    if (!path || !out) return hfail(BOS_ERR_INVALID, "null argument");
    *out = nullptr;
    bos_dataset* d = new bos_dataset();
    const int rc = proj02::parse_g2o(path, d->state, d->bearings, d->odometry, d->fixed_pose_id, d->bound);
    if (rc) { delete d; return hfail(BOS_ERR_IO, rc == -1 ? "cannot open g2o file" : "malformed g2o line"); }
    if (d->state.number_of_poses() == 0) { delete d; return hfail(BOS_ERR_INVALID, "no poses"); }
    if (d->fixed_pose_id < 0) d->fixed_pose_id = d->state.default_pose_id();   // bearing_only_slam.cpp:63-65
    if (triangulate) proj02::triangulate_landmarks(d->state, d->bearings, verbose != 0);
    const int r2 = d->finalize();
    if (r2) { delete d; return r2; }
    *out = d;
    return BOS_OK;
}

double bos_normalized_angle_f64(double a) { return bos::normalized_angle<double>(a); }
float bos_normalized_angle_f32(float a) { return bos::normalized_angle<float>(a); }

int bos_prior_terms(int32_t kind, const double* node_state, const double* mean, const double* omega, double* A, double* g,
                    double* rho) {
    if (!node_state || !mean || !omega || !A || !g || !rho) return hfail(BOS_ERR_INVALID, "null argument");
    if (kind == 0) {
        const double u[6] = {omega[0], omega[1], omega[2], omega[4], omega[5], omega[8]};
        *rho = bos::prior_pose_terms<double>(node_state[0], node_state[1], node_state[2], mean, u, A, g);
    } else if (kind == 1) {
        const double u[3] = {omega[0], omega[1], omega[3]};
        *rho = bos::prior_landmark_terms<double>(node_state[0], node_state[1], mean, u, A, g);
    } else {
        return hfail(BOS_ERR_INVALID, "bos_prior_terms: kind must be 0 (pose) or 1 (landmark)");
    }
    return BOS_OK;
}

int bos_dataset_synthetic(int32_t num_poses, int32_t num_landmarks, int32_t bearings_per_pose, uint64_t seed,
                          bos_dataset** out) {
    if (!out) return hfail(BOS_ERR_INVALID, "null argument");
    *out = nullptr;
    proj02::SyntheticParams p;
    p.num_poses = num_poses;
    p.num_landmarks = num_landmarks;
    p.bearings_per_pose = bearings_per_pose;
    p.seed = seed;
    proj02::SyntheticWorld w;
    if (!proj02::make_synthetic(p, w)) return hfail(BOS_ERR_INVALID, "infeasible synthetic sizes");
    bos_dataset* d = new bos_dataset();
    d->state = w.initial_guess;
    d->bearings = std::move(w.bearings);
    d->odometry = std::move(w.odometry);
    d->fixed_pose_id = w.fixed_pose_id;
    proj02::triangulate_landmarks(d->state, d->bearings, false);
    const int rc = d->finalize();
    if (rc) { delete d; return rc; }
    // ground truth in the same stix order (landmark ids ascending in both states)
    d->has_gt = true;
    for (const proj02::NEPose& q : w.ground_truth.poses_vec()) {
        d->gt_pose.push_back(q.x); d->gt_pose.push_back(q.y); d->gt_pose.push_back(q.theta);
    }
    d->gt_lm.resize(2 * d->lm_ids.size());
    for (size_t j = 0; j < d->lm_ids.size(); ++j) {
        const proj02::LMPos l = w.ground_truth.get_landmark_by_id(d->lm_ids[j]);
        d->gt_lm[2 * j] = l.x; d->gt_lm[2 * j + 1] = l.y;
    }
    double b = 0;
    for (double v : d->gt_pose) b = std::max(b, std::fabs(v));
    d->bound = (float)b + 3.0f;
    *out = d;
    return BOS_OK;
}

int bos_dataset_problem(const bos_dataset* d, bos_problem* v) {
    if (!d || !v) return hfail(BOS_ERR_INVALID, "null argument");
    std::memset(v, 0, sizeof(*v));
    v->num_poses = (int32_t)d->pose_ids.size();
    v->num_landmarks = (int32_t)d->lm_ids.size();
    v->num_bearings = (int32_t)d->b_pose.size();
    v->num_odometry = (int32_t)d->o_src.size();
    v->pose_xyt = d->pose_xyt.data();
    v->landmark_xy = d->lm_xy.empty() ? nullptr : d->lm_xy.data();
    v->bearing_pose = d->b_pose.data();
    v->bearing_landmark = d->b_lm.data();
    v->bearing_z = d->b_z.data();
    v->bearing_omega = nullptr;
    v->odom_src = d->o_src.data();
    v->odom_dst = d->o_dst.data();
    v->odom_z = d->o_z.data();
    v->odom_omega = d->o_om.data();
    v->fixed_pose = d->fixed_stix;
    return BOS_OK;
}

const int32_t* bos_dataset_pose_ids(const bos_dataset* d) { return d ? d->pose_ids.data() : nullptr; }
const int32_t* bos_dataset_landmark_ids(const bos_dataset* d) { return d ? d->lm_ids.data() : nullptr; }
int32_t bos_dataset_fixed_pose_id(const bos_dataset* d) { return d ? d->fixed_pose_id : -1; }
float bos_dataset_bound(const bos_dataset* d) { return d ? d->bound : 0.f; }

int bos_dataset_ground_truth(const bos_dataset* d, const double** pose_xyt, const double** landmark_xy) {
    if (!d || !d->has_gt) return hfail(BOS_ERR_INVALID, "no ground truth");
    if (pose_xyt) *pose_xyt = d->gt_pose.data();
    if (landmark_xy) *landmark_xy = d->gt_lm.data();
    return BOS_OK;
}

int bos_dataset_write_g2o(const bos_dataset* d, const char* path, const double* pose_xyt, const double* landmark_xy,
                          int with_landmarks) {
    if (!d || !path) return hfail(BOS_ERR_INVALID, "null argument");
    proj02::State st((int)d->pose_ids.size(), (int)d->lm_ids.size());
    const double* P = pose_xyt ? pose_xyt : d->pose_xyt.data();
    const double* L = landmark_xy ? landmark_xy : d->lm_xy.data();
    for (size_t i = 0; i < d->pose_ids.size(); ++i) st.add_pose(P[3 * i], P[3 * i + 1], P[3 * i + 2], d->pose_ids[i]);
    for (size_t j = 0; j < d->lm_ids.size(); ++j) st.add_landmark(L[2 * j], L[2 * j + 1], d->lm_ids[j]);
    if (proj02::write_g2o(path, st, d->bearings, d->odometry, d->fixed_pose_id, with_landmarks != 0))
        return hfail(BOS_ERR_IO, "cannot write g2o file");
    return BOS_OK;
}

void bos_dataset_free(bos_dataset* d) { delete d; }

namespace {
int factor_mode_of(int32_t solver) {
    switch (solver) {
        case BOS_SOLVER_SUPERNODAL: return bos::kFactorMultifrontal;
        case BOS_SOLVER_SCHUR: return bos::kFactorSchur;
        case BOS_SOLVER_ROCSOLVER_RF: return bos::kFactorScalar;
        case BOS_SOLVER_DENSE_CHOL: return bos::kFactorNone;
        default: return -1;
    }
}

// The planning fields of an options struct (NULL = defaults): the problem index with the plan
// options, the factor mode, and the options themselves
int plan_args(const bos_problem* pb, const bos_options* in, bos::ProblemIndex& pi, int& fmode, bos_options& opt) {
    bos_default_options(&opt);
    if (in) opt = *in;
    fmode = factor_mode_of(opt.solver);
    if (fmode < 0) return hfail(BOS_ERR_INVALID, "unknown solver");
    if (opt.partition != BOS_PARTITION_SUBTREE && opt.partition != BOS_PARTITION_OBSERVATIONS)
        return hfail(BOS_ERR_INVALID, "unknown partition");
    pi = index_of(pb);
    pi.lpp = opt.lanes_per_pose;
    pi.schur_leaf = opt.schur_leaf;
    return BOS_OK;
}

// The plan of rank `rank` of `world`: BOS_PARTITION_OBSERVATIONS plans are one-GPU plans (every rank
// holds the whole structure and runs a range of its lanes)
int plan_for(const bos::ProblemIndex& pi, const bos_options& opt, int fmode, int rank, int world, bos::Plan& P,
             std::string& err) {
    if (opt.partition == BOS_PARTITION_OBSERVATIONS) return bos::build_plan(pi, 0, 1, fmode, P, err);
    return bos::build_plan(pi, rank, world, fmode, P, err);
}
}  // namespace

void bos_debug_set_g2o_parser(int32_t line_by_line) { proj02::g_g2o_line_parser = line_by_line != 0; }

int bos_plan_inspect(const bos_problem* pb, const bos_options* options, int32_t rank, int32_t world, int64_t capacity,
                     int32_t* ref_rows, int32_t* ref_cols, uint8_t* owned, uint8_t* b_owned, int32_t* perm_to_ref,
                     bos_plan_info* info) {
    if (!pb) return hfail(BOS_ERR_INVALID, "null problem");
    if (world < 1 || rank < 0 || rank >= world) return hfail(BOS_ERR_INVALID, "bad rank/world");
    bos::ProblemIndex pi;
    bos_options opt;
    int fmode = 0;
    int rc = plan_args(pb, options, pi, fmode, opt);
    if (rc) return rc;
    bos::Plan P;
    std::string err;
    rc = plan_for(pi, opt, fmode, rank, world, P, err);
    if (rc) return hfail(rc, err);
    // observations partition: this rank's share of the one-GPU plan's lanes
    const bool obs = opt.partition == BOS_PARTITION_OBSERVATIONS && world > 1;
    std::vector<char> lane_node;
    std::vector<uint8_t> own_e;
    if (obs) {
        int64_t pb0, pb1, lb0, lb1;
        bos::observation_lanes(P, rank, world, pb0, pb1, lb0, lb1, &lane_node);
        bos::owned_entries(P, lane_node, own_e);
    }
    const int NP = pi.NP;
    std::vector<int32_t> ref(P.n + 3);
    for (int u = 0; u < pi.NP + pi.NL; ++u) {
        const int sz = u < NP ? 3 : 2;
        const int r0 = u < NP ? 3 * u : 3 * NP + 2 * (u - NP);
        for (int d = 0; d < sz; ++d) ref[P.node_dof[u] + d] = r0 + d;
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->n = P.n;
        info->nnz_lower = P.nnzA();
        info->nnz_factor = P.mf.nsuper ? P.mf.L_size : P.nnzL();
        info->num_block_values = P.blk.size;
        info->lanes_per_pose = P.blk.lpp;
        info->flops_temporal = P.ordering.flops_temporal;
        info->flops_nested_dissection = P.ordering.flops_nd;
        info->mf_supernodes = P.mf.nsuper;
        info->mf_fold_fp32 = bos::mf_fold_reads_fp32(P) ? 1 : 0;
        for (int32_t p0 : P.blk.lm_lane_run) info->lm_lanes_consecutive += p0 >= 0;
        for (uint8_t c : P.blk.po_chain) info->pose_odometry_chain += c;
        info->mf_levels = P.mf.nlevels;
        info->mf_max_front = P.mf.max_m;
        info->mf_flops = P.mf.flops;
        info->mf_update_bytes = P.mf.U_size * 8;
        info->mf_fits = P.mf.fits;
        info->mf_max_front_upper = P.mf.max_m_upper;
        info->mf_balance_pct = P.mf.balance_pct;
        const bos::Shard& S = P.shard;
        info->shard_own_fronts = S.n_own_fronts;
        info->shard_top_fronts = S.n_top_fronts;
        info->shard_roots = S.root_ptr.empty() ? 0 : S.root_ptr[rank + 1] - S.root_ptr[rank];
        info->shard_ex1_doubles = S.ex1_count;
        info->shard_ex2_doubles = S.ex2_count;
        info->shard_pose_lanes = (int64_t)S.lane_poses.size();
        info->shard_own_pose_lanes = S.own_pose_lanes;
        info->shard_lm_lanes = (int64_t)S.lane_lms.size();
        info->shard_update_nodes = (int64_t)S.upd_nodes.size();
        std::strncpy(info->ordering, P.ordering.chosen.c_str(), sizeof(info->ordering) - 1);
    }
    if (ref_rows || ref_cols || owned) {
        if (capacity < P.nnzA()) return hfail(BOS_ERR_INVALID, "capacity < nnz_lower");
        for (int64_t r = 0; r < P.n; ++r)
            for (int64_t e = P.rowptr[r]; e < P.rowptr[r + 1]; ++e) {
                const int32_t a = ref[r], c = ref[P.colind[e]];
                if (ref_rows) ref_rows[e] = std::max(a, c);
                if (ref_cols) ref_cols[e] = std::min(a, c);
                if (owned) owned[e] = obs ? own_e[e] : P.blk.csr_src[e] >= 0 ? 1 : 0;
            }
    }
    if (perm_to_ref)
        for (int64_t i = 0; i < P.n + 3; ++i) perm_to_ref[i] = ref[i];
    if (b_owned) {   // b lives in the reference numbering; a lane writes its node's entries
        for (int64_t i = 0; i < P.n + 3; ++i) b_owned[i] = 0;
        for (int32_t p : P.blk.lane_pose)
            if (p >= 0 && (!obs || lane_node[p]))
                for (int d = 0; d < 3; ++d) b_owned[3 * (int64_t)p + d] = 1;
        for (int32_t l : P.blk.lm_lane_lm)
            if (!obs || lane_node[NP + l])
                for (int d = 0; d < 2; ++d) b_owned[3 * (int64_t)NP + 2 * (int64_t)l + d] = 1;
    }
    return BOS_OK;
}

int bos_plan_node_owner(const bos_problem* pb, const bos_options* options, int32_t world, int32_t* owner) {
    if (!pb || !owner || world < 1) return hfail(BOS_ERR_INVALID, "bad argument");
    bos::ProblemIndex pi;
    bos_options opt;
    int fmode = 0;
    int rc = plan_args(pb, options, pi, fmode, opt);
    if (rc) return rc;
    if (opt.partition == BOS_PARTITION_OBSERVATIONS)
        return hfail(BOS_ERR_UNSUPPORTED, "observations partition: every rank holds every node");
    bos::Plan P;
    std::string err;
    rc = bos::build_plan(pi, 0, world, fmode, P, err);
    if (rc) return hfail(rc, err);
    if (P.shard.node_owner.empty()) return hfail(BOS_ERR_UNSUPPORTED, "no shard (not a multifrontal solver)");
    std::copy(P.shard.node_owner.begin(), P.shard.node_owner.end(), owner);
    return BOS_OK;
}

// The fronts of the plan's tree (bos_host.h BOS_PLAN_FRONT_COLS): shapes, levels and links only.
int bos_plan_mf_fronts(const bos_problem* pb, const bos_options* options, int64_t capacity, int32_t* fronts, int32_t* nsuper) {
    if (!pb || (!fronts && !nsuper)) return hfail(BOS_ERR_INVALID, "null argument");
    bos::ProblemIndex pi;
    bos_options opt;
    int fmode = 0;
    int rc = plan_args(pb, options, pi, fmode, opt);
    if (rc) return rc;
    if (opt.solver != BOS_SOLVER_SUPERNODAL && opt.solver != BOS_SOLVER_SCHUR)
        return hfail(BOS_ERR_INVALID, "the fronts need a multifrontal solver");
    bos::Plan P;
    std::string err;
    rc = bos::build_plan(pi, 0, 1, fmode, P, err);
    if (rc) return hfail(rc, err);
    const bos::Multifrontal& F = P.mf;
    if (nsuper) *nsuper = F.nsuper;
    if (!fronts && capacity == 0) return BOS_OK;
    if (!fronts || capacity < (int64_t)BOS_PLAN_FRONT_COLS * F.nsuper) return hfail(BOS_ERR_INVALID, "fronts: capacity BOS_PLAN_FRONT_COLS * supernodes");
    std::vector<int32_t> lev(F.nsuper, -1), folded(F.nsuper, 0);
    for (int l = 0; l < F.nlevels; ++l)
        for (int q = F.level_ptr[l]; q < F.level_ptr[l + 1]; ++q) lev[F.level[q]] = l;
    for (int32_t x : F.fold_list) folded[x] = 1;
    std::vector<int32_t> out_ptr, out_rec;
    bos::CrossRecords cr;
    if (!bos::selinv_records(P, out_ptr, out_rec) ||
        !bos::selinv_cross_records(P, pi.Mb, pi.Mo, pi.b_pose, pi.b_lm, pi.o_src, pi.o_dst, cr))
        return hfail(BOS_ERR_UNSUPPORTED, "a node or an edge's cross block is not inside one front");
    for (int x = 0; x < F.nsuper; ++x) {
        int32_t* o = fronts + (size_t)BOS_PLAN_FRONT_COLS * x;
        o[0] = F.k[x]; o[1] = F.r[x]; o[2] = lev[x]; o[3] = F.parent[x];
        o[4] = F.child_ptr[x + 1] - F.child_ptr[x];
        o[5] = F.fold_cnt.empty() ? 0 : F.fold_cnt[x];
        o[6] = folded[x];
        o[7] = out_ptr[x + 1] - out_ptr[x];
        o[8] = o[9] = o[10] = 0;
        for (int q = cr.ptr[x]; q < cr.ptr[x + 1]; ++q) {
            const int32_t* rec = cr.rec.data() + (size_t)bos::kCrossRec * q;
            ++o[rec[0] >= F.k[x] ? 8 : 9];
            o[10] += rec[5];
        }
    }
    return BOS_OK;
}

// Test hook: runs the multifrontal algorithm of hip/multifrontal.hip on the host with the plan's
// tree and maps (validates the symbolic structure without a GPU). vals: values of the stored
// entries of H_nf in bos_plan_inspect's order (scattered into the block array here), rhs / x:
// permuted order of length n. Not used by any solve path.
int bos_plan_mf_selftest(const bos_problem* pb, const bos_options* options, const double* vals, const double* rhs,
                         double* x) {
    if (!pb || !vals || !rhs || !x) return hfail(BOS_ERR_INVALID, "null argument");
    bos::ProblemIndex pi;
    bos_options opt;
    int fmode = 0;
    int rc = plan_args(pb, options, pi, fmode, opt);
    if (rc) return rc;
    if (opt.solver != BOS_SOLVER_SUPERNODAL && opt.solver != BOS_SOLVER_SCHUR)
        return hfail(BOS_ERR_INVALID, "selftest needs a multifrontal solver");
    bos::Plan P;
    std::string err;
    rc = bos::build_plan(pi, 0, 1, fmode, P, err);
    if (rc) return hfail(rc, err);
    bos::HostMf M(P, vals, rhs);
    auto all = [](int) { return true; };
    M.factor(all);
    M.forward(all);
    M.backward(all);
    std::copy(M.x.begin(), M.x.end(), x);
    return BOS_OK;
}

// Test hook: the selected inverse (HostMf::selected_inverse) of the host factorization of H_nf given
// by vals (bos_plan_inspect's order): the marginal covariance block of every node.
int bos_plan_mf_marginals(const bos_problem* pb, const bos_options* options, const double* vals, double* pose_cov,
                          double* landmark_cov) {
    if (!pb || !vals || !pose_cov || (!landmark_cov && pb->num_landmarks > 0)) return hfail(BOS_ERR_INVALID, "null argument");
    bos::ProblemIndex pi;
    bos_options opt;
    int fmode = 0;
    int rc = plan_args(pb, options, pi, fmode, opt);
    if (rc) return rc;
    if (opt.solver != BOS_SOLVER_SUPERNODAL && opt.solver != BOS_SOLVER_SCHUR)
        return hfail(BOS_ERR_INVALID, "marginals need a multifrontal solver");
    bos::Plan P;
    std::string err;
    rc = bos::build_plan(pi, 0, 1, fmode, P, err);
    if (rc) return hfail(rc, err);
    const std::vector<double> rhs(P.n, 0.0);
    bos::HostMf M(P, vals, rhs.data());
    M.factor([](int) { return true; });
    double none = 0.0;
    if (!M.selected_inverse(pose_cov, landmark_cov ? landmark_cov : &none))
        return hfail(BOS_ERR_INVALID, "a node's dofs are split between two supernodes");
    return BOS_OK;
}

// Test hook: bos_edge_covariances in its literal host form: the host factorization and selected inverse
// with the cross records' emission (plan.hpp selinv_cross_records), then the per-edge projection of
// edge_cov.hpp at the problem's state (theta wrapped as bos_create wraps it).
int bos_plan_mf_edge_covariances(const bos_problem* pb, const bos_options* options, const double* vals, double* bearing_cross,
                                 double* odom_cross, double* bearing_var, double* odom_cov, double* pose_cov,
                                 double* landmark_cov) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0)) return hfail(BOS_ERR_INVALID, "null argument");
    bos::ProblemIndex pi;
    bos_options opt;
    int fmode = 0;
    int rc = plan_args(pb, options, pi, fmode, opt);
    if (rc) return rc;
    if (opt.solver != BOS_SOLVER_SUPERNODAL && opt.solver != BOS_SOLVER_SCHUR)
        return hfail(BOS_ERR_INVALID, "edge covariances need a multifrontal solver");
    bos::Plan P;
    std::string err;
    rc = bos::build_plan(pi, 0, 1, fmode, P, err);
    if (rc) return hfail(rc, err);
    bos::CrossRecords cr;
    if (!bos::selinv_cross_records(P, pi.Mb, pi.Mo, pi.b_pose, pi.b_lm, pi.o_src, pi.o_dst, cr))
        return hfail(BOS_ERR_UNSUPPORTED, "bos_edge_covariances: an edge's cross block is not inside one front");
    const std::vector<double> rhs(P.n, 0.0);
    bos::HostMf M(P, vals, rhs.data());
    M.factor([](int) { return true; });
    std::vector<double> pc(9 * (size_t)P.NP + 1), lc(4 * (size_t)P.NL + 1), pairs(9 * (size_t)cr.n_pairs + 1, 0.0);
    if (!M.selected_inverse(pc.data(), lc.data(), &cr, pairs.data()))
        return hfail(BOS_ERR_UNSUPPORTED, "a node's dofs are split between two supernodes");
    std::vector<double> pose(pb->pose_xyt, pb->pose_xyt + 3 * (size_t)P.NP);
    for (int i = 0; i < P.NP; ++i) pose[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(pose[3 * i + 2]));
    bos::EdgeCovIn in;
    in.Mb = pi.Mb; in.Mo = pi.Mo;
    in.pose = pose.data(); in.lm = pb->landmark_xy;
    in.pose_cov = pc.data(); in.lm_cov = lc.data(); in.pairs = pairs.data();
    in.b_pose = pi.b_pose; in.b_lm = pi.b_lm; in.o_src = pi.o_src; in.o_dst = pi.o_dst;
    in.edge_slot = cr.edge_slot.data(); in.edge_tr = cr.edge_tr.data();
    bos::EdgeCovOut o;
    o.bearing_cross = bearing_cross; o.odom_cross = odom_cross; o.bearing_var = bearing_var; o.odom_cov = odom_cov;
    for (int64_t e = 0; e < pi.Mb; ++e) bos::edge_cov_bearing(in, o, e);
    for (int64_t e = 0; e < pi.Mo; ++e) bos::edge_cov_odometry(in, o, e);
    if (pose_cov) std::copy(pc.begin(), pc.end() - 1, pose_cov);
    if (landmark_cov) std::copy(lc.begin(), lc.end() - 1, landmark_cov);
    return BOS_OK;
}

namespace {
// One kind's lists of bos_plan_mf_edge_consistency: the edges whose w2 is finite and >= gate in a stable sort,
// descending (equal w2 keep the lower index first), the k first listed with their e (D doubles) and T (D x D)
void edge_check_lists(const std::vector<double>& w2, double gate, size_t k, size_t D, const std::vector<double>& e, const std::vector<double>& T,
                      int32_t* cand, double* cand_w2, double* cand_e, double* cand_T, int32_t* n_over) {
    std::vector<int32_t> over;
    for (size_t i = 0; i < w2.size(); ++i)
        if (std::isfinite(w2[i]) && w2[i] >= gate) over.push_back((int32_t)i);
    std::stable_sort(over.begin(), over.end(), [&](int32_t x, int32_t y) { return w2[x] > w2[y]; });
    for (size_t j = 0; j < k; ++j) {
        const bool listed = j < over.size();
        const size_t i = listed ? (size_t)over[j] : 0;
        if (cand) cand[j] = listed ? over[j] : -1;
        if (cand_w2) cand_w2[j] = listed ? w2[i] : -HUGE_VAL;
        for (size_t v = 0; v < D && cand_e; ++v) cand_e[j * D + v] = listed ? e[i * D + v] : 0.0;
        for (size_t v = 0; v < D * D && cand_T; ++v) cand_T[j * D * D + v] = listed ? T[i * D * D + v] : 0.0;
    }
    if (n_over) *n_over = (int32_t)over.size();
}
}  // namespace

// Test hook: bos_edge_consistency in its literal host form: bearing_var / odom_cov of
// bos_plan_mf_edge_covariances, the per-edge evaluation of edge_check.hpp at the problem's state (theta wrapped
// as bos_create wraps it, Omega by its upper triangle), then a plain stable sort per kind.
int bos_plan_mf_edge_consistency(const bos_problem* pb, const bos_options* options, const double* vals, double gate_bearing,
                                 double gate_odom, int32_t k, int32_t* cand_bearing, double* cand_bearing_w2,
                                 double* cand_bearing_innovation, double* cand_bearing_resvar, int32_t* n_over_bearing,
                                 int32_t* cand_odom, double* cand_odom_w2, double* cand_odom_innovation, double* cand_odom_rescov,
                                 int32_t* n_over_odom, double* bearing_w2, double* bearing_chi2, double* bearing_redundancy,
                                 double* odom_w2, double* odom_chi2, double* odom_redundancy) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0)) return hfail(BOS_ERR_INVALID, "null argument");
    if (const char* bad = bos::edge_check_bad_argument(gate_bearing, gate_odom, k))
        return hfail(BOS_ERR_INVALID, std::string("bos_edge_consistency: ") + bad);
    const size_t Mb = (size_t)pb->num_bearings, Mo = (size_t)pb->num_odometry, NP = (size_t)pb->num_poses;
    // P: zero everywhere when the fixed pose is the only node (there is no system then)
    std::vector<double> var(Mb + 1, 0.0), cov(9 * Mo + 1, 0.0);
    if (3 * (NP - 1) + 2 * (size_t)pb->num_landmarks > 0) {
        const int rc = bos_plan_mf_edge_covariances(pb, options, vals, nullptr, nullptr, var.data(), cov.data(), nullptr, nullptr);
        if (rc) return rc;
    }
    std::vector<double> pose(pb->pose_xyt, pb->pose_xyt + 3 * NP);
    for (size_t i = 0; i < NP; ++i) pose[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(pose[3 * i + 2]));
    std::vector<double> bw(Mb), be(Mb), bT(Mb);
    for (size_t i = 0; i < Mb; ++i) {
        const size_t p = (size_t)pb->bearing_pose[i], l = (size_t)pb->bearing_landmark[i];
        const double th = pose[3 * p + 2];
        double gx, gy;
        const double e = bos::bearing_error<double>(pose[3 * p], pose[3 * p + 1], std::cos(th), std::sin(th), pb->landmark_xy[2 * l],
                                                    pb->landmark_xy[2 * l + 1], pb->bearing_z[i], gx, gy);
        const bos::EdgeCheckBearing r = bos::edge_check_bearing(e, pb->bearing_omega ? pb->bearing_omega[i] : 1.0, var[i]);
        bw[i] = r.w2; be[i] = r.e; bT[i] = r.T;
        if (bearing_w2) bearing_w2[i] = r.w2;
        if (bearing_chi2) bearing_chi2[i] = r.chi2;
        if (bearing_redundancy) bearing_redundancy[i] = r.redundancy;
    }
    std::vector<double> ow(Mo), oe(3 * Mo), oT(9 * Mo);
    for (size_t j = 0; j < Mo; ++j) {
        const size_t a = (size_t)pb->odom_src[j], d = (size_t)pb->odom_dst[j];
        const double* m = pb->odom_omega + 9 * j;
        const double* z = pb->odom_z + 3 * j;
        const double u[6] = {m[0], m[1], m[2], m[4], m[5], m[8]};
        double e[3], J[18], R[6];
        bos::odometry_error_jacobian<double>(pose[3 * a], pose[3 * a + 1], pose[3 * a + 2], std::cos(pose[3 * a + 2]), std::sin(pose[3 * a + 2]),
                                             pose[3 * d], pose[3 * d + 1], pose[3 * d + 2], z[0], z[1], z[2], e, J);
        bos::edge_check_information_inverse(u, R);
        bos::EdgeCheckOdom r;
        bos::edge_check_odometry(e, u, R, cov.data() + 9 * j, a == d, r);
        ow[j] = r.w2;
        std::copy_n(r.e, 3, oe.begin() + 3 * j);
        std::copy_n(r.T, 9, oT.begin() + 9 * j);
        if (odom_w2) odom_w2[j] = r.w2;
        if (odom_chi2) odom_chi2[j] = r.chi2;
        if (odom_redundancy) odom_redundancy[j] = r.redundancy;
    }
    edge_check_lists(bw, gate_bearing, (size_t)k, 1, be, bT, cand_bearing, cand_bearing_w2, cand_bearing_innovation, cand_bearing_resvar,
                     n_over_bearing);
    edge_check_lists(ow, gate_odom, (size_t)k, 3, oe, oT, cand_odom, cand_odom_w2, cand_odom_innovation, cand_odom_rescov, n_over_odom);
    return BOS_OK;
}

namespace {
// the one-GPU multifrontal plan of the pair hooks and its path data
static int pair_plan(const bos_problem* pb, const bos_options* options, bos::ProblemIndex& pi, bos::Plan& P, bos::PairPaths& pp) {
    bos_options opt;
    int fmode = 0;
    int rc = plan_args(pb, options, pi, fmode, opt);
    if (rc) return rc;
    if (opt.solver != BOS_SOLVER_SUPERNODAL && opt.solver != BOS_SOLVER_SCHUR)
        return hfail(BOS_ERR_INVALID, "pair covariances need a multifrontal solver");
    std::string err;
    rc = bos::build_plan(pi, 0, 1, fmode, P, err);
    if (rc) return hfail(rc, err);
    if (!bos::pair_paths_build(P, pp, err)) return hfail(BOS_ERR_UNSUPPORTED, err);
    return BOS_OK;
}
}  // namespace

// Test hook: bos_pair_covariances in its literal host form (csrc/host/pair_cov.hpp): the host
// factorization, one root-path solve per distinct node, the products in row order and the per-query
// projection the device kernel runs, at the problem's state (theta wrapped as bos_create wraps it).
int bos_plan_mf_pair_covariances(const bos_problem* pb, const bos_options* options, const double* vals, int64_t n_pairs,
                                 const int32_t* node_a, const int32_t* node_b, double* cross, double* projected, double* cov_a,
                                 double* cov_b) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0) || n_pairs < 0 ||
        (n_pairs > 0 && (!node_a || !node_b)))
        return hfail(BOS_ERR_INVALID, "bad argument");
    if (n_pairs == 0) return BOS_OK;
    if (!bos::pair_ids_valid(pb->num_poses, pb->num_landmarks, n_pairs, node_a, node_b))
        return hfail(BOS_ERR_INVALID, "bos_pair_covariances: a node id outside [0, NP + NL), or a mixed pair not written (pose, landmark)");
    bos::ProblemIndex pi;
    bos::Plan P;
    bos::PairPaths pp;
    const int rc = pair_plan(pb, options, pi, P, pp);
    if (rc) return rc;
    const std::vector<double> rhs(P.n, 0.0);
    bos::HostMf M(P, vals, rhs.data());
    M.factor([](int) { return true; });
    std::vector<int32_t> slot_of((size_t)P.NP + P.NL, -1);
    bos::PairBatchHost B;
    bos::pair_batch_build(P, pp, n_pairs, node_a, node_b, 0, INT64_MAX, INT64_MAX, INT64_MAX, slot_of, B);
    const size_t nn = B.n_node.size();
    std::vector<double> Y((size_t)B.y_count + 1), diag(9 * nn + 1), cb(9 * (size_t)n_pairs);
    for (size_t i = 0; i < nn; ++i) {
        double* Yi = Y.data() + B.y_off[i];
        bos::pair_path_solve_host(P.mf, pp, M.L.data(), B.n_sn[i], B.n_loc[i], B.n_d[i], Yi);
        bos::pair_product_host(Yi, 0, B.n_d[i], Yi, 0, B.n_d[i], B.n_len[i], true, diag.data() + 9 * i);
    }
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int sa = B.q_slot_a[q], sb = B.q_slot_b[q];
        const int da = node_a[q] < P.NP ? 3 : 2, db = node_b[q] < P.NP ? 3 : 2;
        const bool free2 = sa >= 0 && sb >= 0;
        bos::pair_product_host(Y.data() + (free2 ? B.y_off[sa] : 0), B.q_off_a[q], da, Y.data() + (free2 ? B.y_off[sb] : 0), B.q_off_b[q],
                               db, free2 ? B.q_c[q] : 0, false, cb.data() + 9 * q);
    }
    std::vector<double> pose(pb->pose_xyt, pb->pose_xyt + 3 * (size_t)P.NP);
    for (int i = 0; i < P.NP; ++i) pose[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(pose[3 * i + 2]));
    bos::PairQueryIn in;
    in.NP = P.NP; in.pose = pose.data(); in.lm = pb->landmark_xy;
    in.node_a = node_a; in.node_b = node_b; in.slot_a = B.q_slot_a.data(); in.slot_b = B.q_slot_b.data();
    in.crossbuf = cb.data(); in.diag = diag.data();
    bos::PairQueryOut o;
    o.cross = cross; o.projected = projected; o.cov_a = cov_a; o.cov_b = cov_b;
    for (int64_t q = 0; q < n_pairs; ++q) bos::pair_cov_query(in, o, q);
    return BOS_OK;
}

namespace {
// What the node and association hooks share: the plan, the host factorization with its selected inverse
// (need_sig) and the state (theta wrapped as bos_create wraps it); column(a, o): node a's root-path solve,
// the scatter into X, the backward sweep over every front and the per-target gather and projection the
// device kernel runs, into o.
struct NodeColumnHost {
    bos::ProblemIndex pi;
    bos::Plan P;
    bos::PairPaths pp;
    bos::NodeCovPlan np;
    std::vector<double> rhs, sig, pose, Y, X;
    std::unique_ptr<bos::HostMf> M;
    const double* lm = nullptr;
    bool have_sig = false;

    int setup(const bos_problem* pb, const bos_options* options, const double* vals, bool need_sig) {
        const int rc = pair_plan(pb, options, pi, P, pp);
        if (rc) return rc;
        std::string err;
        if (!bos::node_cov_plan_build(P, pp, np, err)) return hfail(BOS_ERR_UNSUPPORTED, err);
        rhs.assign(P.n, 0.0);
        M.reset(new bos::HostMf(P, vals, rhs.data()));
        M->factor([](int) { return true; });
        const size_t np9 = 9 * (size_t)P.NP, nl4 = 4 * (size_t)P.NL;
        sig.resize(np9 + nl4 + 1);
        have_sig = need_sig;
        if (need_sig && !M->selected_inverse(sig.data(), sig.data() + np9))
            return hfail(BOS_ERR_UNSUPPORTED, "a node's dofs are split between two supernodes");
        pose.assign(pb->pose_xyt, pb->pose_xyt + 3 * (size_t)P.NP);
        for (int i = 0; i < P.NP; ++i) pose[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(pose[3 * i + 2]));
        lm = pb->landmark_xy;
        Y.resize(3 * (size_t)np.max_path + 1);
        X.resize(3 * (size_t)P.n + 1);
        return BOS_OK;
    }

    void column(int a, const bos::NodeCovOut& o) {
        const int d = a < P.NP ? 3 : 2;
        const bool fixed = a == P.fixed;
        if (!fixed) {
            bos::pair_path_solve_host(P.mf, pp, M->L.data(), pp.node_sn[a], pp.node_loc[a], d, Y.data());
            bos::node_cov_scatter_host(P.mf, pp, P.n, pp.node_sn[a], d, Y.data(), X.data());
            bos::node_cov_backward_host(P.mf, np, M->L.data(), d, X.data());
        }
        bos::NodeCovIn in;
        in.NP = P.NP; in.NL = P.NL; in.a = a; in.d = d; in.n = P.n;
        in.pose = pose.data(); in.lm = lm; in.X = fixed ? nullptr : X.data(); in.node_dof = P.node_dof.data();
        in.sig = have_sig ? sig.data() : nullptr;
        for (int u = 0; u < P.NP + P.NL; ++u) bos::node_cov_target(in, o, u);
    }
};
}  // namespace

// Test hook: bos_node_covariances in its literal host form (csrc/host/node_cov.hpp): the host
// factorization, per query node the root-path solve, the scatter into X and the backward sweep over every
// front, the host selected inverse for the diagonal blocks, and the per-target gather and projection the
// device kernel runs, at the problem's state (theta wrapped as bos_create wraps it).
int bos_plan_mf_node_covariances(const bos_problem* pb, const bos_options* options, const double* vals, int32_t n_nodes,
                                 const int32_t* nodes, double* cross_pose, double* cross_landmark, double* projected_pose,
                                 double* projected_landmark, double* pose_cov, double* landmark_cov) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0) || n_nodes < 0 || (n_nodes > 0 && !nodes))
        return hfail(BOS_ERR_INVALID, "bad argument");
    if (n_nodes == 0) return BOS_OK;
    if (!bos::node_ids_valid(pb->num_poses, pb->num_landmarks, n_nodes, nodes))
        return hfail(BOS_ERR_INVALID, "bos_node_covariances: a node id outside [0, NP + NL)");
    NodeColumnHost H;
    const int rc = H.setup(pb, options, vals, projected_pose || projected_landmark || pose_cov || landmark_cov);
    if (rc) return rc;
    const size_t np9 = 9 * (size_t)H.P.NP, nl4 = 4 * (size_t)H.P.NL, nl6 = 6 * (size_t)H.P.NL;
    for (int32_t q = 0; q < n_nodes; ++q) {
        bos::NodeCovOut o;
        o.cross_pose = cross_pose ? cross_pose + q * np9 : nullptr;
        o.cross_landmark = cross_landmark ? cross_landmark + q * nl6 : nullptr;
        o.projected_pose = projected_pose ? projected_pose + q * np9 : nullptr;
        o.projected_landmark = projected_landmark ? projected_landmark + q * nl4 : nullptr;
        H.column(nodes[q], o);
    }
    if (pose_cov) std::copy(H.sig.begin(), H.sig.begin() + np9, pose_cov);
    if (landmark_cov) std::copy(H.sig.begin() + np9, H.sig.begin() + np9 + nl4, landmark_cov);
    return BOS_OK;
}

// Test hook: bos_associate_bearings in its literal host form (csrc/host/associate.hpp): per distinct pose
// the node hook's column for projected_landmark, per bearing e, S and nis by the shared code, then a plain
// sort of the landmarks inside the gate by (nis, stix).
int bos_plan_mf_associate_bearings(const bos_problem* pb, const bos_options* options, const double* vals, int32_t n_bearings,
                                   const int32_t* pose, const double* z, const double* omega, double gate, int32_t k,
                                   int32_t* cand_landmark, double* cand_nis, double* cand_innovation, double* cand_var,
                                   int32_t* n_inside, double* nis_all) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0)) return hfail(BOS_ERR_INVALID, "bad argument");
    if (const char* bad = bos::assoc_bad_argument(pb->num_poses, n_bearings, pose, z, omega, gate, k))
        return hfail(BOS_ERR_INVALID, std::string("bos_associate_bearings: ") + bad);
    if (n_bearings == 0) return BOS_OK;
    NodeColumnHost H;
    const int rc = H.setup(pb, options, vals, true);
    if (rc) return rc;
    const size_t NL = (size_t)H.P.NL, K = (size_t)k;
    std::vector<double> var(4 * NL + 1), row(NL + 1), e(NL + 1), S(NL + 1);
    std::vector<int32_t> inside;
    int last_pose = -1;
    for (int32_t q = 0; q < n_bearings; ++q) {
        const int a = pose[q];
        if (a != last_pose) {   // the column depends on the pose alone
            bos::NodeCovOut o;
            o.projected_landmark = var.data();
            H.column(a, o);
            last_pose = a;
        }
        const bos::AssocFrame f = bos::assoc_frame(H.pose.data(), a);
        inside.clear();
        for (size_t l = 0; l < NL; ++l) {
            e[l] = bos::assoc_innovation(f, H.lm[2 * l], H.lm[2 * l + 1], z[q]);
            S[l] = bos::assoc_innovation_var(var[4 * l], omega ? omega[q] : 1.0);
            row[l] = bos::assoc_nis(e[l], S[l]);
            if (bos::assoc_inside(row[l], gate)) inside.push_back((int32_t)l);
        }
        std::sort(inside.begin(), inside.end(), [&](int32_t x, int32_t y) { return bos::assoc_less(row[x], x, row[y], y); });
        for (size_t j = 0; j < K; ++j) {
            const bool listed = j < inside.size();
            const int32_t l = listed ? inside[j] : -1;
            if (cand_landmark) cand_landmark[q * K + j] = l;
            if (cand_nis) cand_nis[q * K + j] = listed ? row[l] : HUGE_VAL;
            if (cand_innovation) cand_innovation[q * K + j] = listed ? e[l] : 0.0;
            if (cand_var) cand_var[q * K + j] = listed ? S[l] : 0.0;
        }
        if (n_inside) n_inside[q] = (int32_t)inside.size();
        if (nis_all) std::copy(row.begin(), row.begin() + NL, nis_all + q * NL);
    }
    return BOS_OK;
}

// Test hook: bos_joint_compatibility in its literal host form (csrc/host/joint.hpp): the host factorization,
// per batch the pair hook's path solves and products for the batch's distinct nodes and node pairs, then per
// hypothesis e, J, S through its table, the serial recurrence and the prefixes, at the problem's state (theta
// wrapped as bos_create wraps it).
int bos_plan_mf_joint_compatibility(const bos_problem* pb, const bos_options* options, const double* vals, int32_t n_hyp,
                                    const int32_t* hyp_start, const int32_t* pose, const int32_t* landmark, const double* z,
                                    const double* omega, int64_t max_batch, double* prefix_nis, double* joint_nis,
                                    double* innovation, double* innovation_cov) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0) || max_batch < 0)
        return hfail(BOS_ERR_INVALID, "bad argument");
    if (const char* bad = bos::joint_bad_argument(pb->num_poses, pb->num_landmarks, n_hyp, hyp_start, pose, landmark, z, omega))
        return hfail(BOS_ERR_INVALID, std::string("bos_joint_compatibility: ") + bad);
    if (n_hyp == 0) return BOS_OK;
    bos::ProblemIndex pi;
    bos::Plan P;
    bos::PairPaths pp;
    const int rc = pair_plan(pb, options, pi, P, pp);
    if (rc) return rc;
    const std::vector<double> rhs(P.n, 0.0);
    bos::HostMf M(P, vals, rhs.data());
    M.factor([](int) { return true; });
    std::vector<double> state(pb->pose_xyt, pb->pose_xyt + 3 * (size_t)P.NP);
    for (int i = 0; i < P.NP; ++i) state[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(state[3 * i + 2]));
    std::vector<int32_t> slot_of((size_t)P.NP + P.NL, -1);
    bos::JointBatchHost B;
    std::vector<double> Y, diag, cross;
    int64_t s_done = 0;
    for (int32_t h0 = 0; h0 < n_hyp; h0 += B.nh) {
        bos::joint_batch_build(P, pp, n_hyp, hyp_start, pose, landmark, h0, INT64_MAX, max_batch > 0 ? max_batch : INT64_MAX, INT64_MAX,
                               slot_of, B);
        const bos::PairBatchHost& Q = B.pairs;
        const size_t nn = Q.n_node.size();
        Y.assign((size_t)Q.y_count + 1, 0.0);
        diag.assign(9 * nn + 1, 0.0);
        cross.assign(9 * (size_t)Q.nq + 1, 0.0);
        for (size_t i = 0; i < nn; ++i) {
            double* Yi = Y.data() + Q.y_off[i];
            bos::pair_path_solve_host(P.mf, pp, M.L.data(), Q.n_sn[i], Q.n_loc[i], Q.n_d[i], Yi);
            bos::pair_product_host(Yi, 0, Q.n_d[i], Yi, 0, Q.n_d[i], Q.n_len[i], true, diag.data() + 9 * i);
        }
        for (int64_t q = 0; q < Q.nq; ++q) {
            const int sa = Q.q_slot_a[q], sb = Q.q_slot_b[q];
            const int da = B.pair_a[q] < P.NP ? 3 : 2, db = B.pair_b[q] < P.NP ? 3 : 2;
            const bool free2 = sa >= 0 && sb >= 0;
            bos::pair_product_host(Y.data() + (free2 ? Q.y_off[sa] : 0), Q.q_off_a[q], da, Y.data() + (free2 ? Q.y_off[sb] : 0),
                                   Q.q_off_b[q], db, free2 ? Q.q_c[q] : 0, false, cross.data() + 9 * q);
        }
        for (int32_t h = h0; h < h0 + B.nh; ++h) {
            const int32_t p0 = hyp_start[h], m = hyp_start[h + 1] - p0;
            double J[5 * bos::kJointMaxM], om[bos::kJointMaxM], y[bos::kJointMaxM], pre[bos::kJointMaxM];
            double A[bos::kJointMaxM * bos::kJointLd];
            for (int32_t i = 0; i < m; ++i) {
                y[i] = bos::joint_innovation(state.data(), pb->landmark_xy, pose[p0 + i], landmark[p0 + i], z[p0 + i], J + 5 * i);
                om[i] = omega ? omega[p0 + i] : 1.0;
                if (innovation) innovation[p0 + i] = y[i];
            }
            bos::JointEntryIn in;
            in.pose = state.data(); in.lm = pb->landmark_xy; in.diag = diag.data(); in.cross = cross.data();
            in.tab = B.tab.data() + 4 * B.tab_off[h - h0];
            in.J = J; in.omega = om;
            double* cov = innovation_cov ? innovation_cov + s_done + B.s_off[h - h0] : nullptr;
            for (int32_t i = 0; i < m; ++i)
                for (int32_t j = 0; j <= i; ++j) {
                    const double v = bos::joint_S_entry(in, i, j);
                    A[i * bos::kJointLd + j] = v;
                    A[j * bos::kJointLd + i] = v;
                    if (cov) {
                        cov[i * m + j] = v;
                        cov[j * m + i] = v;
                    }
                }
            if (prefix_nis || joint_nis) {
                bos::joint_ldl_prefix(m, A, bos::kJointLd, y, pre);
                for (int32_t i = 0; i < m && prefix_nis; ++i) prefix_nis[p0 + i] = pre[i];
                if (joint_nis) joint_nis[h] = m > 0 ? pre[m - 1] : 0.0;
            }
        }
        s_done += B.s_count;
    }
    return BOS_OK;
}

namespace {
// One frame's result as the call returns it
void jcbb_store(const bos::JcbbFrame& f, const bos::JcbbResult& r, int32_t* assignment, int32_t* n_paired, double* joint_nis,
                double* prefix_nis, int32_t* complete, int64_t* nodes) {
    for (int b = 0; b < f.m; ++b) {
        if (assignment)
            assignment[b] = r.choice[b] == bos::kJcbbNothing ? -1 : f.cand_landmark[f.cand_start[b] - f.cand_start[0] + r.choice[b]];
        if (prefix_nis) prefix_nis[b] = r.prefix[b];
    }
    if (n_paired) *n_paired = r.n;
    if (joint_nis) *joint_nis = r.nis;
    if (complete) *complete = r.complete ? 1 : 0;
    if (nodes) *nodes = r.nodes;
}
}  // namespace

// Test hook: the serial search of csrc/host/jcbb.hpp on a given S_all and e_all.
int bos_jcbb_search_host(int32_t m, const int32_t* cand_start, const int32_t* cand_landmark, const double* S_all, const double* e_all,
                         const double* gate, int64_t max_nodes, int32_t no_bound, int32_t* assignment, int32_t* n_paired,
                         double* joint_nis, double* prefix_nis, int32_t* complete, int64_t* nodes) {
    if (m < 0 || m > bos::kJcbbMaxBearings) return hfail(BOS_ERR_INVALID, "bos_jcbb: a frame of more than BOS_JCBB_MAX_BEARINGS bearings");
    if (const char* bad = bos::jcbb_bad_lists(INT32_MAX, m, cand_start, cand_landmark, gate, max_nodes))
        return hfail(BOS_ERR_INVALID, std::string("bos_jcbb: ") + bad);
    const int32_t P = cand_start[m];
    if (P > bos::kJointMaxM) return hfail(BOS_ERR_INVALID, "bos_jcbb: a frame of more than BOS_JOINT_MAX_M pairings");
    if (P > 0 && (!S_all || !e_all)) return hfail(BOS_ERR_INVALID, "bad argument");
    bos::JcbbFrame f;
    f.m = m; f.cand_start = cand_start; f.cand_landmark = cand_landmark; f.S = S_all; f.e = e_all; f.ld = P; f.gate = gate;
    f.budget = bos::jcbb_budget(max_nodes); f.bound = !no_bound;
    bos::JcbbResult r;
    bos::jcbb_search(f, r);
    jcbb_store(f, r, assignment, n_paired, joint_nis, prefix_nis, complete, nodes);
    return BOS_OK;
}

// Test hook: bos_jcbb in its literal host form: the frames' all-pairings hypotheses through
// bos_plan_mf_joint_compatibility, then the serial search per frame.
int bos_plan_mf_jcbb(const bos_problem* pb, const bos_options* options, const double* vals, int32_t n_frames, const int32_t* frame_start,
                     const int32_t* pose, const double* z, const double* omega, const int32_t* cand_start, const int32_t* cand_landmark,
                     const double* gate, int64_t max_nodes, int64_t max_batch, int32_t* assignment, int32_t* n_paired, double* joint_nis,
                     double* prefix_nis, int32_t* complete, double* innovation, double* innovation_cov, int64_t* nodes) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0) || max_batch < 0)
        return hfail(BOS_ERR_INVALID, "bad argument");
    if (const char* bad = bos::jcbb_bad_argument(pb->num_poses, pb->num_landmarks, n_frames, frame_start, pose, z, omega, cand_start,
                                                 cand_landmark, gate, max_nodes))
        return hfail(BOS_ERR_INVALID, std::string("bos_jcbb: ") + bad);
    if (n_frames == 0) return BOS_OK;
    bos::JcbbPairings A;
    bos::jcbb_pairings(n_frames, frame_start, pose, z, omega, cand_start, A);
    const int32_t np = A.hyp_start[n_frames];
    int64_t s_count = 0;
    for (int32_t f = 0; f < n_frames; ++f) s_count += (int64_t)(A.hyp_start[f + 1] - A.hyp_start[f]) * (A.hyp_start[f + 1] - A.hyp_start[f]);
    std::vector<double> e((size_t)np + 1), S((size_t)s_count + 1);
    const int rc = bos_plan_mf_joint_compatibility(pb, options, vals, n_frames, A.hyp_start.data(), A.pose.data(), cand_landmark, A.z.data(),
                                                   A.omega.data(), max_batch, nullptr, nullptr, e.data(), S.data());
    if (rc) return rc;
    int64_t s_off = 0;
    for (int32_t fr = 0; fr < n_frames; ++fr) {
        const int32_t b0 = frame_start[fr], p0 = A.hyp_start[fr], P = A.hyp_start[fr + 1] - p0;
        bos::JcbbFrame f;
        f.m = frame_start[fr + 1] - b0; f.cand_start = cand_start + b0; f.cand_landmark = cand_landmark + p0;
        f.S = S.data() + s_off; f.e = e.data() + p0; f.ld = P; f.gate = gate; f.budget = bos::jcbb_budget(max_nodes);
        bos::JcbbResult r;
        bos::jcbb_search(f, r);
        jcbb_store(f, r, assignment ? assignment + b0 : nullptr, n_paired ? n_paired + fr : nullptr, joint_nis ? joint_nis + fr : nullptr,
                   prefix_nis ? prefix_nis + b0 : nullptr, complete ? complete + fr : nullptr, nodes ? nodes + fr : nullptr);
        s_off += (int64_t)P * P;
    }
    if (innovation) std::copy(e.begin(), e.begin() + np, innovation);
    if (innovation_cov) std::copy(S.begin(), S.begin() + s_count, innovation_cov);
    return BOS_OK;
}

int32_t bos_associate_tile(void) { return bos::kAssocTile; }

namespace {
// What the two matching hooks share behind a query's score row: the targets inside the gate sorted by
// (score, stix), the k first listed with their details (detail(target, out), dd doubles; cov likewise), the
// rest of the slots padded
struct MatchLists {
    int32_t* cand_ix;
    double *cand_score, *cand_detail, *cand_cov;
    int32_t* n_inside;
    double* all;
    int dd, dc;
};
typedef std::function<void(int32_t, double*)> MatchFill;
void match_list_row(const MatchLists& o, int32_t q, size_t N, size_t K, double gate, const std::vector<double>& row, const MatchFill& detail,
                    const MatchFill& cov) {
    std::vector<int32_t> inside;
    for (size_t t = 0; t < N; ++t)
        if (bos::assoc_inside(row[t], gate)) inside.push_back((int32_t)t);
    std::sort(inside.begin(), inside.end(), [&](int32_t x, int32_t y) { return bos::assoc_less(row[x], x, row[y], y); });
    for (size_t j = 0; j < K; ++j) {
        const bool listed = j < inside.size();
        const int32_t t = listed ? inside[j] : -1;
        const size_t at = (size_t)q * K + j;
        if (o.cand_ix) o.cand_ix[at] = t;
        if (o.cand_score) o.cand_score[at] = listed ? row[t] : HUGE_VAL;
        if (o.cand_detail) {
            std::fill_n(o.cand_detail + at * o.dd, o.dd, 0.0);
            if (listed) detail(t, o.cand_detail + at * o.dd);
        }
        if (o.cand_cov) {
            std::fill_n(o.cand_cov + at * o.dc, o.dc, 0.0);
            if (listed) cov(t, o.cand_cov + at * o.dc);
        }
    }
    if (o.n_inside) o.n_inside[q] = (int32_t)inside.size();
    if (o.all) std::copy(row.begin(), row.begin() + N, o.all + (size_t)q * N);
}
}  // namespace

// Test hook: bos_match_landmarks in its literal host form (csrc/host/match.hpp): per query the node hook's
// column for projected_landmark, d and d2 by the shared code, then a plain sort.
int bos_plan_mf_match_landmarks(const bos_problem* pb, const bos_options* options, const double* vals, int32_t n_queries,
                                const int32_t* landmark, double gate, int32_t k, int32_t* cand_landmark, double* cand_d2,
                                double* cand_diff, double* cand_cov, int32_t* n_inside, double* d2_all) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0)) return hfail(BOS_ERR_INVALID, "bad argument");
    if (const char* bad = bos::match_landmarks_bad_argument(pb->num_landmarks, n_queries, landmark, gate, k))
        return hfail(BOS_ERR_INVALID, std::string("bos_match_landmarks: ") + bad);
    if (n_queries == 0) return BOS_OK;
    NodeColumnHost H;
    const int rc = H.setup(pb, options, vals, true);
    if (rc) return rc;
    const size_t NL = (size_t)H.P.NL;
    const MatchLists o = {cand_landmark, cand_d2, cand_diff, cand_cov, n_inside, d2_all, 2, 4};
    std::vector<double> C(4 * NL + 1), row(NL + 1);
    int last = -1;
    for (int32_t q = 0; q < n_queries; ++q) {
        const int a = landmark[q];
        if (a != last) {   // the column depends on the landmark alone
            bos::NodeCovOut co;
            co.projected_landmark = C.data();
            H.column(H.P.NP + a, co);
            last = a;
        }
        const double ax = H.lm[2 * a], ay = H.lm[2 * a + 1];
        auto diff = [&](int32_t l, double* d) { bos::match_landmark_diff(ax, ay, H.lm[2 * l], H.lm[2 * l + 1], d); };
        for (size_t l = 0; l < NL; ++l) {
            double d[2];
            diff((int32_t)l, d);
            row[l] = (int)l == a ? bos::match_nan() : bos::match_landmark_d2(d, C[4 * l], C[4 * l + 2], C[4 * l + 3]);
        }
        match_list_row(o, q, NL, (size_t)k, gate, row, diff, [&](int32_t l, double* c) { std::copy_n(C.begin() + 4 * (size_t)l, 4, c); });
    }
    return BOS_OK;
}

// Test hook: bos_match_poses in its literal host form: per distinct pose the node hook's column for
// projected_pose, per measurement e, S and nis by the shared code, then a plain sort.
int bos_plan_mf_match_poses(const bos_problem* pb, const bos_options* options, const double* vals, int32_t n_meas, const int32_t* pose,
                            const double* z, const double* omega, double gate, int32_t k, int32_t* cand_pose, double* cand_nis,
                            double* cand_innovation, double* cand_cov, int32_t* n_inside, double* nis_all) {
    if (!pb || !vals || !pb->pose_xyt || (!pb->landmark_xy && pb->num_landmarks > 0)) return hfail(BOS_ERR_INVALID, "bad argument");
    std::vector<double> R(9 * (size_t)std::max(n_meas, 0));
    if (const char* bad = bos::match_poses_bad_argument(pb->num_poses, n_meas, pose, z, omega, gate, k, R.data()))
        return hfail(BOS_ERR_INVALID, std::string("bos_match_poses: ") + bad);
    if (n_meas == 0) return BOS_OK;
    NodeColumnHost H;
    const int rc = H.setup(pb, options, vals, true);
    if (rc) return rc;
    const size_t NP = (size_t)H.P.NP;
    const MatchLists o = {cand_pose, cand_nis, cand_innovation, cand_cov, n_inside, nis_all, 3, 9};
    std::vector<double> P(9 * NP + 1), row(NP + 1);
    int last = -1;
    for (int32_t q = 0; q < n_meas; ++q) {
        const int a = pose[q];
        if (a != last) {   // the column depends on the pose alone
            bos::NodeCovOut co;
            co.projected_pose = P.data();
            H.column(a, co);
            last = a;
        }
        const bos::MatchFrame f = bos::match_frame(H.pose.data(), a);
        const double* Rq = R.data() + 9 * (size_t)q;
        const double Rl[6] = {Rq[0], Rq[3], Rq[4], Rq[6], Rq[7], Rq[8]};
        auto error = [&](int32_t u, double* e) { bos::match_pose_error(f, H.pose[3 * u], H.pose[3 * u + 1], H.pose[3 * u + 2], z + 3 * (size_t)q, e); };
        for (size_t u = 0; u < NP; ++u) {
            double e[3], S[6];
            error((int32_t)u, e);
            bos::match_pose_S(P.data() + 9 * u, Rl, S);
            row[u] = bos::match_pose_nis(e, S);
        }
        match_list_row(o, q, NP, (size_t)k, gate, row, error, [&](int32_t u, double* full) {
            double S[6];
            bos::match_pose_S(P.data() + 9 * (size_t)u, Rl, S);
            bos::match_mirror(S, full);
        });
    }
    return BOS_OK;
}

int bos_match_information_inverse(const double omega[9], double R[9]) {
    if (!omega || !R) return hfail(BOS_ERR_INVALID, "null argument");
    if (!bos::match_information_inverse(omega, R))
        return hfail(BOS_ERR_INVALID, "bos_match_information_inverse: omega is not finite, symmetric and positive definite");
    return BOS_OK;
}

int bos_plan_pair_paths(const bos_problem* pb, const bos_options* options, int64_t n_pairs, const int32_t* node_a,
                        const int32_t* node_b, int32_t* out) {
    if (!pb || n_pairs < 0 || (n_pairs > 0 && (!node_a || !node_b || !out))) return hfail(BOS_ERR_INVALID, "bad argument");
    if (n_pairs == 0) return BOS_OK;
    if (!bos::pair_ids_valid(pb->num_poses, pb->num_landmarks, n_pairs, node_a, node_b))
        return hfail(BOS_ERR_INVALID, "bos_pair_covariances: a node id outside [0, NP + NL), or a mixed pair not written (pose, landmark)");
    bos::ProblemIndex pi;
    bos::Plan P;
    bos::PairPaths pp;
    const int rc = pair_plan(pb, options, pi, P, pp);
    if (rc) return rc;
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int a = node_a[q], b = node_b[q], sa = a == P.fixed ? -1 : pp.node_sn[a], sb = b == P.fixed ? -1 : pp.node_sn[b];
        int32_t* o = out + 5 * q;
        o[0] = sa; o[1] = sb;
        o[2] = sa < 0 || sb < 0 ? -2 : bos::pair_lca(pp, sa, sb);
        o[3] = o[2] >= 0 ? (int32_t)pp.path_dofs[o[2]] : 0;
        o[4] = (int32_t)std::max(sa >= 0 ? pp.path_dofs[sa] : 0, sb >= 0 ? pp.path_dofs[sb] : 0);
    }
    return BOS_OK;
}

// The sharded solve (plan.hpp Shard) simulated on the host for all `world` ranks, exchanges
// included (the all-gathers become concatenations of the per-rank send buffers). Every rank builds
// its own plan, holds only the block values its J+H computes (vals scattered through its
// csr_src), factors and forward-solves its subtrees, packs its roots' U / u (exchange1_segments),
// unpacks the others', factors and solves the top, solves its subtrees backward and packs its
// boundary solution (exchange 2). Checks: the ranks agree on the top bit for bit; the merged x
// (each node from its owner) equals the one-rank run bit for bit; every observation's chi^2 is
// counted by exactly one rank; every node a rank's J+H lanes read is in its box-plus set.
int bos_plan_shard_selftest(const bos_problem* pb, const bos_options* options, int32_t world, const double* vals,
                            const double* rhs, double* x) {
    if (!pb || !vals || !rhs || !x || world < 1) return hfail(BOS_ERR_INVALID, "bad argument");
    bos::ProblemIndex pi;
    bos_options opt;
    int fmode = 0;
    const int arc = plan_args(pb, options, pi, fmode, opt);
    if (arc) return arc;
    if (opt.solver != BOS_SOLVER_SUPERNODAL && opt.solver != BOS_SOLVER_SCHUR)
        return hfail(BOS_ERR_INVALID, "selftest needs a multifrontal solver");
    if (opt.partition != BOS_PARTITION_SUBTREE) return hfail(BOS_ERR_INVALID, "selftest of the subtree partition");
    const int NP = pi.NP, NL = pi.NL;
    std::vector<bos::Plan> plans(world);
    for (int r = 0; r < world; ++r) {
        std::string err;
        const int rc = bos::build_plan(pi, r, world, fmode, plans[r], err);
        if (rc) return hfail(rc, err);
    }
    bos::Plan one;
    {
        std::string err;
        const int rc = bos::build_plan(pi, 0, 1, fmode, one, err);
        if (rc) return hfail(rc, err);
    }
    const int64_t n = one.n;
    // the one-rank run: the values each rank's J+H computes are the one-rank values of those entries
    bos::HostMf ref(one, vals, rhs);
    auto all = [](int) { return true; };
    ref.factor(all);
    ref.forward(all);
    ref.backward(all);
    std::vector<bos::HostMf> M;
    M.reserve(world);
    for (int r = 0; r < world; ++r) {
        const bos::Plan& P = plans[r];
        if (P.n != n || P.mf.nsuper != one.mf.nsuper || P.mf.L_size != one.mf.L_size)
            return hfail(BOS_ERR_INVALID, "ranks disagree on the tree");
        M.emplace_back(P, vals, rhs);
    }
    // phase 1: own subtrees
    std::vector<std::vector<double>> send1(world);
    for (int r = 0; r < world; ++r) {
        const bos::Shard& S = plans[r].shard;
        auto own = [&](int s) { return S.sn_owner[s] == r; };
        M[r].factor(own);
        M[r].forward(own);
        std::vector<bos::ExchangeSeg> pk, un;
        bos::exchange1_segments(plans[r], pk, un);
        send1[r].assign(S.ex1_count, 0.0);
        for (const bos::ExchangeSeg& g : pk) {
            const std::vector<double>& src = g.src_kind == 0 ? M[r].U : M[r].u;
            if (g.dst_kind != 2 || g.dst + g.len > S.ex1_count) return hfail(BOS_ERR_INVALID, "exchange 1 pack out of range");
            std::copy(src.begin() + g.src, src.begin() + g.src + g.len, send1[r].begin() + g.dst);
        }
    }
    for (int r = 0; r < world; ++r) {   // the all-gather + unpack
        const bos::Shard& S = plans[r].shard;
        std::vector<double> recv;
        for (int q = 0; q < world; ++q) {
            if (plans[q].shard.ex1_count != S.ex1_count) return hfail(BOS_ERR_INVALID, "ranks disagree on exchange 1");
            recv.insert(recv.end(), send1[q].begin(), send1[q].end());
        }
        std::vector<bos::ExchangeSeg> pk, un;
        bos::exchange1_segments(plans[r], pk, un);
        for (const bos::ExchangeSeg& g : un) {
            std::vector<double>& dst = g.dst_kind == 0 ? M[r].U : M[r].u;
            if (g.src_kind != 3 || g.src + g.len > (int64_t)recv.size()) return hfail(BOS_ERR_INVALID, "exchange 1 unpack out of range");
            std::copy(recv.begin() + g.src, recv.begin() + g.src + g.len, dst.begin() + g.dst);
        }
        auto topf = [&](int s) { return S.sn_owner[s] == -1; };
        auto own = [&](int s) { return S.sn_owner[s] == r; };
        M[r].factor(topf);
        M[r].forward(topf);
        M[r].backward(topf);
        M[r].backward(own);
    }
    // exchange 2: boundary solution from its owner
    for (int r = 0; r < world; ++r) {
        const bos::Shard& S = plans[r].shard;
        for (int q = 0; q < world; ++q) {
            if (q == r) continue;
            for (int i = S.bnd_ptr[q]; i < S.bnd_ptr[q + 1]; ++i) M[r].x[S.bnd_dof[i]] = M[q].x[S.bnd_dof[i]];
        }
    }
    // checks
    const bos::Shard& S0 = plans[0].shard;
    std::vector<int> owner_of_dof(n, -3);
    for (int u = 0; u < NP + NL; ++u) {
        if (S0.node_owner[u] == -2) continue;
        const int sz = u < NP ? 3 : 2;
        for (int d = 0; d < sz; ++d) owner_of_dof[one.node_dof[u] + d] = S0.node_owner[u];
    }
    for (int64_t i = 0; i < n; ++i) {
        const int o = owner_of_dof[i];
        if (o == -3) return hfail(BOS_ERR_INVALID, "dof without an owner");
        const double v = M[o < 0 ? 0 : o].x[i];
        if (o < 0)
            for (int r = 1; r < world; ++r)
                if (M[r].x[i] != v) return hfail(BOS_ERR_INVALID, "ranks disagree on a top dof");
        if (v != ref.x[i]) return hfail(BOS_ERR_INVALID, "sharded solution differs from the one-rank solution");
        x[i] = v;
    }
    std::vector<int> chi(pi.Mb + pi.Mo, 0);
    for (int r = 0; r < world; ++r) {
        const bos::Plan& P = plans[r];
        const bos::Shard& S = P.shard;
        if (S.node_owner != S0.node_owner) return hfail(BOS_ERR_INVALID, "ranks disagree on node ownership");
        std::vector<char> fresh(NP + NL, 0);
        for (int u : S.upd_nodes) fresh[u] = 1;
        fresh[pi.fixed] = 1;
        std::vector<char> lane(NP + NL, 0);
        for (size_t i = 0; i < S.lane_poses.size(); ++i) {
            const int p = S.lane_poses[i];
            if (p < 0) continue;
            lane[p] = 1;
            if ((int)i < S.own_pose_lanes || r == 0) {
                for (int k = 0; k < pi.Mb; ++k) if (pi.b_pose[k] == p) ++chi[k];
                for (int k = 0; k < pi.Mo; ++k) if (pi.o_src[k] == p && pi.o_src[k] != pi.o_dst[k]) ++chi[pi.Mb + k];
            }
        }
        for (int l : S.lane_lms) lane[NP + l] = 1;
        for (int k = 0; k < pi.Mb; ++k) {
            const int p = pi.b_pose[k], l = NP + pi.b_lm[k];
            if ((lane[p] || lane[l]) && !(fresh[p] && fresh[l])) return hfail(BOS_ERR_INVALID, "a J+H lane reads a stale node");
        }
        for (int k = 0; k < pi.Mo; ++k) {
            const int a = pi.o_src[k], b = pi.o_dst[k];
            if ((lane[a] || lane[b]) && !(fresh[a] && fresh[b])) return hfail(BOS_ERR_INVALID, "a J+H lane reads a stale node");
        }
    }
    for (int k = 0; k < pi.Mb + pi.Mo; ++k) {
        const bool loop = k >= pi.Mb && pi.o_src[k - pi.Mb] == pi.o_dst[k - pi.Mb];
        if (chi[k] != (loop ? 0 : 1)) return hfail(BOS_ERR_INVALID, "chi^2 of an observation not counted exactly once");
    }
    return BOS_OK;
}

}  // extern "C"
