// bos_create / bos_destroy (solver_handle.hpp): option checks, the static plan, every upload and
// allocation of the handle. bos_create holds the handle in an owning pointer until its last line, so
// every failing step below frees what was made so far by returning.
#include <algorithm>
#include <cstring>
#include <memory>

#include "solver_handle.hpp"

using namespace bos::capi;

namespace {

int no_mem(const char* what) { return fail(BOS_ERR_DEVICE, std::string(what) + ": device allocation or upload failed"); }

int check_arguments(const bos_problem* pb, const bos_options& opt, int& ndev) {
    if (opt.precision != BOS_FP64 && opt.precision != BOS_FP32) return fail(BOS_ERR_INVALID, "precision must be 32 or 64");
    if (opt.solver != BOS_SOLVER_SUPERNODAL && opt.solver != BOS_SOLVER_DENSE_CHOL &&
        opt.solver != BOS_SOLVER_ROCSOLVER_RF && opt.solver != BOS_SOLVER_SCHUR)
        return fail(BOS_ERR_INVALID, "unknown solver");
    if (opt.partition != BOS_PARTITION_SUBTREE && opt.partition != BOS_PARTITION_OBSERVATIONS)
        return fail(BOS_ERR_INVALID, "unknown partition");
    if (pb->num_poses <= 0 || pb->num_landmarks < 0 || pb->num_bearings < 0 || pb->num_odometry < 0)
        return fail(BOS_ERR_INVALID, "bad problem sizes");
    if (!pb->pose_xyt ||
        (pb->num_bearings && (!pb->bearing_pose || !pb->bearing_landmark || !pb->bearing_z)) ||
        (pb->num_odometry && (!pb->odom_src || !pb->odom_dst || !pb->odom_z || !pb->odom_omega)))
        return fail(BOS_ERR_INVALID, "null problem array");
    // host waits spin instead of sleeping (bos_step is synchronous: its wait is on the critical path
    // of every iteration); only possible before the process's first device use, ignored afterwards
    (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
    (void)hipGetLastError();
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(BOS_ERR_DEVICE, "no HIP device visible (the HIP path has no CPU fallback)");
    if (opt.world_size < 1 || opt.rank < 0 || opt.rank >= opt.world_size) return fail(BOS_ERR_INVALID, "bad rank / world_size");
    return BOS_OK;
}

// the options and sizes into the handle, the device, the static plan (host) and what follows from it
int build_plan(bos_solver* s, const bos_problem* pb, const bos_options& opt, int ndev) {
    s->precision = opt.precision;
    s->tsize = opt.precision == BOS_FP32 ? 4 : 8;
    s->solver_kind = opt.solver;
    s->rank = opt.rank;
    s->world = opt.world_size;
    s->kt = opt.kernel_threshold;
    s->damping = opt.damping;
    s->NP = pb->num_poses; s->NL = pb->num_landmarks; s->Mb = pb->num_bearings; s->Mo = pb->num_odometry;
    if (opt.device >= 0) {
        if (opt.device >= ndev) return fail(BOS_ERR_DEVICE, "device ordinal out of range");
        if (hipSetDevice(opt.device) != hipSuccess) return fail(BOS_ERR_DEVICE, "hipSetDevice failed");
        s->device = opt.device;
    } else {
        if (hipGetDevice(&s->device) != hipSuccess) return fail(BOS_ERR_DEVICE, "hipGetDevice failed");
    }
    bos::ProblemIndex pi;
    pi.NP = s->NP; pi.NL = s->NL; pi.Mb = s->Mb; pi.Mo = s->Mo; pi.fixed = pb->fixed_pose;
    pi.b_pose = pb->bearing_pose; pi.b_lm = pb->bearing_landmark; pi.o_src = pb->odom_src; pi.o_dst = pb->odom_dst;
    pi.b_omega = pb->bearing_omega; pi.o_omega = pb->odom_omega;
    pi.lpp = opt.lanes_per_pose;
    pi.schur_leaf = opt.schur_leaf;
    // multi-rank (world > 1, or a communicator given with world 1: a one-GPU test of the path)
    const bool multi = s->world > 1 || opt.nccl_unique_id;
    s->partition = opt.partition;
    s->obs = multi && opt.partition == BOS_PARTITION_OBSERVATIONS;
    s->sharded = multi && opt.partition == BOS_PARTITION_SUBTREE;
    s->external = multi && !opt.nccl_unique_id;
    std::string err;
    const int fmode = s->solver_kind == BOS_SOLVER_SUPERNODAL    ? bos::kFactorMultifrontal
                      : s->solver_kind == BOS_SOLVER_SCHUR        ? bos::kFactorSchur
                      : s->solver_kind == BOS_SOLVER_ROCSOLVER_RF ? bos::kFactorScalar
                                                                  : bos::kFactorNone;
    // the observations partition runs a range of the one-GPU plan's lanes
    const int rc = s->obs ? bos::build_plan(pi, 0, 1, fmode, s->plan, err) : bos::build_plan(pi, s->rank, s->world, fmode, s->plan, err);
    if (rc) return fail(rc, "plan: " + err);
    const bos::Plan& P = s->plan;
    if (s->solver_kind == BOS_SOLVER_DENSE_CHOL && P.n > 40000) return fail(BOS_ERR_UNSUPPORTED, "dense solver limited to n <= 40000");
    s->has_dups = P.blk.has_dups;
    s->has_w = false;
    if (pb->bearing_omega)
        for (int k = 0; k < s->Mb; ++k)
            if (pb->bearing_omega[k] != 1.0) { s->has_w = true; break; }
    s->pl_factored = s->precision == BOS_FP32 && uses_mf(s) && !s->has_w && !s->has_dups;
    // permuted dof -> reference dof
    s->ref_dof.assign(P.n + 3, 0);
    for (int u = 0; u < s->NP + s->NL; ++u) {
        const int sz = u < s->NP ? 3 : 2;
        const int ref0 = u < s->NP ? 3 * u : 3 * s->NP + 2 * (u - s->NP);
        for (int d = 0; d < sz; ++d) s->ref_dof[P.node_dof[u] + d] = ref0 + d;
    }
    return BOS_OK;
}

int create_streams_and_libraries(bos_solver* s, const bos_options& opt) {
    if (opt.stream) {
        s->stream = (hipStream_t)opt.stream;
    } else {
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) return fail(BOS_ERR_DEVICE, "hipStreamCreate failed");
        s->own_stream = true;
    }
    for (hipEvent_t& e : s->ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(BOS_ERR_DEVICE, "hipEventCreate failed");
    if (rocblas_create_handle(&s->rb) != rocblas_status_success) return fail(BOS_ERR_SOLVER, "rocblas_create_handle");
    if (rocblas_set_stream(s->rb, s->stream) != rocblas_status_success) return fail(BOS_ERR_SOLVER, "rocblas_set_stream");
    if (s->solver_kind == BOS_SOLVER_ROCSOLVER_RF) {
        const rocblas_status st = rocsolver_create_rfinfo(&s->rf, s->rb);
        if (st != rocblas_status_success) {
            size_t fr = 0, tot = 0;
            (void)hipMemGetInfo(&fr, &tot);
            return fail(BOS_ERR_SOLVER, "rocsolver_create_rfinfo: status " + std::to_string((int)st) + ", device memory free " +
                                            std::to_string(fr >> 20) + " MiB");
        }
        if (rocsolver_set_rfinfo_mode(s->rf, rocsolver_rfinfo_mode_cholesky) != rocblas_status_success)
            return fail(BOS_ERR_SOLVER, "set_rfinfo_mode");
    }
    if ((s->sharded || s->obs) && !uses_mf(s)) return fail(BOS_ERR_UNSUPPORTED, "sharding needs a multifrontal solver");
    if (opt.nccl_unique_id) {
        ncclUniqueId id;
        std::memcpy(&id, opt.nccl_unique_id, sizeof(id));
        ncclResult_t r = ncclCommInitRank(&s->comm, s->world, id, s->rank);
        if (r != ncclSuccess) return fail(BOS_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
        int count = 0;   // the ranks the communicator actually holds
        r = ncclCommCount(s->comm, &count);
        if (r != ncclSuccess) return fail(BOS_ERR_COMM, std::string("ncclCommCount: ") + ncclGetErrorString(r));
        if (count != s->world)
            return fail(BOS_ERR_COMM, "communicator holds " + std::to_string(count) + " ranks, world_size " + std::to_string(s->world));
    }
    return BOS_OK;
}

// Exchange tables and buffers of the sharded step (host/shard.cpp): exchange 1 by segments of the
// update-matrix / u-vector arrays, exchange 2 by dof index lists.
int setup_shard(bos_solver* s) {
    const bos::Shard& S = s->plan.shard;
    const int W = s->world;
    bos::dev::DeviceMem& mem = s->mem;
    s->ex1_count = S.ex1_count;
    s->ex2_count = S.ex2_count;
    std::vector<bos::ExchangeSeg> hp, hu;
    bos::exchange1_segments(s->plan, hp, hu);
    auto conv = [](const std::vector<bos::ExchangeSeg>& v, int64_t& maxlen) {
        std::vector<bos::dev::ExSeg> o(v.size());
        for (size_t i = 0; i < v.size(); ++i) {
            o[i] = {v[i].src, v[i].dst, v[i].len, v[i].src_kind, v[i].dst_kind};
            maxlen = std::max(maxlen, v[i].len);
        }
        return o;
    };
    const std::vector<bos::dev::ExSeg> pack = conv(hp, s->maxlen1p);
    std::vector<bos::dev::ExSeg> unpack = conv(hu, s->maxlen1u);
    for (int q = 0; q < W; ++q)   // rank q's header -> hdr1[q * kExHeader] (kind 4), after the wait
        unpack.push_back({(int64_t)q * S.ex1_count, (int64_t)q * bos::kExHeader, bos::kExHeader, 3, 4});
    s->maxlen1u = std::max<int64_t>(s->maxlen1u, bos::kExHeader);
    s->n1p = (int)pack.size();
    s->n1u = (int)unpack.size();
    std::vector<int32_t> bnd(S.bnd_dof.begin() + S.bnd_ptr[s->rank], S.bnd_dof.begin() + S.bnd_ptr[s->rank + 1]);
    std::vector<int32_t> usrc, udst;
    for (int q = 0; q < W; ++q) {
        if (q == s->rank) continue;
        for (int i = S.bnd_ptr[q]; i < S.bnd_ptr[q + 1]; ++i) {
            usrc.push_back((int32_t)((int64_t)q * S.ex2_count + bos::kExHeader + (i - S.bnd_ptr[q])));
            udst.push_back(S.bnd_dof[i]);
        }
    }
    s->n_bnd = (int)bnd.size();
    s->n_bnd_remote = (int)usrc.size();
    s->n_upd = (int)S.upd_nodes.size();
    s->n_upd_local = S.n_upd_local;
    if (!(mem.upload(&s->ex1_pack, pack) && mem.upload(&s->ex1_unpack, unpack) && mem.upload(&s->ex2_bnd, bnd) &&
          mem.upload(&s->ex2_usrc, usrc) && mem.upload(&s->ex2_udst, udst) && mem.upload(&s->upd_nodes, S.upd_nodes) &&
          mem.alloc(&s->ex1_send, (size_t)s->ex1_count, true) && mem.alloc(&s->ex2_send, (size_t)s->ex2_count, true) &&
          mem.alloc(&s->hdr1, (size_t)W * bos::kExHeader, true) &&
          mem.alloc(&s->abs_part, (size_t)std::max(1, (S.n_upd_local + 255) / 256), false)))
        return no_mem("exchange buffers");
    // the mailbox: [exchange 1: W x ex1_count][exchange 2: W x ex2_count][flags: 2 x W x 64 B]
    auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    s->mb_ex1 = 0;
    s->mb_ex2 = al((int64_t)W * s->ex1_count * (int64_t)sizeof(double));
    s->mb_flag1 = s->mb_ex2 + al((int64_t)W * s->ex2_count * (int64_t)sizeof(double));
    s->mb_flag2 = s->mb_flag1 + 64 * (int64_t)W;
    const size_t bytes = (size_t)(s->mb_flag2 + 64 * (int64_t)W);
    if (hipExtMallocWithFlags((void**)&s->mailbox, bytes, hipDeviceMallocUncached) == hipSuccess) {
        mem.adopt(s->mailbox, bytes);
        s->mailbox_uncached = true;
        HIP_TRY(hipMemset(s->mailbox, 0, bytes));
    } else {
        (void)hipGetLastError();
        if (!mem.alloc(&s->mailbox, bytes, true)) return no_mem("exchange mailbox");
    }
    s->ex1_recv = reinterpret_cast<double*>(s->mailbox + s->mb_ex1);
    s->ex2_recv = reinterpret_cast<double*>(s->mailbox + s->mb_ex2);
    return BOS_OK;
}

// The master state (angles normalised). landmark_xy == NULL: the landmarks are triangulated on the
// device at the end of bos_create (the reference's triangulate_landmarks before the Solver ctor,
// bearing_only_slam.cpp / slam/triangulation.cpp)
int upload_state(bos_solver* s, const bos_problem* pb) {
    std::vector<double> pose(pb->pose_xyt, pb->pose_xyt + 3 * (size_t)s->NP);
    for (int i = 0; i < s->NP; ++i) pose[3 * i + 2] = bos::normalized_angle<double>(bos::smallest_angle<double>(pose[3 * i + 2]));
    std::vector<double> lm(2 * (size_t)s->NL, 0.0);
    if (pb->landmark_xy) lm.assign(pb->landmark_xy, pb->landmark_xy + 2 * (size_t)s->NL);
    if (!(s->mem.upload(&s->d_pose, pose) && s->mem.upload(&s->d_lm, lm))) return no_mem("state");
    return BOS_OK;
}

// One field of the J+H arena in T
void add_T(const bos_solver* s, bos::dev::Arena& ar, void** p, const std::vector<double>& v) {
    if (s->precision == BOS_FP32) ar.add(reinterpret_cast<float**>(p), std::vector<float>(v.begin(), v.end()));
    else ar.add(reinterpret_cast<double**>(p), v);
}

// The J+H's slot records, work lists and lane tables into the arena (padding slots: index 0, z 0)
void stage_jh_lists(bos_solver* s, const bos_problem* pb, bos::dev::Arena& ar) {
    const bos::Plan& P = s->plan;
    const bos::BlockLayout& B = P.blk;
    // The arrays carry kRecPad extra padding records so the kernel's two-ahead prefetch never leaves
    // them; a prefetched padding record is never evaluated.
    const std::vector<int32_t>& po = B.pose_lanes.obs;
    const std::vector<int32_t>& lo = B.lm_lanes.obs;
    const size_t pad = bos::dev::kRecPad;
    std::vector<double> pbz(po.size() + pad, 0.0), lbz(lo.size() + pad, 0.0), pbw, lbw;
    std::vector<int32_t> pbi(po.size() + pad, 0), lbi(lo.size() + pad, 0);
    for (size_t i = 0; i < po.size(); ++i)
        if (po[i] >= 0) { pbi[i] = pb->bearing_landmark[po[i]]; pbz[i] = pb->bearing_z[po[i]]; }
    for (size_t i = 0; i < lo.size(); ++i)
        if (lo[i] >= 0) { lbi[i] = pb->bearing_pose[lo[i]]; lbz[i] = pb->bearing_z[lo[i]]; }
    {   // runs of duplicate (pose, landmark) observations: every record but the run's last is flagged
        const bos::LaneLists& PLn = B.pose_lanes;
        for (size_t g = 0; g < PLn.cnt.size(); ++g)
            for (int j = 0; j + 1 < PLn.cnt[g]; ++j) {
                const int64_t sl = PLn.slot((int)g, j), sn = PLn.slot((int)g, j + 1);
                if (pbi[sl] == pbi[sn]) pbi[sl] |= bos::dev::kRunCont;
            }
    }
    // odometry entries, padded (entry 0 / other pose 0 / no block): the J+H reads a pose's first
    // two entries unconditionally, in bounds even for the last pose without entries
    std::vector<int32_t> po_oth(B.po_ent.size() + pad, 0), po_ent(B.po_ent), po_blk(B.po_blk);
    po_ent.resize(B.po_ent.size() + pad, 0);
    po_blk.resize(B.po_blk.size() + pad, -1);
    for (size_t x = 0; x < B.po_ent.size(); ++x) {
        const int32_t e = B.po_ent[x];
        po_oth[x] = (e & 1) ? pb->odom_src[e >> 1] : pb->odom_dst[e >> 1];
    }
    // chain poses flagged in their first lane's count; interleaved groups: each lane's count with
    // the group's round count (its first lane's) in bits 16-29 (kernels.hip pose_lanes)
    std::vector<int32_t> plc(B.pose_lanes.cnt);
    if (B.interleaved)
        for (size_t g = 0; g < plc.size(); ++g) plc[g] |= B.pose_lanes.cnt[g - g % B.lpp] << 16;
    if (!B.has_dups)
        for (size_t i = 0; i < B.lane_pose.size(); ++i)
            if (B.lane_pose[i] >= 0 && B.po_chain[B.lane_pose[i]]) plc[i * B.lpp] |= bos::dev::kOdoChain;
    ar.add(&s->pw_base, B.pose_lanes.w_base); ar.add(&s->pl_cnt, plc);
    ar.add(&s->pw_stride, B.pose_lanes.w_stride); ar.add(&s->lw_stride, B.lm_lanes.w_stride);
    ar.add(&s->lw_base, B.lm_lanes.w_base);
    {   // a landmark lane's header in one 8-byte record {landmark | count << 20, first pose of the
        // lane's consecutive run or -1} when they fit (one load instead of three; LinParams::ll_hdr)
        const size_t nl = B.lm_lane_lm.size();
        bool fits = nl < ((size_t)1 << 20);
        for (size_t g = 0; g < nl && fits; ++g)
            fits = B.lm_lane_lm[g] >= 0 && B.lm_lane_lm[g] < (1 << 20) && B.lm_lanes.cnt[g] >= 0 && B.lm_lanes.cnt[g] < (1 << 12);
        if (fits && nl > 0) {
            std::vector<int32_t> hdr(2 * nl);
            for (size_t g = 0; g < nl; ++g) {
                hdr[2 * g] = (int32_t)((uint32_t)B.lm_lane_lm[g] | ((uint32_t)B.lm_lanes.cnt[g] << 20));
                hdr[2 * g + 1] = B.lm_lane_run.empty() ? -1 : B.lm_lane_run[g];
            }
            ar.add(&s->ll_hdr, hdr);
        } else {
            ar.add(&s->ll_cnt, B.lm_lanes.cnt);
            ar.add(&s->ll_lm, B.lm_lane_lm); ar.add(&s->ll_run, B.lm_lane_run);
        }
    }
    ar.add(&s->po_ptr, B.po_ptr); ar.add(&s->po_ent, po_ent); ar.add(&s->po_oth, po_oth);
    ar.add(&s->po_blk, po_blk); ar.add(&s->pb_idx, pbi); add_T(s, ar, &s->pb_z, pbz);
    ar.add(&s->lb_idx, lbi); add_T(s, ar, &s->lb_z, lbz);
    if (s->has_w) {
        pbw.assign(po.size() + pad, 0.0); lbw.assign(lo.size() + pad, 0.0);
        for (size_t i = 0; i < po.size(); ++i) if (po[i] >= 0) pbw[i] = pb->bearing_omega[po[i]];
        for (size_t i = 0; i < lo.size(); ++i) if (lo[i] >= 0) lbw[i] = pb->bearing_omega[lo[i]];
        add_T(s, ar, &s->pb_w, pbw); add_T(s, ar, &s->lb_w, lbw);
    }
    static_assert(bos::kJhBlock == bos::dev::kBlock, "J+H block size");
    s->pose_blocks = (int)B.pose_blocks();
    // J+H blocks this rank runs: all of them, or (observations partition) its ranges
    if (s->obs) {
        int64_t pb1 = 0, lb1 = 0;
        bos::observation_lanes(P, s->rank, s->world, s->pose_b0, pb1, s->lm_b0, lb1, nullptr);
        s->n_pose_run = pb1 - s->pose_b0;
        s->n_lm_run = lb1 - s->lm_b0;
    } else {
        s->n_pose_run = s->pose_blocks;
        s->n_lm_run = B.lm_blocks();
    }
    // chi^2 partials: own lanes (a whole number of blocks when sharded), the top lanes on rank 0;
    // observations partition: every block (the others' partials stay 0)
    s->chi_parts = bos::dev::kJhSub *
                   (s->rank == 0 || s->obs ? s->pose_blocks : (int)((int64_t)P.shard.own_pose_lanes * B.lpp / bos::dev::kBlock));
    ar.add(&s->lane_pose, B.lane_pose);
    s->lane_identity = true;
    for (size_t i = 0; i < B.lane_pose.size() && s->lane_identity; ++i) s->lane_identity = B.lane_pose[i] == (int32_t)i;
}

// The odometry into the arena, its self-loops and fp64 originals onto the handle
void stage_odometry(bos_solver* s, const bos_problem* pb, bos::dev::Arena& ar) {
    for (int k = 0; k < s->Mo; ++k)
        if (pb->odom_src[k] == pb->odom_dst[k]) {
            const double* m = pb->odom_omega + 9 * (size_t)k;
            for (int v = 0; v < 3; ++v) s->loop_z.push_back(pb->odom_z[3 * (size_t)k + v]);
            for (double v : {m[0], m[1], m[2], m[4], m[5], m[8]}) s->loop_om.push_back(v);
        }
    std::vector<int32_t> os(pb->odom_src, pb->odom_src + s->Mo), od(pb->odom_dst, pb->odom_dst + s->Mo);
    // one zero edge of padding (the J+H's unconditional reads of entry 0 when there is none)
    std::vector<double> oz(pb->odom_z, pb->odom_z + 3 * (size_t)s->Mo), om(6 * (size_t)s->Mo + 6, 0.0);
    oz.resize(3 * (size_t)s->Mo + 3, 0.0);
    bool same = true;   // every edge's information equal (bit for bit): one row, om_stride 0
    for (int k = 0; k < s->Mo; ++k) {
        const double* m = pb->odom_omega + 9 * (size_t)k;
        const double u[6] = {m[0], m[1], m[2], m[4], m[5], m[8]};
        for (int q = 0; q < 6; ++q) {
            om[6 * (size_t)k + q] = u[q];
            same = same && std::memcmp(&om[6 * (size_t)k + q], &om[q], sizeof(double)) == 0;
        }
    }
    s->om_stride = 6;
    // the cost pass of bos_cost / bos_optimize reads them in fp64 whatever T is (uploaded at its first use)
    s->h_oz.assign(pb->odom_z, pb->odom_z + 3 * (size_t)s->Mo);
    s->h_oom.assign(om.begin(), om.begin() + 6 * (size_t)s->Mo);
    if (s->has_w) s->h_bw.assign(pb->bearing_omega, pb->bearing_omega + s->Mb);
    if (same && s->Mo > 0) {   // the J+H then reads 24 (fp32) / 48 bytes of information in all, not per edge
        om.resize(12);
        s->om_stride = 0;
    }
    ar.add(&s->o_src, os); ar.add(&s->o_dst, od); add_T(s, ar, &s->o_z, oz); add_T(s, ar, &s->o_om, om);
}

// the J+H's inputs: the state caches (filled by upload_cache, then by the box-plus) and the static
// work lists, records and odometry, in one allocation
int stage_jh_inputs(bos_solver* s, const bos_problem* pb) {
    bos::dev::Arena ar;
    add_T(s, ar, &s->d_pc, std::vector<double>(4 * (size_t)s->NP, 0.0));
    add_T(s, ar, &s->d_pth, std::vector<double>((size_t)s->NP, 0.0));
    add_T(s, ar, &s->d_lc, std::vector<double>(2 * (size_t)s->NL, 0.0));
    stage_jh_lists(s, pb, ar);
    stage_odometry(s, pb, ar);
    if (!ar.commit(s->mem)) return no_mem("J+H inputs");
    return BOS_OK;
}

int alloc_system(bos_solver* s) {
    const bos::Plan& P = s->plan;
    bos::dev::DeviceMem& mem = s->mem;
    const bool f32 = s->precision == BOS_FP32;
    auto zeros_T = [&](void** p, size_t count) {
        return f32 ? mem.alloc((float**)p, count, true) : mem.alloc((double**)p, count, true);
    };
    const int64_t nval = std::max<int64_t>(P.blk.size, 1), nb = 3 * (int64_t)s->NP + 2 * (int64_t)s->NL;
    bool ok = mem.upload(&s->node_dof, P.node_dof);
    if (s->obs) {
        // [block array (even length) | b] in one buffer, all-reduced in one call into d_sys; the
        // values outside this rank's lanes stay 0
        const int64_t nv2 = (nval + 1) & ~(int64_t)1;
        s->vb_count = nv2 + nb;
        s->ex1_count = bos::kExHeader + (s->external ? s->vb_count : 0);
        ok = ok && zeros_T(&s->d_val, s->vb_count) && zeros_T(&s->d_sys, s->vb_count) &&
             mem.alloc(&s->ex1_send, (size_t)s->ex1_count, true) && mem.alloc(&s->ex1_recv, (size_t)s->ex1_count, true);
        if (!ok) return no_mem("system");
        s->d_b = (char*)s->d_val + nv2 * s->tsize;
        s->sys_val = s->d_sys;
        s->sys_b = (char*)s->d_sys + nv2 * s->tsize;
        s->solve_stamp = 4;
    } else {
        ok = ok && zeros_T(&s->d_val, nval) && zeros_T(&s->d_b, nb);
        s->sys_val = s->d_val;
        s->sys_b = s->d_b;
    }
    ok = ok && mem.alloc(&s->d_rhs, std::max<int64_t>(P.n, 1), false) && (!(f32 && uses_mf(s)) || mem.alloc(&s->d_val64, nval, false)) &&
         mem.upload(&s->elim_ref, std::vector<int32_t>(s->ref_dof.begin(), s->ref_dof.begin() + P.n));
    if (!uses_mf(s))
        ok = ok && mem.upload(&s->d_rowptr, P.rowptr) && mem.upload(&s->d_colind, P.colind) && mem.upload(&s->csr_src, P.blk.csr_src) &&
             mem.alloc(&s->d_csr64, std::max<int64_t>(P.nnzA(), 1), false);
    return ok ? BOS_OK : no_mem("system");
}

// the multifrontal engine, or rocSOLVER's refactorization arrays, or the dense matrix
int create_solver_backend(bos_solver* s) {
    const bos::Plan& P = s->plan;
    bos::dev::DeviceMem& mem = s->mem;
    if (uses_mf(s)) {
        std::string merr;
        if (bos::dev::mf_create(P.mf, s->sharded ? P.shard.sn_owner.data() : nullptr, s->rank, &s->mf, merr))
            return fail(BOS_ERR_DEVICE, merr);
        s->fold32 = s->pl_factored && bos::mf_fold_reads_fp32(P);
        if (s->fold32) bos::dev::mf_set_fold_source(s->mf, (const float*)s->sys_val, P.blk.off_pl);
    } else if (s->solver_kind == BOS_SOLVER_ROCSOLVER_RF) {
        std::vector<int32_t> piv(P.n);
        for (int64_t i = 0; i < P.n; ++i) piv[i] = (int32_t)i;   // ordering already applied in the layout
        if (!(mem.upload(&s->d_Lptr, P.Lptr) && mem.upload(&s->d_Lind, P.Lind) && mem.upload(&s->d_pivQ, piv) &&
              mem.alloc(&s->d_Lval, std::max<int64_t>(P.nnzL(), 1), true)))
            return no_mem("factor structure");
    } else if (!mem.alloc(&s->d_dense, (size_t)P.n * P.n, false)) {
        return no_mem("dense matrix");
    }
    return BOS_OK;
}

// the step's partials, solver word and status (the abort flag is sticky) with its host-mapped mirror
int alloc_status(bos_solver* s) {
    bos::dev::DeviceMem& mem = s->mem;
    const int nt = std::max(1, s->pose_blocks * bos::dev::kJhSub);   // chi^2 partials: one per pose workgroup
    if (!(mem.alloc(&s->d_info, 1, true) && mem.alloc(&s->d_chi_part, nt, true) && mem.alloc(&s->d_nrob_part, nt, true) &&
          mem.alloc(&s->d_status, 1, true) &&
          mem.alloc(&s->d_maxpart, (size_t)std::max(1, (s->NP + s->NL + bos::dev::kUpdateBlock - 1) / bos::dev::kUpdateBlock), false)))
        return no_mem("step status");
    if (!mem.host_mapped(&s->h_status, &s->m_status)) return fail(BOS_ERR_DEVICE, "host-mapped status allocation failed");
    return BOS_OK;
}

// triangulation inputs (kept for bos_triangulate) and the bearings' landmarks
int stage_triangulation(bos_solver* s, const bos_problem* pb) {
    bos::dev::DeviceMem& mem = s->mem;
    s->bearing_lm.assign(pb->bearing_landmark, pb->bearing_landmark + s->Mb);
    std::vector<int32_t> tptr(s->NL + 1, 0), tobs(s->Mb), tpose(pb->bearing_pose, pb->bearing_pose + s->Mb);
    for (int k = 0; k < s->Mb; ++k) ++tptr[pb->bearing_landmark[k] + 1];
    for (int l = 0; l < s->NL; ++l) tptr[l + 1] += tptr[l];
    std::vector<int32_t> w(tptr.begin(), tptr.end() - 1);
    for (int k = 0; k < s->Mb; ++k) tobs[w[pb->bearing_landmark[k]]++] = k;
    std::vector<double> tz(pb->bearing_z, pb->bearing_z + s->Mb);
    if (!(mem.upload(&s->tri_ptr, tptr) && mem.upload(&s->tri_obs, tobs) && mem.upload(&s->tri_pose, tpose) &&
          mem.upload(&s->tri_z, tz) && mem.alloc(&s->tri_scr, 3 * (size_t)std::max(1, s->Mb), false)))
        return no_mem("triangulation inputs");
    return BOS_OK;
}

// the landmarks where none were given, then the state caches in T
int init_state(bos_solver* s, const bos_problem* pb) {
    int rc;
    if (!pb->landmark_xy && s->NL) {
        if ((rc = enqueue_triangulate(s))) return rc;
        HIP_TRY(hipStreamSynchronize(s->stream));   // upload_cache reads the landmarks back
    }
    if ((rc = upload_cache(s))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return BOS_OK;
}

}  // namespace

extern "C" {

void bos_default_options(bos_options* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->precision = BOS_FP64;
    o->solver = BOS_SOLVER_SPARSE_CHOL;
    o->device = -1;
    o->rank = 0;
    o->world_size = 1;
    o->kernel_threshold = 1.0;
    o->damping = 0.01;
}

// Graphs are dropped and the stream drained before anything is freed; the handle's memory goes last,
// with the handle (bos_solver::mem)
int bos_destroy(bos_solver* s) {
    if (!s) return BOS_OK;
    if (s->device >= 0) (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    drop_graph(s);
    for (void* m : s->peer_maps) (void)hipIpcCloseMemHandle(m);
    if (s->rf) rocsolver_destroy_rfinfo(s->rf);
    if (s->mf) bos::dev::mf_destroy(s->mf);
    bos::dev::pair_cov_destroy(s->pair);
    bos::dev::node_cov_destroy(s->node);
    bos::dev::associate_destroy(s->assoc);
    bos::dev::match_destroy(s->match);
    bos::dev::joint_destroy(s->joint);
    bos::dev::jcbb_destroy(s->jcbb);
    bos::dev::edge_check_destroy(s->edge_check);
    if (s->rb) rocblas_destroy_handle(s->rb);
    if (s->comm) ncclCommDestroy(s->comm);
    for (hipEvent_t& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return BOS_OK;
}

int bos_create(const bos_problem* pb, const bos_options* opt_in, bos_solver** out) {
    if (!pb || !out) return fail(BOS_ERR_INVALID, "bos_create: null argument");
    *out = nullptr;
    bos_options opt;
    bos_default_options(&opt);
    if (opt_in) opt = *opt_in;
    int ndev = 0, rc;
    if ((rc = check_arguments(pb, opt, ndev))) return rc;
    // from here every return destroys the half-built handle
    std::unique_ptr<bos_solver, int (*)(bos_solver*)> handle(new bos_solver(), bos_destroy);
    bos_solver* s = handle.get();
    if ((rc = build_plan(s, pb, opt, ndev)) || (rc = create_streams_and_libraries(s, opt)) || (s->sharded && (rc = setup_shard(s))) ||
        (rc = upload_state(s, pb)) || (rc = stage_jh_inputs(s, pb)) || (rc = alloc_system(s)) || (rc = create_solver_backend(s)) ||
        (rc = alloc_status(s)) || (rc = stage_triangulation(s, pb)) || (rc = init_state(s, pb)))
        return rc;
    *out = handle.release();
    return BOS_OK;
}

}  // extern "C"
