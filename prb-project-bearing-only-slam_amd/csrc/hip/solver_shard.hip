// The multi-rank forms of the GN step on the C ABI handle (solver_handle.hpp), their exchanges and
// entry points.
// Sharded over world > 1 ranks, BOS_PARTITION_SUBTREE (host/plan.hpp Shard, host/shard.cpp): the
// J+H runs this rank's own and the top nodes' lanes, the multifrontal solve its subtrees, then
// (exchange 1, all-gather of the subtree roots' U / u) the replicated top, the backward solves, then
// (exchange 2, all-gather of the boundary solution) the box-plus of its own, top and boundary nodes.
// BOS_PARTITION_OBSERVATIONS (the north star's form): the J+H runs a contiguous range of the
// one-GPU plan's lanes, one all-reduce (sum) of (H, b) and the chi^2 header, then the one-GPU solve
// and box-plus on every rank. The exchanges run on RCCL, or — external mode, no communicator — the
// caller moves the buffers between the phases (bos_step_phase; tests on one GPU, gloo).
#include <algorithm>
#include <cstring>

#include "solver_handle.hpp"

using namespace bos::capi;

namespace {

// ---- sharded GN iteration in three phases (exchanges between them). With a communicator the
// whole iteration — the phases and the two ncclAllGather calls between them — is captured once into
// one graph and replayed (do_step_sharded); in external mode (the caller moves the buffers) each
// phase is a graph of its own. Phase boundaries are stamped by the phases' own kernels (StepStatus
// stamp slots 0-7), not by events.
// phase 0: J+H (own + top lanes), solver inputs, own subtrees factored (and forward-solved),
// exchange-1 buffer packed (roots' U / u, this rank's chi^2 partials)
// phase 1: the other ranks' roots in place, the top factored and solved, own subtrees solved
// backward, exchange-2 buffer packed (max |x| of own + top, solver word, boundary solution)
// phase 2: boundary solution in place, box-plus of own + top + boundary nodes (skipped when any
// rank's factorization aborted: every rank's header), step status combined from every rank's headers
// the wait for exchange `which` of the direct exchange, fused into the launch that reads it (none
// without the direct exchange)
bos::dev::P2PWait p2p_wait(const bos_solver* s, int which) {
    bos::dev::P2PWait w;
    if (!s->p2p) return w;
    w.mailbox = s->mailbox;
    w.flag_off = which == 1 ? s->mb_flag1 : s->mb_flag2;
    w.world = s->world;
    w.epoch = bos::dev::mf_epoch_ptr(s->mf);
    w.info = bos::dev::mf_info_ptr(s->mf);
    w.timeout_ticks = s->ex_timeout_ticks;
    return w;
}

// the one exchange: (H values | b) in T and the header, summed over the ranks (one RCCL group)
int rccl_allreduce_obs(bos_solver* s) {
    const ncclDataType_t t = s->precision == BOS_FP32 ? ncclFloat : ncclDouble;
    NC_TRY(ncclGroupStart());
    const ncclResult_t r1 = ncclAllReduce(s->d_val, s->d_sys, (size_t)s->vb_count, t, ncclSum, s->comm, s->stream);
    const ncclResult_t r2 = ncclAllReduce(s->ex1_send, s->ex1_recv, bos::kExHeader, ncclDouble, ncclSum, s->comm, s->stream);
    NC_TRY(ncclGroupEnd());
    NC_TRY(r1);
    NC_TRY(r2);
    return BOS_OK;
}

// one phase of either partition: its graph (captured on first use; capture's phase numbers)
int run_phase(bos_solver* s, int phase) {
    int rc;
    if (!s->pexec[phase] && !s->graph_failed && (rc = capture(s, (s->obs ? 10 : 0) + phase, &s->pgraph[phase], &s->pexec[phase])))
        return rc;
    if (s->pexec[phase]) HIP_TRY(hipGraphLaunch(s->pexec[phase], s->stream));
    else if ((rc = s->obs ? obs_enqueue(s, phase) : shard_enqueue(s, phase))) return rc;
    return BOS_OK;
}

// one all-gather of the sharded step: RCCL, or the direct peer exchange's push to every rank's
// mailbox (the push gathers its payload and computes the header; the receiving side's wait is fused
// into the launch that reads the data, p2p_wait)
int exchange(bos_solver* s, int which) {
    const double* send = which == 1 ? s->ex1_send : s->ex2_send;
    double* recv = which == 1 ? s->ex1_recv : s->ex2_recv;
    const int64_t count = which == 1 ? s->ex1_count : s->ex2_count;
    if (!s->p2p) {
        NC_TRY(ncclAllGather(send, recv, (size_t)count, ncclDouble, s->comm, s->stream));
        return BOS_OK;
    }
    const int64_t data = which == 1 ? s->mb_ex1 : s->mb_ex2, flag = which == 1 ? s->mb_flag1 : s->mb_flag2;
    // the push gathers its payload where it lives (exchange 1: the subtree roots' U / u by the pack
    // segments, with the chi^2 header; exchange 2: the boundary solution with the max |x| / solver-word
    // header): no pack launch before it
    bos::dev::P2PPush p;
    p.which = which;
    p.peers = s->d_peers;
    p.data_off = data;
    p.flag_off = flag;
    p.count = count;
    p.rank = s->rank;
    p.world = s->world;
    p.epoch = bos::dev::mf_epoch_ptr(s->mf);
    if (which == 1) {
        p.stamp = s->d_status->stamp + 4;
        p.chi_part = s->d_chi_part;
        p.nrob_part = s->d_nrob_part;
        p.n_parts = s->chi_parts;
        p.U = bos::dev::mf_update_ptr(s->mf);
        p.u = bos::dev::mf_uvec_ptr(s->mf);
        p.segs = s->ex1_pack;
        p.nseg = s->n1p;
    } else {
        p.stamp = s->d_status->stamp + 6;
        p.x = s->d_rhs;
        p.abs_part = s->abs_part;
        p.n_abs = s->n_abs;
        p.info = bos::dev::mf_info_ptr(s->mf);
        p.bnd = s->ex2_bnd;
        p.n_bnd = s->n_bnd;
    }
    HIP_TRY(bos::dev::launch_p2p_push_gather(p, s->stream));
    return BOS_OK;
}

// the whole sharded iteration with its exchanges (on the handle's stream); with_jh false:
// everything after the J+H build
int enqueue_sharded_step(bos_solver* s, bool with_jh = true) {
    int rc;
    if ((rc = shard_enqueue(s, 0, with_jh)) || (rc = exchange(s, 1)) || (rc = shard_enqueue(s, 1)) ||
        (rc = exchange(s, 2)))
        return rc;
    return shard_enqueue(s, 2);
}

// the whole observations-partition iteration with its all-reduce (with_jh false: after the J+H build)
int enqueue_obs_step(bos_solver* s, bool with_jh = true) {
    int rc;
    if ((rc = obs_enqueue(s, 0, with_jh)) || (rc = rccl_allreduce_obs(s))) return rc;
    return obs_enqueue(s, 1);
}

// One graph for a multi-rank iteration with its RCCL collectives, and one of the iteration after
// its J+H build (captured on first use). If the collectives cannot be captured,
// rccl_capture_failed is set and the caller runs the phase graphs with the collectives between them
// instead (the same launches in the same order).
int capture_rccl_graph(bos_solver* s, bool with_jh, hipGraph_t* graph, hipGraphExec_t* exec) {
    if (hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        s->graph_failed = true;
        return BOS_OK;
    }
    const int rc = s->obs ? enqueue_obs_step(s, with_jh) : enqueue_sharded_step(s, with_jh);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s->stream, &g);
    if (rc || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        s->rccl_capture_failed = true;   // (a launch error reappears on the eager path)
        return BOS_OK;
    }
    if (hipGraphInstantiate(exec, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipGraphDestroy(g);
        *exec = nullptr;
        s->rccl_capture_failed = true;
        return BOS_OK;
    }
    *graph = g;
    return BOS_OK;
}

int capture_rccl_step(bos_solver* s) {
    int rc;
    if (s->graph_failed || s->rccl_capture_failed) return BOS_OK;
    if (!s->sexec && (rc = capture_rccl_graph(s, true, &s->sgraph, &s->sexec))) return rc;
    if (s->sexec && !s->stail_exec && (rc = capture_rccl_graph(s, false, &s->stail, &s->stail_exec))) return rc;
    return BOS_OK;
}

}  // namespace

namespace bos {
namespace capi {

int shard_enqueue(bos_solver* s, int phase, bool with_jh) {
    int rc;
    double* U = bos::dev::mf_update_ptr(s->mf);
    double* u = bos::dev::mf_uvec_ptr(s->mf);
    if (phase == 0) {
        if (with_jh && (rc = enqueue_linearize(s, s->d_status->stamp))) return rc;
        if ((rc = enqueue_solver_inputs(s))) return rc;   // opens this step's flow epoch
        HIP_TRY(bos::dev::mf_factor(s->mf, 0, mf_matrix(s), s->d_rhs, s->stream));
        if (!s->p2p) {   // (the direct exchange's push gathers the payload and computes the header itself)
            HIP_TRY(bos::dev::launch_seg_copy<double>(U, u, s->ex1_send, s->ex1_recv, s->hdr1, s->ex1_pack, s->n1p,
                                                      s->maxlen1p, s->stream));
            HIP_TRY(bos::dev::launch_shard_header1(s->d_chi_part, s->d_nrob_part, s->chi_parts, s->ex1_send, s->stream,
                                                   s->d_status->stamp + 4));
        }
    } else if (phase == 1) {
        HIP_TRY(bos::dev::launch_seg_copy<double>(U, u, s->ex1_send, s->ex1_recv, s->hdr1, s->ex1_unpack, s->n1u, s->maxlen1u,
                                                  s->stream, s->d_status->stamp + 5, p2p_wait(s, 1)));
        HIP_TRY(bos::dev::mf_factor(s->mf, 1, mf_matrix(s), s->d_rhs, s->stream));
        HIP_TRY(bos::dev::mf_solve(s->mf, 1, s->d_rhs, s->stream));
        HIP_TRY(bos::dev::mf_solve(s->mf, 0, s->d_rhs, s->stream));
        if (s->p2p) {   // the push packs exchange 2 itself (exchange()); the max |x| partials first
            hipError_t e = hipSuccess;
            s->n_abs = bos::dev::launch_node_absmax(s->d_rhs, s->upd_nodes, s->n_upd_local, s->node_dof, s->NP,
                                                    s->abs_part, s->stream, &e);
            HIP_TRY(e);
        } else {
            HIP_TRY(bos::dev::launch_shard_pack2(s->d_rhs, s->upd_nodes, s->n_upd_local, s->node_dof, s->NP,
                                                 bos::dev::mf_info_ptr(s->mf), s->ex2_bnd, s->n_bnd, s->abs_part,
                                                 s->ex2_send, s->stream, s->d_status->stamp + 6));
        }
    } else {
        HIP_TRY(bos::dev::launch_index_copy(s->ex2_recv, s->ex2_usrc, s->d_rhs, s->ex2_udst, s->n_bnd_remote, s->stream,
                                            s->d_status->stamp + 7, p2p_wait(s, 2)));
        if ((rc = enqueue_update(s))) return rc;
        int32_t nrob_c = 0;
        const double chi_c = self_loop_chi(s, nrob_c);
        // exchange-1 headers from phase 1's local copy (the mailbox may already hold the next
        // iteration's); exchange 2's are still current (no rank pushes again before this rank does)
        HIP_TRY(bos::dev::launch_shard_combine(s->hdr1, bos::kExHeader, s->ex2_recv, s->ex2_count, s->world, chi_c,
                                               nrob_c, bos::dev::mf_info_ptr(s->mf), s->d_status, s->m_status, s->stream,
                                               s->p2p));
    }
    return BOS_OK;
}

// ---- BOS_PARTITION_OBSERVATIONS step (the north star's form): phase 0 = this rank's range of J+H
// lanes and its chi^2 / robust-count header (external mode: the whole [header | H values | b] in
// fp64 into the exchange buffer); one all-reduce (sum) over the ranks; phase 1 = (external: the
// summed buffer back into T) the one-GPU solve, box-plus of every node and stats. Every value of H and
// b is written by exactly one rank's lanes and is zero on the others, so the sum is exact and every
// rank solves the one-GPU system bit for bit.
int obs_enqueue(bos_solver* s, int phase, bool with_jh) {
    int rc;
    const bool f32 = s->precision == BOS_FP32;
    if (phase == 0) {
        if (with_jh && (rc = enqueue_linearize(s, s->d_status->stamp))) return rc;
        HIP_TRY(bos::dev::launch_shard_header1(s->d_chi_part, s->d_nrob_part, s->chi_parts, s->ex1_send, s->stream,
                                               s->d_status->stamp + 1));
        if (s->external)
            HIP_TRY(f32 ? bos::dev::launch_to_f64<float>((const float*)s->d_val, s->ex1_send + bos::kExHeader, s->vb_count, s->stream)
                        : bos::dev::launch_to_f64<double>((const double*)s->d_val, s->ex1_send + bos::kExHeader, s->vb_count, s->stream));
        return BOS_OK;
    }
    if (s->external)
        HIP_TRY(f32 ? bos::dev::launch_from_f64<float>(s->ex1_recv + bos::kExHeader, (float*)s->d_sys, s->vb_count, s->stream)
                    : bos::dev::launch_from_f64<double>(s->ex1_recv + bos::kExHeader, (double*)s->d_sys, s->vb_count, s->stream));
    return enqueue_step_tail(s);
}

// A multi-rank iteration on RCCL (sharded or observations partition): a batch's steps before its
// last replay the whole iteration's graph; a synchronous step launches its J+H build directly and
// the rest as a graph submitted while the build runs (as the one-GPU step, launch_step).
int launch_rccl_step(bos_solver* s, bool sync) {
    int rc;
    if ((rc = capture_rccl_step(s))) return rc;
    if (!sync && s->sexec) {
        HIP_TRY(hipGraphLaunch(s->sexec, s->stream));
    } else if (s->stail_exec) {
        if ((rc = enqueue_linearize(s, s->d_status->stamp))) return rc;
        HIP_TRY(hipGraphLaunch(s->stail_exec, s->stream));
    } else if (s->obs) {
        if ((rc = run_phase(s, 0)) || (rc = rccl_allreduce_obs(s)) || (rc = run_phase(s, 1))) return rc;
    } else if ((rc = run_phase(s, 0)) || (rc = exchange(s, 1)) || (rc = run_phase(s, 1)) || (rc = exchange(s, 2)) ||
               (rc = run_phase(s, 2))) {
        return rc;
    }
    ++s->seq_pending;   // the iteration's status launch bumps the device counter once
    return BOS_OK;
}

int do_step_sharded(bos_solver* s, bos_step_stats* st, bool sync) {
    if (!s->comm && !s->p2p)
        return fail(BOS_ERR_INVALID, "sharded handle without a communicator or direct exchange: drive bos_step_phase");
    int rc;
    if ((rc = launch_rccl_step(s, sync))) return rc;
    s->have_dx = true;
    if (!sync) return BOS_OK;
    return finish_step(s, st);
}

}  // namespace capi
}  // namespace bos

extern "C" {

int bos_nccl_unique_id(void* out, int64_t len) {
    if (!out || len < (int64_t)sizeof(ncclUniqueId)) return fail(BOS_ERR_INVALID, "bos_nccl_unique_id: buffer too small");
    ncclUniqueId id;
    NC_TRY(ncclGetUniqueId(&id));
    std::memcpy(out, &id, sizeof(id));
    return BOS_OK;
}

int bos_step_phase(bos_solver* s, int32_t phase, bos_step_stats* st) {
    if (!s) return fail(BOS_ERR_INVALID, "null handle");
    if (s->obs) {   // observations partition: phases 0 and 1, the all-reduce between them
        if (phase != s->phase) return fail(BOS_ERR_INVALID, "bos_step_phase: phases run 0, 1 in order");
        HIP_TRY(hipSetDevice(s->device));
        const int rc = run_phase(s, phase);
        if (rc) { s->phase = 0; return rc; }
        s->phase = (phase + 1) % 2;
        if (phase == 0) return BOS_OK;
        ++s->seq_pending;
        s->have_dx = true;
        return finish_step(s, st);
    }
    if (!s->sharded) return fail(BOS_ERR_INVALID, "bos_step_phase needs a sharded handle (world_size > 1)");
    if (s->p2p) return fail(BOS_ERR_INVALID, "bos_step_phase: the handle exchanges directly (bos_exchange_p2p_connect); use bos_step");
    if (phase != s->phase) return fail(BOS_ERR_INVALID, "bos_step_phase: phases run 0, 1, 2 in order");
    HIP_TRY(hipSetDevice(s->device));
    const int rc = run_phase(s, phase);
    if (rc) { s->phase = 0; return rc; }
    s->phase = (phase + 1) % 3;
    if (phase < 2) return BOS_OK;
    ++s->seq_pending;   // phase 2's status launch bumps the device counter
    s->have_dx = true;
    return finish_step(s, st);
}

int bos_exchange_size(const bos_solver* s, int32_t which, int64_t* doubles_per_rank) {
    if (!s || !doubles_per_rank || (which != 1 && which != 2)) return fail(BOS_ERR_INVALID, "bad argument");
    if (!s->sharded && !(s->obs && which == 1)) return fail(BOS_ERR_INVALID, "not a sharded handle / no such exchange");
    *doubles_per_rank = which == 1 ? s->ex1_count : s->ex2_count;
    return BOS_OK;
}

int bos_exchange_download(bos_solver* s, int32_t which, double* send) {
    if (!s || !send || (which != 1 && which != 2)) return fail(BOS_ERR_INVALID, "bad argument");
    if (s->p2p) return fail(BOS_ERR_INVALID, "bos_exchange_download: the handle exchanges directly (bos_exchange_p2p_connect)");
    if (!s->sharded && !(s->obs && which == 1)) return fail(BOS_ERR_INVALID, "not a sharded handle / no such exchange");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int64_t c = which == 1 ? s->ex1_count : s->ex2_count;
    HIP_TRY(hipMemcpy(send, which == 1 ? s->ex1_send : s->ex2_send, c * sizeof(double), hipMemcpyDeviceToHost));
    return BOS_OK;
}

int bos_exchange_upload(bos_solver* s, int32_t which, const double* recv_all) {
    if (!s || !recv_all || (which != 1 && which != 2)) return fail(BOS_ERR_INVALID, "bad argument");
    if (s->p2p) return fail(BOS_ERR_INVALID, "bos_exchange_upload: the handle exchanges directly (bos_exchange_p2p_connect)");
    if (!s->sharded && !(s->obs && which == 1)) return fail(BOS_ERR_INVALID, "not a sharded handle / no such exchange");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    // subtree partition: every rank's buffer (all-gather); observations partition: their sum
    const int64_t c = s->obs ? s->ex1_count : (which == 1 ? s->ex1_count : s->ex2_count) * s->world;
    HIP_TRY(hipMemcpy(which == 1 ? s->ex1_recv : s->ex2_recv, recv_all, c * sizeof(double), hipMemcpyHostToDevice));
    return BOS_OK;
}

int bos_set_exchange_timeout(bos_solver* s, double seconds) {
    if (!s || !(seconds > 0.0) || seconds > 3600.0) return fail(BOS_ERR_INVALID, "bad argument");
    const uint64_t t = (uint64_t)(seconds * 1e8);   // 100 MHz realtime clock
    if (t != s->ex_timeout_ticks) drop_graph(s);     // a launch argument of the captured step
    s->ex_timeout_ticks = t;
    return BOS_OK;
}

int bos_exchange_p2p_handle(bos_solver* s, void* handle) {
    if (!s || !handle) return fail(BOS_ERR_INVALID, "null argument");
    if (!s->sharded) return fail(BOS_ERR_UNSUPPORTED, "direct exchange: subtree-sharded handles only");
    if (!s->mailbox_uncached) return fail(BOS_ERR_UNSUPPORTED, "direct exchange: no uncached device memory for the mailbox");
    HIP_TRY(hipSetDevice(s->device));
    hipIpcMemHandle_t h;
    const hipError_t e = hipIpcGetMemHandle(&h, s->mailbox);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(BOS_ERR_UNSUPPORTED, std::string("direct exchange: hipIpcGetMemHandle: ") + hipGetErrorString(e));
    }
    static_assert(sizeof(h) == BOS_P2P_HANDLE_BYTES, "IPC handle size");
    std::memcpy(handle, &h, sizeof(h));
    return BOS_OK;
}

int bos_exchange_p2p_connect(bos_solver* s, const void* handles) {
    if (!s || !handles) return fail(BOS_ERR_INVALID, "null argument");
    if (!s->sharded || !s->mailbox_uncached) return fail(BOS_ERR_UNSUPPORTED, "direct exchange: not available on this handle");
    if (s->p2p) return fail(BOS_ERR_INVALID, "direct exchange: already connected");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    // the peers' mailboxes are written by this device's kernels: every other visible device must be
    // reachable (xGMI), or the caller keeps the RCCL exchange
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    for (int d = 0; d < ndev; ++d) {
        int ok = 0;
        if (d != s->device && (hipDeviceCanAccessPeer(&ok, s->device, d) != hipSuccess || !ok)) {
            (void)hipGetLastError();
            return fail(BOS_ERR_UNSUPPORTED, "direct exchange: device " + std::to_string(s->device) +
                                                 " has no peer access to device " + std::to_string(d));
        }
    }
    std::vector<double*> peers(s->world, nullptr);
    for (int q = 0; q < s->world; ++q) {
        if (q == s->rank) { peers[q] = reinterpret_cast<double*>(s->mailbox); continue; }
        hipIpcMemHandle_t h;
        std::memcpy(&h, static_cast<const char*>(handles) + (size_t)q * BOS_P2P_HANDLE_BYTES, sizeof(h));
        void* p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess || !p) {
            (void)hipGetLastError();
            for (void* m : s->peer_maps) (void)hipIpcCloseMemHandle(m);
            s->peer_maps.clear();
            return fail(BOS_ERR_UNSUPPORTED, std::string("direct exchange: hipIpcOpenMemHandle (rank ") + std::to_string(q) +
                                                 "): " + hipGetErrorString(e));
        }
        s->peer_maps.push_back(p);
        peers[q] = reinterpret_cast<double*>(p);
    }
    if (!s->mem.upload(&s->d_peers, peers)) return fail(BOS_ERR_DEVICE, "direct exchange: device allocation or upload failed");
    drop_graph(s);   // the next step captures the iteration with the direct exchange
    s->rccl_capture_failed = false;
    s->p2p = true;
    return BOS_OK;
}

int bos_node_owner(const bos_solver* s, int32_t* owner) {
    if (!s || !owner) return fail(BOS_ERR_INVALID, "null argument");
    if (s->obs) return fail(BOS_ERR_UNSUPPORTED, "observations partition: every rank holds every node");
    const std::vector<int32_t>& o = s->plan.shard.node_owner;
    if (o.empty()) return fail(BOS_ERR_UNSUPPORTED, "no shard (not a multifrontal solver)");
    std::copy(o.begin(), o.end(), owner);
    return BOS_OK;
}

}  // extern "C"
