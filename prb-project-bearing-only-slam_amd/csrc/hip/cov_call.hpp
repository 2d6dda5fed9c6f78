// What the covariance entry points share (solver_cov.hip, solver_cov_pair.hip, solver_cov_node.hip, which alone
// include this): the device layers' codes as BOS errors, the feature setups, and the frame of a call that reads
// the factorization's word before anything reads the panels (CovCall). An entry point runs, in this order:
// cov_handle_check, its argument rule, the empty call (BOS_OK, nothing touched), begin(), its fill for
// plan.n == 0, its lazy setup, factor(), its own work, done().
#pragma once

#include <algorithm>
#include <chrono>

#include "../host/row_lists.hpp"
#include "solver_handle.hpp"

namespace bos {
namespace capi {

typedef std::chrono::steady_clock Clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// the device layers' codes: -1 is a shape they do not run, anything else a device failure
inline int dev_fail(int prc, const std::string& err) { return fail(prc == -1 ? BOS_ERR_UNSUPPORTED : BOS_ERR_DEVICE, err); }
// kMfStall in the factorization's word
inline int stall_fail() { return fail(BOS_ERR_SOLVER, "sparse factorization aborted: a dataflow dependency wait timed out"); }
// a timing getter's outputs: the feature's n slots and, where asked for, its device bytes
inline int timing_out(const double* slots, int n, double* ms, int64_t* bytes, int64_t feature_bytes) {
    std::copy_n(slots, n, ms);
    if (bytes) *bytes = feature_bytes;
    return BOS_OK;
}

// solver_cov.hip
hipError_t take_factor_info(bos_solver* s, int32_t* info);
int enqueue_factorization(bos_solver* s, int32_t* info_now);
int edge_cov_setup(bos_solver* s);
int pair_paths_setup(bos_solver* s, const char* name);
int node_cov_setup(bos_solver* s, const char* name);
// the null handle, then a handle that does not hold the whole multifrontal factor on one GPU
int cov_handle_check(const bos_solver* s, const char* name);

struct CovCall {
    bos_solver* s;
    double* ms;             // the feature's slots on the handle: 0 host preparation, 1 J+H, 2 factorization
    int n_ms;
    int32_t* solver_info;   // the caller's, may be null
    int32_t info = 0;       // the factorization's word
    Clock::time_point t_begin = {};

    // the handle's device, *solver_info and the slots zeroed
    int begin();
    // The host's time since begin() to slot 0, then the system and its factorization (enqueue_factorization),
    // the word read and cleared and the stream drained; fails on kMfStall, with *solver_info left 0
    int factor();
    // the marginals' own pass on this factorization, between events 2 and 3, to slot 3: *sig is Sigma's
    // diagonal blocks (device, [9 NP | 4 NL]); emit_cross: the edges' cross blocks into the pair buffer as well
    // (after edge_cov_setup), as bos_edge_covariances' pass runs it
    int selected_inverse(const double** sig, bool emit_cross = false);
    // event ev recorded and the stream drained, then the device layers' code of what was enqueued (dev_fail)
    int drain(int ev, int prc, const std::string& err);
    void host_ms(int slot, Clock::time_point t0) { ms[slot] += ms_since(t0); }
    int done() {
        if (solver_info) *solver_info = info;
        return BOS_OK;
    }
};

// B's tables as the pair call's device layer takes them; q_a, q_b: the batch's node ids
inline bos::dev::PairCovBatch pair_batch_view(const bos::PairBatchHost& B, const int32_t* q_a, const int32_t* q_b) {
    bos::dev::PairCovBatch b;
    b.n_nodes = (int32_t)B.n_node.size(); b.n_queries = B.nq; b.y_count = B.y_count;
    b.y_off = B.y_off.data(); b.n_sn = B.n_sn.data(); b.n_loc = B.n_loc.data(); b.n_d = B.n_d.data(); b.n_len = B.n_len.data();
    b.q_a = q_a; b.q_b = q_b; b.q_slot_a = B.q_slot_a.data(); b.q_slot_b = B.q_slot_b.data();
    b.q_off_a = B.q_off_a.data(); b.q_off_b = B.q_off_b.data(); b.q_c = B.q_c.data();
    return b;
}

// What bos_associate_bearings and the matching calls run after factor(): the selected inverse (the projection's
// diagonal blocks), the column-and-chunk loop, done(). Per group of G: the column of node node_base + the
// group's (outputs want), then the group's rows in chunks of at most chunk_rows; one_row: the column gives one
// row, which every query of the group receives. enqueue(a, col, rows, dst, err) stages and enqueues a chunk,
// events 5 and 6 around its first kernel (row i is query dst[i].second; the device layers' codes);
// download(rows, dst) takes its results to the caller's arrays (a BOS code). Events 4 .. 7 and the download's
// host time feed slots 4 .. 7, the column's time once per group.
template <class Enqueue, class Download>
int column_chunks(CovCall& c, const bos::RowGroups& G, int node_base, bool one_row, const bool want[4], int chunk_rows,
                  Enqueue enqueue, Download download) {
    bos_solver* s = c.s;
    int rc;
    const double* sig = nullptr;
    if ((rc = c.selected_inverse(&sig))) return rc;
    const bos::dev::MfView view = bos::dev::mf_view(s->mf);
    std::vector<bos::RowDest> dst;
    for (size_t g = 0; g < G.nodes.size(); ++g) {
        const int a = G.nodes[g], a_node = node_base + a;
        const std::vector<int32_t>& mem = G.members[g];
        std::string err;
        bos::dev::NodeCovDev col;
        HIP_TRY(hipEventRecord(s->ev[4], s->stream));
        const int prc = bos::dev::node_cov_enqueue(s->node, view, a_node, a_node == s->plan.fixed, want, sig, s->d_pose, s->d_lm, s->stream,
                                                   nullptr, &col, err);
        if (prc) return dev_fail(prc, err);
        const size_t rows_of_node = one_row ? 1 : mem.size();
        for (size_t c0 = 0; c0 < rows_of_node; c0 += (size_t)chunk_rows) {
            const size_t rows = std::min(rows_of_node - c0, (size_t)chunk_rows);
            dst.clear();
            if (one_row)
                for (int32_t q : mem) dst.emplace_back(0, q);
            else
                for (size_t i = 0; i < rows; ++i) dst.emplace_back((int32_t)i, mem[c0 + i]);
            if ((rc = c.drain(7, enqueue(a, col, rows, dst, err), err))) return rc;
            if (c0 == 0) c.ms[4] += elapsed(s->ev[4], s->ev[5]);
            c.ms[5] += elapsed(s->ev[5], s->ev[6]);
            c.ms[6] += elapsed(s->ev[6], s->ev[7]);
            const auto t_dl = Clock::now();
            if ((rc = download(rows, dst))) return rc;
            c.host_ms(7, t_dl);
        }
    }
    return c.done();
}

}  // namespace capi
}  // namespace bos
