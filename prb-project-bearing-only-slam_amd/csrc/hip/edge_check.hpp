// Edge consistency on the device (hip/edge_check.hip): see host/edge_check.hpp for the quantities. In plain
// stream order behind the projection kernel (hip/edge_cov.hip) whose bearing_var / odom_cov it reads in
// place: the scoring kernel, one thread per edge, then per kind the shared selection's two stages
// (hip/topk_select.hpp) over the one row of negated scores. No kernel communicates between workgroups, none
// uses an atomic, and a list is the unique minimum of a total order: it depends on no grid shape.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../host/edge_check.hpp"

namespace bos {
namespace dev {

struct EdgeCheck;   // the feature's device buffers; owned by the solver handle

constexpr int kEdgeCheckBlock = 256;

// What the scoring kernel reads, every pointer device memory: the master state, the edges and their fp64
// measurements as the cost pass reads them (hip/lm.hpp CostParams), and the projection's outputs
struct EdgeCheckIn {
    int Mb = 0, Mo = 0;
    const double *pose = nullptr, *lm = nullptr;
    const int32_t *b_pose = nullptr, *b_lm = nullptr, *o_src = nullptr, *o_dst = nullptr;
    const double *b_z = nullptr, *b_w = nullptr;    // b_w null: 1
    const double *o_z = nullptr, *o_om = nullptr;   // [Mo][3]; [Mo][6] upper triangle
    const double *bearing_var = nullptr, *odom_cov = nullptr;   // [Mb]; [Mo][9]
};

// The lists of one kind as the device keeps them, downloaded in one copy: the selection's own outputs (ix,
// score: the negated w2, +inf where nothing is listed; n_over) and the epilogue's (w2, e, T). An entry's e
// and T take the first 1 (bearing) or 3 and 9 (odometry) doubles of its slot.
struct EdgeCheckLists {
    int32_t ix[kEdgeCheckMaxK];
    int32_t n_over, pad;
    double score[kEdgeCheckMaxK], w2[kEdgeCheckMaxK], e[kEdgeCheckMaxK][3], T[kEdgeCheckMaxK][9];
};
// what a default call downloads per kind: bos.py EDGE_CHECK_LIST_BYTES (tools/edge_consistency_time.py reports it)
static_assert(sizeof(EdgeCheckLists) == 936, "bos.py EDGE_CHECK_LIST_BYTES and the documents' 1 872 bytes follow this struct");

// per-edge rows on the device: the negated scores and, where asked for, chi2 and the redundancy numbers
struct EdgeCheckDev {
    const EdgeCheckLists* lists = nullptr;   // [2]: bearings, odometry
    const double *b_neg = nullptr, *b_chi2 = nullptr, *b_red = nullptr;
    const double *o_neg = nullptr, *o_chi2 = nullptr, *o_red = nullptr;
};

EdgeCheck* edge_check_create();
void edge_check_destroy(EdgeCheck* p);
int64_t edge_check_bytes(const EdgeCheck* p);
bool edge_check_built(const EdgeCheck* p);
// Builds, once, the arena for Mb bearings and Mo odometry edges: R ([Mo][6], the lower triangles of the
// edges' Omega^-1, uploaded), the per-edge rows, the selection's partial lists and the final lists. 0; -2
// with err (the byte count) when the allocation or the upload fails: nothing is kept then.
int edge_check_build(EdgeCheck* p, int Mb, int Mo, const double* R, std::string& err);
// Enqueues on s the scoring kernel over the kinds in `kind` (bearings, odometry) and the selections of those
// in `select`; after_score is recorded between the two. rows: chi2 and redundancy are written as well.
int edge_check_enqueue(EdgeCheck* p, const EdgeCheckIn& in, const bool kind[2], const bool select[2], bool rows, double gate_bearing,
                       double gate_odom, hipStream_t s, hipEvent_t after_score, EdgeCheckDev* out, std::string& err);

}  // namespace dev
}  // namespace bos
