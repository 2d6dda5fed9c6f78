// Node matching on the device (hip/match.hip): see host/match.hpp for the quantities. Per chunk of rows of
// one query node, in plain stream order after the node_cov_enqueue whose projected slice they read in
// place: the score kernel (one thread per target and row) and the shared selection's two stages
// (hip/topk_select.hpp). A landmark query is one row; the measurements taken from one pose are the rows
// of a pose query. No kernel communicates between workgroups, none uses an atomic, and the list a row
// gets is the unique minimum of a total order: it depends on no grid shape.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../host/match.hpp"

namespace bos {
namespace dev {

struct Match;   // the feature's device buffers; owned by the solver handle

constexpr int64_t kMatchRowBudgetBytes = 64ll << 20;   // score rows of one chunk
constexpr int kMatchMaxRows = 4096;                    // rows of one chunk at most (a grid dimension)
constexpr int kMatchRowDoubles = 9;                    // a pose row's upload: z[3], R's lower triangle[6]

// device results of the last enqueued chunk: [rows][kMatchMaxK] lists, [rows] counts, [rows][N] scores;
// cand_detail [rows][kMatchMaxK][3] (a landmark row: d in the first 2), cand_cov [rows][kMatchMaxK][9]
// (a landmark row: C in the first 4)
struct MatchDev {
    const int32_t *cand_ix = nullptr, *n_inside = nullptr;
    const double *cand_score = nullptr, *cand_detail = nullptr, *cand_cov = nullptr, *score = nullptr;
};
constexpr int kMatchDetailStride = 3, kMatchCovStride = 9;

Match* match_create();
void match_destroy(Match* p);
int64_t match_bytes(const Match* p);
// rows one chunk may hold for rows of N scores: the byte budget's, at least 1, at most kMatchMaxRows
int match_budget_rows(int N);
// Room for chunks of `rows` rows of at most N scores (kept when it is already there). 0; -2 with err (the
// byte count) when the allocation fails: nothing is kept then.
int match_reserve(Match* p, int N, int rows, std::string& err);
// Enqueues the one row of landmark a on s: C = the node call's projected_landmark slice of node NP + a
// ([NL][4], device), lm the fp64 master state. before_score is recorded in front of the score kernel,
// after_score between that kernel and the selection; select false: the row alone.
int match_landmark_enqueue(Match* p, int NL, int a, double gate, bool select, const double* C, const double* lm, hipStream_t s,
                           hipEvent_t before_score, hipEvent_t after_score, MatchDev* out, std::string& err);
// Enqueues one chunk of pose a's measurements on s: zr = [rows][kMatchRowDoubles] host array, copied before
// the call returns; P = the node call's projected_pose slice of node a ([NP][9], device), pose the fp64
// master state. The events as above (before_score behind the upload).
int match_pose_enqueue(Match* p, int NP, int a, int rows, const double* zr, double gate, bool select, const double* P,
                       const double* pose, hipStream_t s, hipEvent_t before_score, hipEvent_t after_score, MatchDev* out,
                       std::string& err);

}  // namespace dev
}  // namespace bos
