// Node matching: the score rows of a chunk of rows of one query node and the k best targets of each
// (host/match.hpp). All arithmetic is fp64. Plain grid launches, no atomics, no waiting between workgroups;
// a launch depends on the one before through stream order.
//
// match_landmark_kernel: one thread per target landmark l of the query's one row: d = l_a - l_l, the lower
//   triangle of C read in place from the node call's [NL][4] slice, d2 into the row; l == a is NaN without
//   evaluation. The query's coordinates are loaded by one thread of the workgroup and read from LDS.
// match_pose_kernel: one thread per (target pose u, measurement): 24 B of state and six of the nine
//   doubles of P at a 72 B stride, plain loads; e, S = P + R and nis into the chunk's row [row][NP]. The
//   row's constants (the query pose's frame with its fp64 cos / sin, z, R's lower triangle) are evaluated
//   or loaded by one thread of the workgroup and read from LDS.
// The selection is the shared two-stage one (topk_select.hpp); its epilogues re-evaluate the details of a
//   listed target with the score kernel's own functions, so a listed detail is the one its score was
//   formed from, in whichever chunk the row ran.
#include "match.hpp"
#include "device_mem.hpp"
#include "topk_select.hpp"

#include <algorithm>

namespace bos {
namespace dev {

namespace {

constexpr int kScoreBlock = 256;

// ---- landmark match ------------------------------------------------------------------------------------
struct MatchLmRow { double ax, ay; };

struct MatchLmEpilogue {
    typedef MatchLmRow Row;
    int a;
    const double *lm, *C;       // master state; C: [NL][4] row-major
    double *cand_d, *cand_C;    // [rows][kMatchMaxK][kMatchDetailStride], [..][kMatchCovStride]
    __device__ Row row(int) const {
        Row r;
        r.ax = lm[2 * a]; r.ay = lm[2 * a + 1];
        return r;
    }
    __device__ void write(const Row& r, int q, int slot, int32_t l, bool listed) const {
        const int64_t at = (int64_t)q * kMatchMaxK + slot;
        double d[2] = {0.0, 0.0}, c[4] = {0.0, 0.0, 0.0, 0.0};
        if (listed) {
            match_landmark_diff(r.ax, r.ay, lm[2 * l], lm[2 * l + 1], d);
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = C[4 * (int64_t)l + i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) cand_d[at * kMatchDetailStride + i] = d[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) cand_C[at * kMatchCovStride + i] = c[i];
    }
};

struct MatchLmArgs {
    int NL;
    MatchLmEpilogue ep;   // the query and what the row reads
    double* score;        // [1][NL]
};

__global__ __launch_bounds__(kScoreBlock) void match_landmark_kernel(const MatchLmArgs g) {
    __shared__ MatchLmRow rs;
    if (threadIdx.x == 0) rs = g.ep.row(0);
    __syncthreads();
    const MatchLmRow r = rs;
    const int l = blockIdx.x * kScoreBlock + threadIdx.x;
    if (l >= g.NL) return;
    double d2 = match_nan();
    if (l != g.ep.a) {
        double d[2];
        match_landmark_diff(r.ax, r.ay, g.ep.lm[2 * l], g.ep.lm[2 * l + 1], d);
        const double* c = g.ep.C + 4 * (int64_t)l;
        d2 = match_landmark_d2(d, c[0], c[2], c[3]);
    }
    g.score[l] = d2;
}

// ---- pose match ----------------------------------------------------------------------------------------
struct MatchPoseRow {
    MatchFrame f;
    double z[3], R[6];
};

struct MatchPoseEpilogue {
    typedef MatchPoseRow Row;
    int a;
    const double *pose, *P;     // master state; P: [NP][9] row-major
    const double* zr;           // [rows][kMatchRowDoubles]
    double *cand_e, *cand_S;    // [rows][kMatchMaxK][kMatchDetailStride], [..][kMatchCovStride]
    __device__ Row row(int q) const {
        Row r;
        r.f = match_frame(pose, a);
        const double* v = zr + (int64_t)q * kMatchRowDoubles;
#pragma unroll
        for (int i = 0; i < 3; ++i) r.z[i] = v[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) r.R[i] = v[3 + i];
        return r;
    }
    // e and the lower triangle of S of target u
    __device__ void evaluate(const Row& r, int u, double e[3], double S[6]) const {
        match_pose_error(r.f, pose[3 * u], pose[3 * u + 1], pose[3 * u + 2], r.z, e);
        match_pose_S(P + 9 * (int64_t)u, r.R, S);
    }
    __device__ void write(const Row& r, int q, int slot, int32_t u, bool listed) const {
        const int64_t at = (int64_t)q * kMatchMaxK + slot;
        double e[3] = {0.0, 0.0, 0.0}, full[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (listed) {
            double S[6];
            evaluate(r, u, e, S);
            match_mirror(S, full);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) cand_e[at * kMatchDetailStride + i] = e[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) cand_S[at * kMatchCovStride + i] = full[i];
    }
};

struct MatchPoseArgs {
    int NP;
    MatchPoseEpilogue ep;
    double* score;   // [rows][NP]
};

__global__ __launch_bounds__(kScoreBlock) void match_pose_kernel(const MatchPoseArgs g) {
    __shared__ MatchPoseRow rs;
    const int q = blockIdx.y;
    if (threadIdx.x == 0) rs = g.ep.row(q);
    __syncthreads();
    const int u = blockIdx.x * kScoreBlock + threadIdx.x;
    if (u >= g.NP) return;
    double e[3], S[6];
    g.ep.evaluate(rs, u, e, S);
    g.score[(int64_t)q * g.NP + u] = match_pose_nis(e, S);
}

}  // namespace

struct Match {
    DeviceMem mem;   // the arena alone
    char* arena = nullptr;
    int N = 0, rows = 0;
    double *zr = nullptr, *score = nullptr, *part_score = nullptr, *cand_score = nullptr, *cand_detail = nullptr, *cand_cov = nullptr;
    int32_t *part_ix = nullptr, *part_count = nullptr, *cand_ix = nullptr, *n_inside = nullptr;
};

Match* match_create() { return new Match(); }

void match_destroy(Match* p) { delete p; }

int64_t match_bytes(const Match* p) { return p ? (int64_t)p->mem.bytes() : 0; }

int match_budget_rows(int N) {
    const int64_t rows = kMatchRowBudgetBytes / ((int64_t)std::max(N, 1) * (int64_t)sizeof(double));
    return (int)std::min<int64_t>(std::max<int64_t>(rows, 1), kMatchMaxRows);
}

int match_reserve(Match* p, int N, int rows, std::string& err) {
    if (p->arena && p->N >= N && p->rows >= rows) return 0;
    N = std::max(N, p->N);
    rows = std::max(rows, p->rows);
    // one arena: [rows' constants | score rows | the tiles' lists and counts | the final lists, details and counts]
    const size_t R = (size_t)rows, tiles = (size_t)topk_tiles(N);
    p->mem.release(p->arena);
    p->arena = nullptr;
    p->rows = 0;
    p->N = 0;
    Arena ar(true);
    ar.reserve(&p->zr, R * kMatchRowDoubles);
    ar.reserve(&p->score, R * (size_t)N);
    ar.reserve(&p->part_score, R * tiles * kMatchMaxK);
    ar.reserve(&p->part_ix, R * tiles * kMatchMaxK);
    ar.reserve(&p->part_count, R * tiles);
    ar.reserve(&p->cand_ix, R * kMatchMaxK);
    ar.reserve(&p->cand_score, R * kMatchMaxK);
    ar.reserve(&p->cand_detail, R * kMatchMaxK * kMatchDetailStride);
    ar.reserve(&p->cand_cov, R * kMatchMaxK * kMatchCovStride);
    ar.reserve(&p->n_inside, R);
    if (!ar.commit(p->mem, &p->arena)) {
        err = "node matching: device allocation of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    p->N = N; p->rows = rows;
    return 0;
}

namespace {

// what both enqueues share behind their score kernel: the selection over `rows` rows of N scores
template <class Epilogue>
hipError_t select_rows(Match* p, int N, int rows, double gate, const Epilogue& ep, hipStream_t s) {
    TopkArgs t;
    t.N = N; t.n_tiles = topk_tiles(N); t.gate = gate; t.score = p->score;
    t.part_score = p->part_score; t.part_ix = p->part_ix; t.part_count = p->part_count;
    t.cand_ix = p->cand_ix; t.n_inside = p->n_inside; t.cand_score = p->cand_score;
    return topk_select_enqueue(t, ep, rows, s);
}

void results(const Match* p, bool select, MatchDev* out) {
    out->score = p->score;
    out->cand_ix = select ? p->cand_ix : nullptr; out->n_inside = select ? p->n_inside : nullptr;
    out->cand_score = select ? p->cand_score : nullptr; out->cand_detail = select ? p->cand_detail : nullptr;
    out->cand_cov = select ? p->cand_cov : nullptr;
}

}  // namespace

int match_landmark_enqueue(Match* p, int NL, int a, double gate, bool select, const double* C, const double* lm, hipStream_t s,
                           hipEvent_t before_score, hipEvent_t after_score, MatchDev* out, std::string& err) {
    if (!p->arena || p->rows < 1 || NL < 1 || NL > p->N || a < 0 || a >= NL || !C || !lm) {
        err = "bos_match_landmarks: the row does not fit the buffers";
        return -1;
    }
    MatchLmArgs g;
    g.NL = NL; g.score = p->score;
    g.ep.a = a; g.ep.lm = lm; g.ep.C = C; g.ep.cand_d = p->cand_detail; g.ep.cand_C = p->cand_cov;
    hipError_t e = before_score ? hipEventRecord(before_score, s) : hipSuccess;
    if (e == hipSuccess) {
        match_landmark_kernel<<<dim3((NL + kScoreBlock - 1) / kScoreBlock, 1), kScoreBlock, 0, s>>>(g);
        e = hipGetLastError();
    }
    if (e == hipSuccess && after_score) e = hipEventRecord(after_score, s);
    if (e == hipSuccess && select) e = select_rows(p, NL, 1, gate, g.ep, s);
    if (e != hipSuccess) { err = std::string("bos_match_landmarks: launch: ") + hipGetErrorString(e); return -2; }
    results(p, select, out);
    return 0;
}

int match_pose_enqueue(Match* p, int NP, int a, int rows, const double* zr, double gate, bool select, const double* P,
                       const double* pose, hipStream_t s, hipEvent_t before_score, hipEvent_t after_score, MatchDev* out,
                       std::string& err) {
    if (!p->arena || rows < 1 || rows > p->rows || rows > kMatchMaxRows || NP < 1 || NP > p->N || a < 0 || a >= NP || !P || !pose || !zr) {
        err = "bos_match_poses: the chunk does not fit the buffers";
        return -1;
    }
    if (!dm_copy(p->zr, zr, (size_t)rows * kMatchRowDoubles * sizeof(double))) {
        err = "bos_match_poses: upload of the chunk's measurements failed";
        return -2;
    }
    MatchPoseArgs g;
    g.NP = NP; g.score = p->score;
    g.ep.a = a; g.ep.pose = pose; g.ep.P = P; g.ep.zr = p->zr; g.ep.cand_e = p->cand_detail; g.ep.cand_S = p->cand_cov;
    hipError_t e = before_score ? hipEventRecord(before_score, s) : hipSuccess;
    if (e == hipSuccess) {
        match_pose_kernel<<<dim3((NP + kScoreBlock - 1) / kScoreBlock, rows), kScoreBlock, 0, s>>>(g);
        e = hipGetLastError();
    }
    if (e == hipSuccess && after_score) e = hipEventRecord(after_score, s);
    if (e == hipSuccess && select) e = select_rows(p, NP, rows, gate, g.ep, s);
    if (e != hipSuccess) { err = std::string("bos_match_poses: launch: ") + hipGetErrorString(e); return -2; }
    results(p, select, out);
    return 0;
}

}  // namespace dev
}  // namespace bos
