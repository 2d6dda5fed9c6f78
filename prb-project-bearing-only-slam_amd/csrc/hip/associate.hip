// Bearing association: the NIS rows of a chunk of bearings of one pose and the k best landmarks of each
// (host/associate.hpp). All arithmetic is fp64. Plain grid launches, no atomics, no waiting between
// workgroups; a launch depends on the one before through stream order.
//
// assoc_nis_kernel: one thread per (landmark, bearing): e, S and nis into the chunk's row [bearing][NL]. The
//   pose's frame (px, py, cos, sin) is evaluated by one thread of the workgroup and read from LDS by all; the
//   selection's second stage evaluates the same expression, so a listed e has the bits the row's nis was
//   formed from, whatever chunk the bearing falls in.
// assoc_select_tile_kernel: one workgroup per (tile of kAssocTile landmarks, bearing). A thread keeps the
//   kAssocMaxK best of its landmarks (l = tile start + thread, + 256, ...) in registers and counts those
//   inside the gate; the workgroup merges the lists pairwise through LDS (thread t takes list t + stride,
//   stride halving) and sums the counts the same way. It writes the tile's sorted list and count.
// assoc_select_final_kernel: one workgroup (one wavefront) per bearing. Lane t merges the lists of tiles t,
//   t + 64, ... in tile order, the wavefront merges as above; lane j < kAssocMaxK then writes entry j of
//   the final list with the e and S of its landmark.
// The order (nis, stix) is total, so the k smallest are one set whatever the merge order: the fixed order
// above is not what makes the result independent of the grid, it only keeps the kernels free of anything
// that could.
//
// LDS: the lists are stored slot-major, [slot][thread], so the threads of a wavefront read and write
// consecutive 8-byte (nis) or 4-byte (stix) words: no bank is hit twice by one half-wave.
#include "associate.hpp"
#include "device_mem.hpp"

#include <algorithm>

namespace bos {
namespace dev {

namespace {

constexpr int kNisBlock = 256, kTileBlock = 256, kFinalBlock = 64;
static_assert(kAssocTile % kTileBlock == 0, "a tile is a whole number of passes of the workgroup");

struct AssocArgs {
    int NL, a, n_tiles;
    double gate;
    const double *pose, *lm, *var;   // master state; var: [NL][4], entry 0
    const double *z, *omega;         // [rows]
    double* nis;                     // [rows][NL]
    double* part_nis;                // [rows][n_tiles][kAssocMaxK]
    int32_t *part_l, *part_count;    // the same; [rows][n_tiles]
    int32_t *cand_l, *n_inside;      // [rows][kAssocMaxK]; [rows]
    double *cand_nis, *cand_e, *cand_S;
};

// the frame of pose a, evaluated once per workgroup
__device__ __forceinline__ AssocFrame frame_once(const AssocArgs& g, AssocFrame* shared) {
    if (threadIdx.x == 0) *shared = assoc_frame(g.pose, g.a);
    __syncthreads();
    return *shared;
}

__global__ __launch_bounds__(kNisBlock) void assoc_nis_kernel(const AssocArgs g) {
    __shared__ AssocFrame fs;
    const AssocFrame f = frame_once(g, &fs);
    const int l = blockIdx.x * kNisBlock + threadIdx.x, q = blockIdx.y;
    if (l >= g.NL) return;
    const double e = assoc_innovation(f, g.lm[2 * l], g.lm[2 * l + 1], g.z[q]);
    const double S = assoc_innovation_var(g.var[4 * (int64_t)l], g.omega[q]);
    g.nis[(int64_t)q * g.NL + l] = assoc_nis(e, S);
}

// The workgroup's T lists to list 0, its T counts to count 0: thread t < stride takes list t + stride
template <int T> __device__ __forceinline__ void merge_lists(AssocTop& top, int& count, double* s_nis, int32_t* s_l, int32_t* s_count) {
    const int t = threadIdx.x;
    for (int stride = T / 2; stride > 0; stride >>= 1) {
        if (t >= stride && t < 2 * stride) {
#pragma unroll
            for (int i = 0; i < kAssocMaxK; ++i) {
                s_nis[i * T + t] = top.nis[i];
                s_l[i * T + t] = top.l[i];
            }
            s_count[t] = count;
        }
        __syncthreads();
        if (t < stride) {
#pragma unroll
            for (int i = 0; i < kAssocMaxK; ++i) assoc_top_insert(top, s_nis[i * T + t + stride], s_l[i * T + t + stride]);
            count += s_count[t + stride];
        }
    }
}

__global__ __launch_bounds__(kTileBlock) void assoc_select_tile_kernel(const AssocArgs g) {
    __shared__ double s_nis[kAssocMaxK * kTileBlock];
    __shared__ int32_t s_l[kAssocMaxK * kTileBlock];
    __shared__ int32_t s_count[kTileBlock];
    const int tile = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
    const double* row = g.nis + (int64_t)q * g.NL;
    AssocTop top;
    assoc_top_clear(top);
    int count = 0;
    const int l0 = tile * kAssocTile, l1 = min(l0 + kAssocTile, g.NL);
    for (int l = l0 + t; l < l1; l += kTileBlock) {
        const double nis = row[l];
        if (assoc_inside(nis, g.gate)) {
            assoc_top_insert(top, nis, l);
            ++count;
        }
    }
    merge_lists<kTileBlock>(top, count, s_nis, s_l, s_count);
    if (t == 0) {
        const int64_t at = (int64_t)q * g.n_tiles + tile;
#pragma unroll
        for (int i = 0; i < kAssocMaxK; ++i) {
            g.part_nis[at * kAssocMaxK + i] = top.nis[i];
            g.part_l[at * kAssocMaxK + i] = top.l[i];
        }
        g.part_count[at] = count;
    }
}

__global__ __launch_bounds__(kFinalBlock) void assoc_select_final_kernel(const AssocArgs g) {
    __shared__ double s_nis[kAssocMaxK * kFinalBlock];
    __shared__ int32_t s_l[kAssocMaxK * kFinalBlock];
    __shared__ int32_t s_count[kFinalBlock];
    __shared__ AssocFrame fs;
    const AssocFrame f = frame_once(g, &fs);
    const int q = blockIdx.x, t = threadIdx.x;
    AssocTop top;
    assoc_top_clear(top);
    int count = 0;
    for (int tile = t; tile < g.n_tiles; tile += kFinalBlock) {
        const int64_t at = (int64_t)q * g.n_tiles + tile;
#pragma unroll
        for (int i = 0; i < kAssocMaxK; ++i) assoc_top_insert(top, g.part_nis[at * kAssocMaxK + i], g.part_l[at * kAssocMaxK + i]);
        count += g.part_count[at];
    }
    merge_lists<kFinalBlock>(top, count, s_nis, s_l, s_count);
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < kAssocMaxK; ++i) {
            s_nis[i] = top.nis[i];
            s_l[i] = top.l[i];
        }
        g.n_inside[q] = count;
    }
    __syncthreads();
    if (t < kAssocMaxK) {
        const int32_t l = s_l[t];
        const bool listed = l != kAssocNone;   // then 0 <= l < NL: only the tile kernel's landmarks are inserted
        const int64_t at = (int64_t)q * kAssocMaxK + t;
        g.cand_l[at] = listed ? l : -1;
        g.cand_nis[at] = s_nis[t];
        g.cand_e[at] = listed ? assoc_innovation(f, g.lm[2 * l], g.lm[2 * l + 1], g.z[q]) : 0.0;
        g.cand_S[at] = listed ? assoc_innovation_var(g.var[4 * (int64_t)l], g.omega[q]) : 0.0;
    }
}

}  // namespace

struct Associate {
    DeviceMem mem;   // the arena alone
    char* arena = nullptr;
    int NL = 0, rows = 0, n_tiles = 0;
    double *z = nullptr, *omega = nullptr, *nis = nullptr, *part_nis = nullptr, *cand_nis = nullptr, *cand_e = nullptr, *cand_S = nullptr;
    int32_t *part_l = nullptr, *part_count = nullptr, *cand_l = nullptr, *n_inside = nullptr;
};

Associate* associate_create() { return new Associate(); }

void associate_destroy(Associate* p) { delete p; }

int64_t associate_bytes(const Associate* p) { return p ? (int64_t)p->mem.bytes() : 0; }

int associate_budget_rows(int NL) {
    const int64_t rows = kAssocRowBudgetBytes / ((int64_t)std::max(NL, 1) * (int64_t)sizeof(double));
    return (int)std::min<int64_t>(std::max<int64_t>(rows, 1), kAssocMaxRows);
}

int associate_reserve(Associate* p, int NL, int rows, std::string& err) {
    if (p->arena && p->NL == NL && p->rows >= rows) return 0;
    // one arena: [z | omega | NIS rows | the tiles' lists and counts | the final lists and counts]
    const size_t R = (size_t)rows, tiles = ((size_t)NL + kAssocTile - 1) / kAssocTile;
    p->mem.release(p->arena);
    p->arena = nullptr;
    p->rows = 0;
    Arena ar(true);
    ar.reserve(&p->z, R);
    ar.reserve(&p->omega, R);
    ar.reserve(&p->nis, R * (size_t)NL);
    ar.reserve(&p->part_nis, R * tiles * kAssocMaxK);
    ar.reserve(&p->part_l, R * tiles * kAssocMaxK);
    ar.reserve(&p->part_count, R * tiles);
    ar.reserve(&p->cand_l, R * kAssocMaxK);
    ar.reserve(&p->cand_nis, R * kAssocMaxK);
    ar.reserve(&p->cand_e, R * kAssocMaxK);
    ar.reserve(&p->cand_S, R * kAssocMaxK);
    ar.reserve(&p->n_inside, R);
    if (!ar.commit(p->mem, &p->arena)) {
        err = "bos_associate_bearings: device allocation of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    p->NL = NL; p->rows = rows; p->n_tiles = (int)tiles;
    return 0;
}

int associate_enqueue(Associate* p, int a, int rows, const double* z, const double* omega, double gate, bool select,
                      const double* var, const double* pose, const double* lm, hipStream_t s, hipEvent_t before_nis,
                      hipEvent_t after_nis, AssociateDev* out, std::string& err) {
    if (!p->arena || rows < 1 || rows > p->rows || p->NL < 1 || !var) { err = "bos_associate_bearings: the chunk does not fit the buffers"; return -1; }
    if (!dm_copy(p->z, z, (size_t)rows * sizeof(double)) || !dm_copy(p->omega, omega, (size_t)rows * sizeof(double))) {
        err = "bos_associate_bearings: upload of the chunk's bearings failed";
        return -2;
    }
    AssocArgs g;
    g.NL = p->NL; g.a = a; g.n_tiles = p->n_tiles; g.gate = gate;
    g.pose = pose; g.lm = lm; g.var = var; g.z = p->z; g.omega = p->omega; g.nis = p->nis;
    g.part_nis = p->part_nis; g.part_l = p->part_l; g.part_count = p->part_count;
    g.cand_l = p->cand_l; g.n_inside = p->n_inside; g.cand_nis = p->cand_nis; g.cand_e = p->cand_e; g.cand_S = p->cand_S;
    hipError_t e = before_nis ? hipEventRecord(before_nis, s) : hipSuccess;
    if (e == hipSuccess) {
        assoc_nis_kernel<<<dim3((p->NL + kNisBlock - 1) / kNisBlock, rows), kNisBlock, 0, s>>>(g);
        e = hipGetLastError();
    }
    if (e == hipSuccess && after_nis) e = hipEventRecord(after_nis, s);
    if (e == hipSuccess && select) {
        assoc_select_tile_kernel<<<dim3(p->n_tiles, rows), kTileBlock, 0, s>>>(g);
        e = hipGetLastError();
        if (e == hipSuccess) {
            assoc_select_final_kernel<<<rows, kFinalBlock, 0, s>>>(g);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) { err = std::string("bos_associate_bearings: launch: ") + hipGetErrorString(e); return -2; }
    out->nis = p->nis;
    out->cand_landmark = select ? p->cand_l : nullptr; out->n_inside = select ? p->n_inside : nullptr;
    out->cand_nis = select ? p->cand_nis : nullptr; out->cand_innovation = select ? p->cand_e : nullptr;
    out->cand_var = select ? p->cand_S : nullptr;
    return 0;
}

}  // namespace dev
}  // namespace bos
