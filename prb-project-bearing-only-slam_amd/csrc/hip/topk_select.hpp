// The two-stage selection of the k best of a score row, shared by the bearing association
// (hip/associate.hip) and the node matching (hip/match.hip): per row of N scores the kAssocMaxK smallest
// inside the gate, ascending by (score, index) (assoc_less / assoc_inside, host/associate.hpp), and the
// count of all inside it. All arithmetic is comparisons: the listed scores are the row's own bits.
//
// topk_tile_kernel: one workgroup per (tile of kAssocTile entries, row). A thread keeps the kAssocMaxK best
//   of its entries (i = tile start + thread, + 256, ...) in registers and counts those inside the gate; the
//   workgroup merges the lists pairwise through LDS (thread t takes list t + stride, stride halving) and
//   sums the counts the same way. It writes the tile's sorted list and count.
// topk_final_kernel<Epilogue>: one workgroup (one wavefront) per row. Lane t merges the lists of tiles t,
//   t + 64, ... in tile order, the wavefront merges as above; lane j < kAssocMaxK then writes entry j of
//   the final list and hands it to the epilogue, which writes the feature's details of that entry. The
//   epilogue's per-row constants (Epilogue::Row) are evaluated by one thread and read from LDS.
// The order (score, index) is total, so the k smallest are one set whatever the merge order: the fixed
// order above is not what makes the result independent of the grid, it only keeps the kernels free of
// anything that could. Plain grid launches, no atomics, no waiting between workgroups.
//
// LDS: the lists are stored slot-major, [slot][thread], so the threads of a wavefront read and write
// consecutive 8-byte (score) or 4-byte (index) words: no bank is hit twice by one half-wave.
//
// An Epilogue is a trivially copyable struct with
//   struct Row;                                                       the row's constants
//   __device__ Row row(int q) const;                                  evaluated by one thread of the workgroup
//   __device__ void write(const Row&, int q, int slot, int32_t ix, bool listed) const;
//                                                                     ix in [0, N) when listed
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/associate.hpp"

namespace bos {
namespace dev {

constexpr int kTopkTileBlock = 256, kTopkFinalBlock = 64;
static_assert(kAssocTile % kTopkTileBlock == 0, "a tile is a whole number of passes of the workgroup");

struct TopkArgs {
    int N = 0, n_tiles = 0;                // the row's length; its tiles of kAssocTile
    double gate = 0.0;
    const double* score = nullptr;         // [rows][N]
    double* part_score = nullptr;          // [rows][n_tiles][kAssocMaxK]
    int32_t *part_ix = nullptr, *part_count = nullptr;   // the same; [rows][n_tiles]
    int32_t *cand_ix = nullptr, *n_inside = nullptr;     // [rows][kAssocMaxK]; [rows]
    double* cand_score = nullptr;          // [rows][kAssocMaxK]
};

inline int topk_tiles(int N) { return (N + kAssocTile - 1) / kAssocTile; }

namespace {

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

__global__ __launch_bounds__(kTopkTileBlock) void topk_tile_kernel(const TopkArgs g) {
    __shared__ double s_nis[kAssocMaxK * kTopkTileBlock];
    __shared__ int32_t s_l[kAssocMaxK * kTopkTileBlock];
    __shared__ int32_t s_count[kTopkTileBlock];
    const int tile = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
    const double* row = g.score + (int64_t)q * g.N;
    AssocTop top;
    assoc_top_clear(top);
    int count = 0;
    const int l0 = tile * kAssocTile, l1 = min(l0 + kAssocTile, g.N);
    for (int l = l0 + t; l < l1; l += kTopkTileBlock) {
        const double nis = row[l];
        if (assoc_inside(nis, g.gate)) {
            assoc_top_insert(top, nis, l);
            ++count;
        }
    }
    merge_lists<kTopkTileBlock>(top, count, s_nis, s_l, s_count);
    if (t == 0) {
        const int64_t at = (int64_t)q * g.n_tiles + tile;
#pragma unroll
        for (int i = 0; i < kAssocMaxK; ++i) {
            g.part_score[at * kAssocMaxK + i] = top.nis[i];
            g.part_ix[at * kAssocMaxK + i] = top.l[i];
        }
        g.part_count[at] = count;
    }
}

template <class Epilogue> __global__ __launch_bounds__(kTopkFinalBlock) void topk_final_kernel(const TopkArgs g, const Epilogue ep) {
    __shared__ double s_nis[kAssocMaxK * kTopkFinalBlock];
    __shared__ int32_t s_l[kAssocMaxK * kTopkFinalBlock];
    __shared__ int32_t s_count[kTopkFinalBlock];
    __shared__ typename Epilogue::Row s_row;
    const int q = blockIdx.x, t = threadIdx.x;
    if (t == 0) s_row = ep.row(q);
    __syncthreads();
    AssocTop top;
    assoc_top_clear(top);
    int count = 0;
    for (int tile = t; tile < g.n_tiles; tile += kTopkFinalBlock) {
        const int64_t at = (int64_t)q * g.n_tiles + tile;
#pragma unroll
        for (int i = 0; i < kAssocMaxK; ++i) assoc_top_insert(top, g.part_score[at * kAssocMaxK + i], g.part_ix[at * kAssocMaxK + i]);
        count += g.part_count[at];
    }
    merge_lists<kTopkFinalBlock>(top, count, s_nis, s_l, s_count);
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
        const bool listed = l != kAssocNone;   // then 0 <= l < N: only the tile kernel's entries are inserted
        const int64_t at = (int64_t)q * kAssocMaxK + t;
        g.cand_ix[at] = listed ? l : -1;
        g.cand_score[at] = s_nis[t];
        ep.write(s_row, q, t, l, listed);
    }
}

// the two launches on s over `rows` rows, in stream order behind the kernel that wrote g.score
template <class Epilogue> hipError_t topk_select_enqueue(const TopkArgs& g, const Epilogue& ep, int rows, hipStream_t s) {
    topk_tile_kernel<<<dim3(g.n_tiles, rows), kTopkTileBlock, 0, s>>>(g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    topk_final_kernel<Epilogue><<<rows, kTopkFinalBlock, 0, s>>>(g, ep);
    return hipGetLastError();
}

}  // namespace

}  // namespace dev
}  // namespace bos
