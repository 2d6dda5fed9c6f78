// Bearing association: the NIS rows of a chunk of bearings of one pose and the k best landmarks of each
// (host/associate.hpp). All arithmetic is fp64. Plain grid launches, no atomics, no waiting between
// workgroups; a launch depends on the one before through stream order.
//
// assoc_nis_kernel: one thread per (landmark, bearing): e, S and nis into the chunk's row [bearing][NL]. The
//   pose's frame (px, py, cos, sin) is evaluated by one thread of the workgroup and read from LDS by all.
// The selection is the shared two-stage one (topk_select.hpp) over rows of NL scores; its epilogue
//   (AssocEpilogue) evaluates e and S of a listed landmark with the NIS kernel's own expressions, so a
//   listed e has the bits the row's nis was formed from, whatever chunk the bearing falls in.
#include "associate.hpp"
#include "device_mem.hpp"
#include "topk_select.hpp"

#include <algorithm>

namespace bos {
namespace dev {

namespace {

constexpr int kNisBlock = 256;

struct AssocArgs {
    int NL, a;
    const double *pose, *lm, *var;   // master state; var: [NL][4], entry 0
    const double *z, *omega;         // [rows]
    double* nis;                     // [rows][NL]
};

__global__ __launch_bounds__(kNisBlock) void assoc_nis_kernel(const AssocArgs g) {
    __shared__ AssocFrame fs;
    if (threadIdx.x == 0) fs = assoc_frame(g.pose, g.a);   // the frame of pose a, evaluated once per workgroup
    __syncthreads();
    const AssocFrame f = fs;
    const int l = blockIdx.x * kNisBlock + threadIdx.x, q = blockIdx.y;
    if (l >= g.NL) return;
    const double e = assoc_innovation(f, g.lm[2 * l], g.lm[2 * l + 1], g.z[q]);
    const double S = assoc_innovation_var(g.var[4 * (int64_t)l], g.omega[q]);
    g.nis[(int64_t)q * g.NL + l] = assoc_nis(e, S);
}

// the details of a listed landmark: the NIS kernel's e and S
struct AssocEpilogue {
    typedef AssocFrame Row;
    int a;
    const double *pose, *lm, *var, *z, *omega;
    double *cand_e, *cand_S;   // [rows][kAssocMaxK]
    __device__ Row row(int) const { return assoc_frame(pose, a); }
    __device__ void write(const Row& f, int q, int slot, int32_t l, bool listed) const {
        const int64_t at = (int64_t)q * kAssocMaxK + slot;
        cand_e[at] = listed ? assoc_innovation(f, lm[2 * l], lm[2 * l + 1], z[q]) : 0.0;
        cand_S[at] = listed ? assoc_innovation_var(var[4 * (int64_t)l], omega[q]) : 0.0;
    }
};

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
    const size_t R = (size_t)rows, tiles = (size_t)topk_tiles(NL);
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
    g.NL = p->NL; g.a = a;
    g.pose = pose; g.lm = lm; g.var = var; g.z = p->z; g.omega = p->omega; g.nis = p->nis;
    hipError_t e = before_nis ? hipEventRecord(before_nis, s) : hipSuccess;
    if (e == hipSuccess) {
        assoc_nis_kernel<<<dim3((p->NL + kNisBlock - 1) / kNisBlock, rows), kNisBlock, 0, s>>>(g);
        e = hipGetLastError();
    }
    if (e == hipSuccess && after_nis) e = hipEventRecord(after_nis, s);
    if (e == hipSuccess && select) {
        TopkArgs t;
        t.N = p->NL; t.n_tiles = p->n_tiles; t.gate = gate; t.score = p->nis;
        t.part_score = p->part_nis; t.part_ix = p->part_l; t.part_count = p->part_count;
        t.cand_ix = p->cand_l; t.n_inside = p->n_inside; t.cand_score = p->cand_nis;
        AssocEpilogue ep;
        ep.a = a; ep.pose = pose; ep.lm = lm; ep.var = var; ep.z = p->z; ep.omega = p->omega;
        ep.cand_e = p->cand_e; ep.cand_S = p->cand_S;
        e = topk_select_enqueue(t, ep, rows, s);
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
