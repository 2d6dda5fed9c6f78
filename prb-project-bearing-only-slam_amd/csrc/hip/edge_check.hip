// Edge consistency: see edge_check.hpp. All arithmetic is fp64 and host/edge_check.hpp's, shared with the
// host twin. Plain grid launches, no atomics, no waiting between workgroups; a launch depends on the one
// before through stream order.
//
// edge_check_kernel: one thread per edge, bearings then odometry, 64-bit index arithmetic. A bearing reads 24 B
//   of pose, 16 B of landmark, z, its weight and its bearing_var in place; an odometry edge 48 B of poses, z,
//   Omega's upper triangle, R's lower triangle and the nine doubles of its odom_cov in place. Each writes the
//   negated score (-w2: the selection below lists the smallest), e and T (16 B / 96 B per edge: the epilogue
//   copies them instead of evaluating the edge again) and, where asked for, chi2 and the redundancy number.
//   Every loop is unrolled over constant bounds: the 3 x 3 LDL^T and the edge's blocks stay in registers.
// The selection is the shared two-stage one (topk_select.hpp), rows = 1 and N = M_b or M_o: the k smallest of
//   -w2 inside the gate -gate, ascending by (score, index), are the k largest w2 at or above the gate,
//   descending, equal w2 to the lower edge first. Its epilogues copy e and T of a listed edge and write +w2.
#include "edge_check.hpp"
#include "device_mem.hpp"
#include "topk_select.hpp"

namespace bos {
namespace dev {

namespace {

struct EdgeCheckArgs {
    EdgeCheckIn in;
    const double* R;   // [Mo][6]
    // a kind whose b_neg / o_neg is null is not evaluated; chi2 and red may be null
    double *b_neg, *b_chi2, *b_red, *b_e, *b_T;   // [Mb] each
    double *o_neg, *o_chi2, *o_red, *o_e, *o_T;   // [Mo]; o_e [Mo][3], o_T [Mo][9]
};

__device__ __forceinline__ void check_bearing(const EdgeCheckArgs& g, int64_t i) {
    const EdgeCheckIn& in = g.in;
    const int64_t p = in.b_pose[i], l = in.b_lm[i];
    const double th = in.pose[3 * p + 2];
    double gx, gy;
    const double e = bos::bearing_error<double>(in.pose[3 * p], in.pose[3 * p + 1], cos(th), sin(th), in.lm[2 * l], in.lm[2 * l + 1],
                                                in.b_z[i], gx, gy);
    const EdgeCheckBearing o = edge_check_bearing(e, in.b_w ? in.b_w[i] : 1.0, in.bearing_var[i]);
    g.b_neg[i] = -o.w2;
    g.b_e[i] = o.e;
    g.b_T[i] = o.T;
    if (g.b_chi2) g.b_chi2[i] = o.chi2;
    if (g.b_red) g.b_red[i] = o.redundancy;
}

__device__ __forceinline__ void check_odometry(const EdgeCheckArgs& g, int64_t k) {
    const EdgeCheckIn& in = g.in;
    const int64_t a = in.o_src[k], d = in.o_dst[k];
    const double* xs = in.pose + 3 * a;
    const double* xd = in.pose + 3 * d;
    const double* z = in.o_z + 3 * k;
    double e[3], J[18], u[6], R[6], P[9];
    bos::odometry_error_jacobian<double>(xs[0], xs[1], xs[2], cos(xs[2]), sin(xs[2]), xd[0], xd[1], xd[2], z[0], z[1], z[2], e, J);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        u[i] = in.o_om[6 * k + i];
        R[i] = g.R[6 * k + i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) P[i] = in.odom_cov[9 * k + i];
    EdgeCheckOdom o;
    edge_check_odometry(e, u, R, P, a == d, o);
    g.o_neg[k] = -o.w2;
#pragma unroll
    for (int i = 0; i < 3; ++i) g.o_e[3 * k + i] = o.e[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) g.o_T[9 * k + i] = o.T[i];
    if (g.o_chi2) g.o_chi2[k] = o.chi2;
    if (g.o_red) g.o_red[k] = o.redundancy;
}

__global__ __launch_bounds__(kEdgeCheckBlock) void edge_check_kernel(const EdgeCheckArgs g) {
    const int64_t i = (int64_t)blockIdx.x * kEdgeCheckBlock + threadIdx.x;
    if (i < g.in.Mb) {
        if (g.b_neg) check_bearing(g, i);
    } else if (i < (int64_t)g.in.Mb + g.in.Mo) {
        if (g.o_neg) check_odometry(g, i - g.in.Mb);
    }
}

// the selection's epilogue of one kind: +w2, e (D doubles) and T (D * D) of a listed edge, the padding otherwise
template <int D> struct EdgeCheckEpilogue {
    struct Row { int32_t none; };
    const double *neg, *e, *T;   // the kind's rows
    EdgeCheckLists* out;
    __device__ Row row(int) const { return Row{0}; }
    __device__ void write(const Row&, int, int slot, int32_t ix, bool listed) const {
        out->w2[slot] = listed ? -neg[ix] : -HUGE_VAL;
#pragma unroll
        for (int i = 0; i < 3; ++i) out->e[slot][i] = listed && i < D ? e[(int64_t)D * ix + i] : 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) out->T[slot][i] = listed && i < D * D ? T[(int64_t)D * D * ix + i] : 0.0;
    }
};

}  // namespace

struct EdgeCheck {
    DeviceMem mem;   // the arena alone
    char* arena = nullptr;
    int Mb = 0, Mo = 0;
    double* R = nullptr;
    double *b_neg = nullptr, *b_chi2 = nullptr, *b_red = nullptr, *b_e = nullptr, *b_T = nullptr;
    double *o_neg = nullptr, *o_chi2 = nullptr, *o_red = nullptr, *o_e = nullptr, *o_T = nullptr;
    double* part_score[2] = {nullptr, nullptr};
    int32_t *part_ix[2] = {nullptr, nullptr}, *part_count[2] = {nullptr, nullptr};
    EdgeCheckLists* lists = nullptr;   // [2]
};

EdgeCheck* edge_check_create() { return new EdgeCheck(); }

void edge_check_destroy(EdgeCheck* p) { delete p; }

int64_t edge_check_bytes(const EdgeCheck* p) { return p ? (int64_t)p->mem.bytes() : 0; }

bool edge_check_built(const EdgeCheck* p) { return p && p->arena; }

int edge_check_build(EdgeCheck* p, int Mb, int Mo, const double* R, std::string& err) {
    if (p->arena) return 0;
    // one arena: [R | the bearings' rows | the odometry's rows | the tiles' lists and counts | the final lists]
    const size_t B = (size_t)Mb, O = (size_t)Mo;
    const size_t tiles[2] = {(size_t)topk_tiles(Mb), (size_t)topk_tiles(Mo)};
    Arena ar(true);
    ar.add(&p->R, R, 6 * O);
    ar.reserve(&p->b_neg, B); ar.reserve(&p->b_chi2, B); ar.reserve(&p->b_red, B); ar.reserve(&p->b_e, B); ar.reserve(&p->b_T, B);
    ar.reserve(&p->o_neg, O); ar.reserve(&p->o_chi2, O); ar.reserve(&p->o_red, O); ar.reserve(&p->o_e, 3 * O); ar.reserve(&p->o_T, 9 * O);
    for (int v = 0; v < 2; ++v) {
        ar.reserve(&p->part_score[v], tiles[v] * kAssocMaxK);
        ar.reserve(&p->part_ix[v], tiles[v] * kAssocMaxK);
        ar.reserve(&p->part_count[v], tiles[v]);
    }
    ar.reserve(&p->lists, 2);
    DeviceMem mem;
    if (!ar.commit(mem, &p->arena)) {
        err = "bos_edge_consistency: device allocation or upload of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    p->mem = std::move(mem);
    p->Mb = Mb; p->Mo = Mo;
    return 0;
}

namespace {

template <int D>
hipError_t select_kind(EdgeCheck* p, int v, int N, double gate, const double* neg, const double* e, const double* T, hipStream_t s) {
    EdgeCheckLists* out = p->lists + v;
    TopkArgs t;
    t.N = N; t.n_tiles = topk_tiles(N); t.gate = -gate; t.score = neg;
    t.part_score = p->part_score[v]; t.part_ix = p->part_ix[v]; t.part_count = p->part_count[v];
    t.cand_ix = out->ix; t.n_inside = &out->n_over; t.cand_score = out->score;
    EdgeCheckEpilogue<D> ep;
    ep.neg = neg; ep.e = e; ep.T = T; ep.out = out;
    return topk_select_enqueue(t, ep, 1, s);
}

}  // namespace

int edge_check_enqueue(EdgeCheck* p, const EdgeCheckIn& in, const bool kind[2], const bool select[2], bool rows, double gate_bearing,
                       double gate_odom, hipStream_t s, hipEvent_t after_score, EdgeCheckDev* out, std::string& err) {
    const bool kb = kind[0] && in.Mb > 0, ko = kind[1] && in.Mo > 0;
    if (!p->arena || in.Mb != p->Mb || in.Mo != p->Mo || !in.pose || (kb && (!in.lm || !in.b_pose || !in.b_lm || !in.b_z || !in.bearing_var)) ||
        (ko && (!in.o_src || !in.o_dst || !in.o_z || !in.o_om || !in.odom_cov))) {
        err = "bos_edge_consistency: the edges do not fit the buffers";
        return -1;
    }
    EdgeCheckArgs g;
    g.in = in; g.R = p->R;
    g.b_neg = kb ? p->b_neg : nullptr; g.b_chi2 = kb && rows ? p->b_chi2 : nullptr; g.b_red = kb && rows ? p->b_red : nullptr;
    g.b_e = p->b_e; g.b_T = p->b_T;
    g.o_neg = ko ? p->o_neg : nullptr; g.o_chi2 = ko && rows ? p->o_chi2 : nullptr; g.o_red = ko && rows ? p->o_red : nullptr;
    g.o_e = p->o_e; g.o_T = p->o_T;
    hipError_t e = hipSuccess;
    if (kb || ko) {
        const int64_t edges = (int64_t)in.Mb + in.Mo;
        edge_check_kernel<<<(unsigned)((edges + kEdgeCheckBlock - 1) / kEdgeCheckBlock), kEdgeCheckBlock, 0, s>>>(g);
        e = hipGetLastError();
    }
    if (e == hipSuccess && after_score) e = hipEventRecord(after_score, s);
    if (e == hipSuccess && select[0] && kb) e = select_kind<1>(p, 0, in.Mb, gate_bearing, p->b_neg, p->b_e, p->b_T, s);
    if (e == hipSuccess && select[1] && ko) e = select_kind<3>(p, 1, in.Mo, gate_odom, p->o_neg, p->o_e, p->o_T, s);
    if (e != hipSuccess) { err = std::string("bos_edge_consistency: launch: ") + hipGetErrorString(e); return -2; }
    out->lists = p->lists;
    out->b_neg = g.b_neg; out->b_chi2 = g.b_chi2; out->b_red = g.b_red;
    out->o_neg = g.o_neg; out->o_chi2 = g.o_chi2; out->o_red = g.o_red;
    return 0;
}

}  // namespace dev
}  // namespace bos
