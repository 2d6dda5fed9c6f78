// Joint compatibility: S = J Sigma J^T + R of a hypothesis from the pair call's blocks, its LDL^T and the
// prefix NIS (host/joint.hpp holds the expressions and the order of every operation). All arithmetic is
// fp64; every wave works alone: no flags, waits, tickets or atomics.
//
// joint_nis_kernel: one wavefront (one workgroup) per hypothesis of m <= 32 pairings.
// Stages 1 and 2 are joint_assemble (joint_stages.hpp), shared with jcbb_kernel (jcbb.hip).
//   1. lane i < m evaluates e_i and J_i at the master state (J_i and omega_i go to LDS).
//   2. the lanes stride over the m (m + 1) / 2 <= 528 lower entries of S: a lane gathers the entry's four
//      blocks through the hypothesis's table (joint_S_entry) and writes the value to LDS at (i, j) and (j, i),
//      rows padded to 33 doubles, and to innovation_cov when that is asked for.
//   3. the right-looking LDL^T with lane = row: at step k every lane reads D_k = A_kk (one address: a
//      broadcast), row i scales its A_ik in a register and updates its A_ij, k < j <= i, from column k,
//      which no lane writes during the step; one barrier (the wave's own) ends the step. With 33-double
//      rows the lanes' reads of one column fall on 32 different bank pairs. y lives in a register per lane;
//      y_k comes by v_readlane. The prefix sum is the same scalar in every lane; lane k keeps prefix_k.
#include "joint.hpp"
#include "device_mem.hpp"
#include "joint_stages.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

constexpr int kWave = 64;

struct JointArgs {
    const int32_t *hyp_start, *pose, *landmark, *tab;
    const int64_t *tab_off, *s_off;
    const double *z, *omega;
    const double *state_pose, *state_lm, *diag, *cross;
    double *prefix, *joint, *innovation, *cov;   // any may be null
};

__global__ __launch_bounds__(kWave) void joint_nis_kernel(const JointArgs a) {
    __shared__ double S[kJointMaxM * kJointLd];
    __shared__ double Jl[kJointMaxM * 5];
    __shared__ double om[kJointMaxM];
    const int h = blockIdx.x, lane = threadIdx.x;
    const int p0 = a.hyp_start[h], m = a.hyp_start[h + 1] - p0;
    if (m == 0) {
        if (lane == 0 && a.joint) a.joint[h] = 0.0;
        return;
    }
    double y = joint_assemble(a, h, lane, p0, m, S, Jl, om);
    if (!a.prefix && !a.joint) return;
    __syncthreads();
    double prev = 0.0, mine = joint_nan();
    for (int k = 0; k < m; ++k) {
        const double D = S[k * kJointLd + k];
        if (!joint_pivot_ok(D)) break;   // the same D in every lane
        const double yk = readlane_d(y, k);
        if (lane > k && lane < m) {
            const double l = joint_l(S[lane * kJointLd + k], D);
            for (int j = k + 1; j <= lane; ++j) S[lane * kJointLd + j] = joint_sub(S[lane * kJointLd + j], l, S[j * kJointLd + k]);
            y = joint_sub(y, l, yk);
        }
        prev = joint_prefix(prev, yk, D);
        if (lane == k) mine = prev;
        __syncthreads();
    }
    if (lane < m && a.prefix) a.prefix[p0 + lane] = mine;
    if (lane == m - 1 && a.joint) a.joint[h] = mine;
}

}  // namespace

struct Joint {
    DeviceMem mem;   // the arena alone
    char* arena = nullptr;
    int32_t n_hyp = 0;
    int32_t *hyp_start = nullptr, *pose = nullptr, *landmark = nullptr, *tab = nullptr;
    int64_t *tab_off = nullptr, *s_off = nullptr;
    double *z = nullptr, *omega = nullptr, *out[4] = {};
};

Joint* joint_create() { return new Joint(); }

void joint_destroy(Joint* p) { delete p; }

int64_t joint_bytes(const Joint* p) { return p ? (int64_t)p->mem.bytes() : 0; }

int joint_upload(Joint* p, const JointBatch& b, const bool want[4], std::string& err) {
    // one arena: [index arrays | z, omega | outputs], every part aligned to 256 bytes (an empty one keeps an
    // element's room); it only grows
    const size_t nh = (size_t)b.n_hyp, np = (size_t)b.n_pair;
    Arena ar(true);
    ar.add(&p->hyp_start, b.hyp_start, nh + 1);
    ar.add(&p->tab_off, b.tab_off, nh); ar.add(&p->s_off, b.s_off, nh);
    ar.add(&p->pose, b.pose, np); ar.add(&p->landmark, b.landmark, np);
    ar.add(&p->tab, b.tab, 4 * (size_t)b.n_entries);
    ar.add(&p->z, b.z, np); ar.add(&p->omega, b.omega, np);
    const size_t count[4] = {np, nh, np, (size_t)b.s_count};
    for (int i = 0; i < 4; ++i) ar.reserve(&p->out[i], want[i] ? count[i] : 0);
    bool ok;
    if (ar.bytes() > p->mem.bytes()) {
        p->mem.release(p->arena);
        ok = ar.commit(p->mem, &p->arena);
    } else {
        ok = ar.place(p->arena);
    }
    if (!ok) {
        err = "bos_joint_compatibility: device allocation or upload of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    p->n_hyp = b.n_hyp;
    for (int i = 0; i < 4; ++i)
        if (!want[i]) p->out[i] = nullptr;
    return 0;
}

int joint_enqueue(Joint* p, const double* pose, const double* lm, const double* diag, const double* cross, hipStream_t s, JointOut* out,
                  std::string& err) {
    if (!p->arena) { err = "bos_joint_compatibility: no batch uploaded"; return -1; }
    if (p->n_hyp > 0) {
        JointArgs a;
        a.hyp_start = p->hyp_start; a.pose = p->pose; a.landmark = p->landmark; a.tab = p->tab;
        a.tab_off = p->tab_off; a.s_off = p->s_off; a.z = p->z; a.omega = p->omega;
        a.state_pose = pose; a.state_lm = lm; a.diag = diag; a.cross = cross;
        a.prefix = p->out[0]; a.joint = p->out[1]; a.innovation = p->out[2]; a.cov = p->out[3];
        joint_nis_kernel<<<(unsigned)p->n_hyp, kWave, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = std::string("bos_joint_compatibility: launch: ") + hipGetErrorString(e); return -2; }
    }
    out->prefix_nis = p->out[0]; out->joint_nis = p->out[1]; out->innovation = p->out[2]; out->innovation_cov = p->out[3];
    return 0;
}

}  // namespace dev
}  // namespace bos
