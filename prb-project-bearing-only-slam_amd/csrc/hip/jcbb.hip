// Joint-compatibility branch and bound: the all-pairings system of a frame assembled in LDS and searched in
// place (host/jcbb.hpp holds the definitions, the total order, the prunings and the order of every operation;
// jcbb_search there is this kernel's loop in serial form and visits the same nodes in the same order). All
// arithmetic is fp64; every wave works alone: no flags, waits, tickets or atomics.
//
// jcbb_kernel: one wavefront (one workgroup) per frame of m <= 32 bearings and P <= 32 pairings.
//   1., 2. e_all, J and S_all as in joint_nis_kernel (joint_stages.hpp joint_assemble); innovation and
//      innovation_cov are written from there when asked for.
//   3. the depth-first search with an explicit stack in registers and LDS. A lane plays three parts: lane q < P
//      keeps e_q and the landmark of pairing q; lane b < m keeps bearing b's list, the next choice to try, the
//      pairings and the prefix NIS on entry, the choice taken, and the best hypothesis's choice and prefix;
//      lane t keeps position t of the current hypothesis: pivot D_t, y_t, pairing and landmark. The unscaled
//      rows of the current hypothesis live in LDS, rows padded to 33 doubles. The loop's control values
//      (bearing, choice, pairings, prefix, best count and NIS, nodes visited) are wave-uniform: they come by
//      v_readlane or a ballot.
//      A new pairing q at position n: lane j <= n reads a_j = S_all[q][q_j]; for k = 0 .. n - 1 the wave reads
//      a_k, D_k and y_k by v_readlane and lane j > k subtracts (a_k / D_k) * A_jk (row j's column k from LDS,
//      33-double rows: 32 different bank pairs; lane n takes a_k itself); y likewise in every lane. The node
//      is accepted when its pivot and prefix pass (jcbb_admissible); the row is then stored and the best
//      hypothesis updated by the total order (the first differing bearing comes from a ballot).
//      The node counter is a uniform register compared with the budget before every visit, so no wave can
//      run past the budget.
#include "jcbb.hpp"
#include "device_mem.hpp"
#include "joint_stages.hpp"
#include "wave_util.hpp"

namespace bos {
namespace dev {

namespace {

constexpr int kWave = 64;

struct JcbbArgs {
    const int32_t *bearing_start, *cand_start;
    const int32_t *hyp_start, *pose, *landmark, *tab;
    const int64_t *tab_off, *s_off;
    const double *z, *omega, *gate;
    const double *state_pose, *state_lm, *diag, *cross;
    unsigned int budget;
    int search;
    int32_t *assignment, *n_paired, *complete;           // any may be null
    double *joint, *prefix, *innovation, *cov;           // any may be null
    int64_t* nodes;                                      // null without the search
};

__device__ __forceinline__ int readlane_i(int x, int l) { return __builtin_amdgcn_readlane(x, l); }

__global__ __launch_bounds__(kWave) void jcbb_kernel(const JcbbArgs a) {
    __shared__ double S[kJointMaxM * kJointLd];
    __shared__ double R[kJointMaxM * kJointLd];
    __shared__ double Jl[kJointMaxM * 5];
    __shared__ double om[kJointMaxM];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int b0 = a.bearing_start[f], m = a.bearing_start[f + 1] - b0;
    const int p0 = a.hyp_start[f], P = a.hyp_start[f + 1] - p0;
    double eq = 0.0;
    if (P > 0) eq = joint_assemble(a, f, lane, p0, P, S, Jl, om);
    if (!a.search) return;
    __syncthreads();
    // lane q: its pairing's landmark; lane j: gate[j]; lane b: bearing b's list
    const int lmQ = lane < P ? a.landmark[p0 + lane] : -1;
    const double gateL = lane < kJointMaxM ? a.gate[lane] : 0.0;
    const int cstart = lane < m ? a.cand_start[b0 + lane] - p0 : 0;
    const int cnt = lane < m ? a.cand_start[b0 + lane + 1] - a.cand_start[b0 + lane] : 0;
    const unsigned long long has = __ballot(lane < m && cnt > 0);
    const int rem_after = lane < kJcbbMaxBearings ? __popcll(has >> (lane + 1)) : 0;
    int pos = 0, n_at = 0, choice = kJcbbNothing, best_choice = kJcbbNothing;
    double pref_at = 0.0, pref_out = 0.0, best_pref = 0.0;
    // lane t: position t of the current hypothesis
    double D_t = 1.0, y_t = 0.0;
    int pq_t = 0, lm_t = -1;
    int best_n = 0;
    double best_nis = 0.0;
    unsigned int nodes = 0;
    int complete = 1;
    int b = 0;
    while (b >= 0) {
        if (b == m) { --b; continue; }
        const int c = readlane_i(pos, b), cb = readlane_i(cnt, b);
        if (c > cb) { --b; continue; }
        if (lane == b) pos = c + 1;
        const int n = readlane_i(n_at, b);
        const double pref = readlane_d(pref_at, b);
        const bool nothing = c == cb;
        if (jcbb_cut(n + readlane_i(rem_after, b) + (nothing ? 0 : 1), pref, best_n, best_nis)) continue;
        int q = 0, lm = -1;
        if (!nothing) {
            q = readlane_i(cstart, b) + c;
            lm = readlane_i(lmQ, q);
            if (__ballot(lane < n && lm_t == lm) != 0ull) continue;   // the landmark is taken
        }
        if (nodes >= a.budget) { complete = 0; break; }
        ++nodes;
        if (nothing) {
            if (lane == b) { choice = kJcbbNothing; pref_out = pref; }
            if (lane == b + 1) { pos = 0; n_at = n; pref_at = pref; }
            ++b;
            continue;
        }
        // row n of the recurrence, lane = column
        double av = 0.0;
        if (lane <= n) av = S[q * kJointLd + (lane == n ? q : pq_t)];
        double yn = readlane_d(eq, q);
        for (int k = 0; k < n; ++k) {
            const double ak = readlane_d(av, k), Dk = readlane_d(D_t, k), yk = readlane_d(y_t, k);
            if (lane > k && lane <= n) av = jcbb_row_step(av, ak, Dk, lane == n ? ak : R[lane * kJointLd + k]);
            yn = jcbb_row_step(yn, ak, Dk, yk);
        }
        const double D = readlane_d(av, n);
        const double pnew = joint_prefix(pref, yn, D);
        if (!jcbb_admissible(pnew, D, readlane_d(gateL, n))) continue;
        if (lane <= n) R[n * kJointLd + lane] = av;
        if (lane == n) { D_t = D; y_t = yn; pq_t = q; lm_t = lm; }
        if (lane == b) { choice = c; pref_out = pnew; }
        if (lane == b + 1) { pos = 0; n_at = n + 1; pref_at = pnew; }
        __syncthreads();
        // the hypothesis: the choices of bearings 0 .. b, nothing afterwards
        const int cur = lane <= b ? choice : kJcbbNothing;
        int cmp = jcbb_compare(n + 1, pnew, best_n, best_nis);
        if (cmp == 0) {
            const unsigned long long diff = __ballot(lane < m && cur != best_choice);
            if (diff != 0ull) {
                const int t = __ffsll((long long)diff) - 1;
                cmp = jcbb_choice_less(readlane_i(cur, t), readlane_i(best_choice, t)) ? 1 : -1;
            }
        }
        if (cmp > 0) {
            best_n = n + 1;
            best_nis = pnew;
            best_choice = cur;
            best_pref = lane <= b ? pref_out : pnew;
        }
        ++b;
    }
    if (lane < m) {
        if (a.assignment) a.assignment[b0 + lane] = best_choice == kJcbbNothing ? -1 : a.landmark[p0 + cstart + best_choice];
        if (a.prefix) a.prefix[b0 + lane] = best_pref;
    }
    if (lane == 0) {
        if (a.n_paired) a.n_paired[f] = best_n;
        if (a.joint) a.joint[f] = best_nis;
        if (a.complete) a.complete[f] = complete;
        if (a.nodes) a.nodes[f] = (int64_t)nodes;
    }
}

}  // namespace

struct Jcbb {
    DeviceMem mem;   // the arena alone
    char* arena = nullptr;
    int32_t n_frames = 0;
    unsigned int budget = 0;
    bool search = false;
    int32_t *bearing_start = nullptr, *cand_start = nullptr, *hyp_start = nullptr, *pose = nullptr, *landmark = nullptr, *tab = nullptr;
    int64_t *tab_off = nullptr, *s_off = nullptr;
    double *z = nullptr, *omega = nullptr, *gate = nullptr;
    int32_t *assignment = nullptr, *n_paired = nullptr, *complete = nullptr;
    double *joint = nullptr, *prefix = nullptr, *innovation = nullptr, *cov = nullptr;
    int64_t* nodes = nullptr;
};

Jcbb* jcbb_create() { return new Jcbb(); }

void jcbb_destroy(Jcbb* p) { delete p; }

int64_t jcbb_bytes(const Jcbb* p) { return p ? (int64_t)p->mem.bytes() : 0; }

int jcbb_upload(Jcbb* p, const JcbbBatch& b, const JcbbWant& want, std::string& err) {
    // one arena: [index arrays | z, omega, gate | outputs], every part aligned to 256 bytes (an empty one keeps an
    // element's room); it only grows
    const size_t nf = (size_t)b.n_frames, nb = (size_t)b.n_bearings, np = (size_t)b.n_pair;
    Arena ar(true);
    ar.add(&p->bearing_start, b.bearing_start, nf + 1);
    ar.add(&p->cand_start, b.cand_start, nb + 1);
    ar.add(&p->hyp_start, b.hyp_start, nf + 1);
    ar.add(&p->tab_off, b.tab_off, nf); ar.add(&p->s_off, b.s_off, nf);
    ar.add(&p->pose, b.pose, np); ar.add(&p->landmark, b.landmark, np);
    ar.add(&p->tab, b.tab, 4 * (size_t)b.n_entries);
    ar.add(&p->z, b.z, np); ar.add(&p->omega, b.omega, np);
    ar.add(&p->gate, b.gate, (size_t)kJointMaxM);
    const bool search = want.search();
    ar.reserve(&p->assignment, want.assignment ? nb : 0);
    ar.reserve(&p->n_paired, want.n_paired ? nf : 0);
    ar.reserve(&p->complete, want.complete ? nf : 0);
    ar.reserve(&p->joint, want.joint_nis ? nf : 0);
    ar.reserve(&p->prefix, want.prefix_nis ? nb : 0);
    ar.reserve(&p->innovation, want.innovation ? np : 0);
    ar.reserve(&p->cov, want.cov ? (size_t)b.s_count : 0);
    ar.reserve(&p->nodes, search ? nf : 0);
    bool ok;
    if (ar.bytes() > p->mem.bytes()) {
        p->mem.release(p->arena);
        ok = ar.commit(p->mem, &p->arena);
    } else {
        ok = ar.place(p->arena);
    }
    if (!ok) {
        err = "bos_jcbb: device allocation or upload of " + std::to_string(ar.bytes()) + " bytes failed";
        return -2;
    }
    p->n_frames = b.n_frames;
    p->budget = (unsigned int)b.budget;
    p->search = search;
    if (!want.assignment) p->assignment = nullptr;
    if (!want.n_paired) p->n_paired = nullptr;
    if (!want.complete) p->complete = nullptr;
    if (!want.joint_nis) p->joint = nullptr;
    if (!want.prefix_nis) p->prefix = nullptr;
    if (!want.innovation) p->innovation = nullptr;
    if (!want.cov) p->cov = nullptr;
    if (!search) p->nodes = nullptr;
    return 0;
}

int jcbb_enqueue(Jcbb* p, const double* pose, const double* lm, const double* diag, const double* cross, hipStream_t s, JcbbOut* out,
                 std::string& err) {
    if (!p->arena) { err = "bos_jcbb: no batch uploaded"; return -1; }
    if (p->n_frames > 0) {
        JcbbArgs a;
        a.bearing_start = p->bearing_start; a.cand_start = p->cand_start;
        a.hyp_start = p->hyp_start; a.pose = p->pose; a.landmark = p->landmark; a.tab = p->tab;
        a.tab_off = p->tab_off; a.s_off = p->s_off; a.z = p->z; a.omega = p->omega; a.gate = p->gate;
        a.state_pose = pose; a.state_lm = lm; a.diag = diag; a.cross = cross;
        a.budget = p->budget; a.search = p->search ? 1 : 0;
        a.assignment = p->assignment; a.n_paired = p->n_paired; a.complete = p->complete;
        a.joint = p->joint; a.prefix = p->prefix; a.innovation = p->innovation; a.cov = p->cov; a.nodes = p->nodes;
        jcbb_kernel<<<(unsigned)p->n_frames, kWave, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = std::string("bos_jcbb: launch: ") + hipGetErrorString(e); return -2; }
    }
    out->assignment = p->assignment; out->n_paired = p->n_paired; out->complete = p->complete;
    out->joint_nis = p->joint; out->prefix_nis = p->prefix; out->innovation = p->innovation; out->innovation_cov = p->cov;
    out->nodes = p->nodes;
    return 0;
}

}  // namespace dev
}  // namespace bos
