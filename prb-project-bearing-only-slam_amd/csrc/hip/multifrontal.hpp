// GPU supernodal multifrontal Cholesky (hip/multifrontal.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

namespace bos {
struct Multifrontal;
namespace dev {

struct MfDevice;

// Upload the static tree / maps and allocate factor buffers. owner (per supernode, plan.hpp
// Shard::sn_owner) null: one GPU, every front in program 0. Otherwise program 0 = the fronts owned
// by `rank`, program 1 = the replicated top (owner -1); other ranks' fronts are never processed.
// Returns 0 or < 0 with err.
int mf_create(const Multifrontal& F, const int8_t* owner, int rank, MfDevice** out, std::string& err);
void mf_destroy(MfDevice* d);
// Numeric factorization of a program's fronts (H read from the block array A through the assembly
// map, fp64), fused with the forward substitution: x (permuted order) holds b on entry and L^{-1} b
// on exit for those fronts' dofs. Sharded: program 0 (own subtrees), then — once the other ranks'
// subtree roots' U / u are in place — program 1 (the top).
hipError_t mf_factor(MfDevice* d, int program, const double* A, double* x, hipStream_t s);
// fp32 J+H with factored pose-landmark blocks whose pose-landmark and landmark-diagonal entries only
// the folds read (bos::mf_fold_reads_fp32): the folds read them from the fp32 block array A32 (the
// factored region starting at pl_lo), so the fp64 copy need not hold them. Null: the folds read A.
void mf_set_fold_source(MfDevice* d, const float* A32, int64_t pl_lo);
// Backward substitution of a program's fronts (x <- L^{-T} x); sharded: program 1, then program 0.
hipError_t mf_solve(MfDevice* d, int program, double* x, hipStream_t s);
// the update matrices / u-vectors (offsets Multifrontal::U_off / u_off): exchange 1 reads and
// writes the subtree roots' there
double* mf_update_ptr(const MfDevice* d);
double* mf_uvec_ptr(const MfDevice* d);
// device word of the last factorization: count of non-positive pivots, | kMfStall when a dataflow
// launch timed out waiting for a dependency (its results are then invalid)
int32_t* mf_info_ptr(const MfDevice* d);
// device word the dataflow launches compare completion flags with: must be bumped (step_mark
// kernel, kernels.hpp) once per GN step before the step's first mf_factor; all flows of one step
// (factor and backward, both programs when sharded) share it
uint32_t* mf_epoch_ptr(const MfDevice* d);
// Diagnostics: the dataflow launches write 8 realtime stamps per front into stamps ([2][nsuper][8]:
// factor, backward); null (the default) turns them off.
void mf_debug_set_stamps(MfDevice* d, unsigned long long* stamps);
constexpr int32_t kMfStall = 1 << 30;
// Diagnostics (bos_debug_solver_routes): the route (bos_host.h BOS_ROUTE_F_* / BOS_ROUTE_B_*) every
// front took, as the launch sites of mf_factor / mf_solve noted it when program 0's (and, sharded,
// program 1's) sequence was first enqueued; -1 until both have been enqueued once. factor /
// backward: one entry per supernode.
int mf_debug_routes(const MfDevice* d, int8_t* factor, int8_t* backward);
// work-queue tickets (kMfTickets ints, then kMfTickets exit counters); every flow launch leaves its
// ticket zero (the last wave out resets it)
int32_t* mf_tickets_ptr(const MfDevice* d);
constexpr int kMfTickets = 3;
// What the selected inverse (hip/selinv.hpp) reads of a handle: the static tree arrays and the L
// panels of the last mf_factor; and the slot where its state hangs (null until marginals are first
// asked for; mf_destroy frees it)
struct MfView {
    const int32_t *k, *r, *parent, *rmap;
    const int64_t *L_off, *rmap_off;
    const double* L;
};
MfView mf_view(const MfDevice* d);
struct SelInv;
SelInv** mf_selinv_slot(MfDevice* d);
// Test hook (bos_debug_inject_stall): the next factor flow launch starts at ticket 1, so its first
// front is never processed and its parent's wait times out — the stall path, end to end.
hipError_t mf_debug_skip_next_front(MfDevice* d, hipStream_t s);

}  // namespace dev
}  // namespace bos
