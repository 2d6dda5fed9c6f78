// Bearing association on the device (hip/associate.hip): see host/associate.hpp for the quantities. Per
// chunk of bearings of one pose, in plain stream order after the node_cov_enqueue whose projected_landmark
// slice they read in place: the NIS kernel (one thread per landmark and bearing) and the selection's two
// stages (per row tile and bearing, then per bearing). No kernel communicates between workgroups, none
// uses an atomic, and the list a bearing gets is the unique minimum of a total order: it depends on no
// grid shape.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../host/associate.hpp"

namespace bos {
namespace dev {

struct Associate;   // the feature's device buffers; owned by the solver handle

constexpr int64_t kAssocRowBudgetBytes = 64ll << 20;   // NIS rows of one chunk
constexpr int kAssocMaxRows = 4096;                    // bearings of one chunk at most (a grid dimension)

// device results of the last enqueued chunk: [rows][kAssocMaxK] lists, [rows] counts, [rows][NL] NIS
struct AssociateDev {
    const int32_t *cand_landmark = nullptr, *n_inside = nullptr;
    const double *cand_nis = nullptr, *cand_innovation = nullptr, *cand_var = nullptr, *nis = nullptr;
};

Associate* associate_create();
void associate_destroy(Associate* p);
int64_t associate_bytes(const Associate* p);
// bearings one chunk may hold for NL landmarks: the byte budget's, at least 1, at most kAssocMaxRows
int associate_budget_rows(int NL);
// Room for chunks of `rows` bearings over NL landmarks (kept when it is already there). 0; -2 with err
// (the byte count) when the allocation fails: nothing is kept then.
int associate_reserve(Associate* p, int NL, int rows, std::string& err);
// Enqueues one chunk on s: rows bearings (z, omega: host arrays, copied before the call returns) taken
// from pose a, var = the node call's projected_landmark slice of a ([NL][4], device), pose / lm the fp64
// master state. before_nis is recorded behind the upload, in front of the NIS kernel, after_nis between
// that kernel and the selection; select false: the rows alone.
int associate_enqueue(Associate* p, int a, int rows, const double* z, const double* omega, double gate, bool select,
                      const double* var, const double* pose, const double* lm, hipStream_t s, hipEvent_t before_nis,
                      hipEvent_t after_nis, AssociateDev* out, std::string& err);

}  // namespace dev
}  // namespace bos
