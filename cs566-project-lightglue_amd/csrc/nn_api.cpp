// C-ABI of the nearest-neighbour matcher (include/lightglue_mi355x.h: lg_nn_*; kernels in
// nn_match.hip).  No model handle: the matcher has no weights.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

namespace {
// flat-index limits of nn_match.hip: the dense outputs and the plane-image rows are indexed in int
const char* shape_error(int64_t B, int64_t M, int64_t N, int64_t D) {
  if (B < 0 || M < 0 || N < 0 || D < 0) return "negative size";
  if (D < 1 || D > 512) return "descriptor width must be in [1, 512]";
  const int64_t lim = 0x7fffffffLL;
  if (B * M * N > lim || B * (M + 1) * (N + 1) > lim || B * (M + N) + 1024 > lim)
    return "shape too large: B * M * N must stay below 2^31";
  return nullptr;
}
}  // namespace

extern "C" {

int lg_nn_workspace_bytes(int32_t B, int32_t M, int32_t N, int32_t D, int32_t flags, size_t* bytes) {
  (void)flags;  // one layout for every flavour
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (const char* e = shape_error(B, M, N, D)) return fail(LG_E_INVALID, e);
  *bytes = lg::nn_workspace_bytes(B, M, N, D);
  return LG_OK;
}

int lg_nn_match(const float* desc0, const float* desc1, int32_t B, int32_t M, int32_t N, int32_t D, double ratio2,
                double dist2, int32_t flags, const int32_t* num0_or_null, const int32_t* num1_or_null,
                float* similarity_or_null, float* log_assignment_or_null, int64_t* matches0, int64_t* matches1,
                float* scores0, float* scores1, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc0 || !desc1 || !matches0 || !matches1 || !scores0 || !scores1) return fail(LG_E_INVALID, "null argument");
  if (const char* e = shape_error(B, M, N, D)) return fail(LG_E_INVALID, e);
  if (flags & ~(LG_NN_RATIO | LG_NN_DISTANCE | LG_NN_MUTUAL)) return fail(LG_E_INVALID, "unknown flag bits");
  if ((num0_or_null == nullptr) != (num1_or_null == nullptr))
    return fail(LG_E_INVALID, "a ragged batch needs both num0 and num1");
  if (B == 0 || M == 0 || N == 0) return LG_OK;  // nothing to compare: the caller fills the empty-set outputs
  if ((flags & LG_NN_RATIO) && (M < 2 || N < 2))
    return fail(LG_E_INVALID, "the ratio test needs two candidates on each side (M, N >= 2)");
  if (!workspace || workspace_bytes < lg::nn_workspace_bytes(B, M, N, D))
    return fail(LG_E_INVALID, "workspace too small (lg_nn_workspace_bytes)");
  if ((uintptr_t)workspace & 255) return fail(LG_E_INVALID, "workspace is not 256-byte aligned");
  if (((uintptr_t)desc0 | (uintptr_t)desc1) & (D % 32 == 0 ? 15 : 3))
    return fail(LG_E_INVALID, "descriptors are not 16-byte aligned (4-byte when D is no multiple of 32)");
  if (((uintptr_t)matches0 | (uintptr_t)matches1) & 7 ||
      ((uintptr_t)scores0 | (uintptr_t)scores1 | (uintptr_t)similarity_or_null | (uintptr_t)log_assignment_or_null |
       (uintptr_t)num0_or_null | (uintptr_t)num1_or_null) & 3)
    return fail(LG_E_INVALID, "misaligned output");
  lg::NnCall c;
  c.desc0 = desc0, c.desc1 = desc1, c.B = B, c.M = M, c.N = N, c.D = D;
  // the thresholds as the reference compares them: ratio_thresh ** 2 in double, then against fp32 distances
  c.r2 = (float)ratio2, c.d2 = (float)dist2, c.flags = flags;
  c.num0 = num0_or_null, c.num1 = num1_or_null;
  c.sim = similarity_or_null, c.la = log_assignment_or_null;
  c.m0 = matches0, c.m1 = matches1, c.s0 = scores0, c.s1 = scores1;
  const hipError_t e = lg::nn_match(c, workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("nn_match: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
