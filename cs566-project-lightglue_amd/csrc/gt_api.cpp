// C-ABI of the homography ground truth (include/lightglue_mi355x.h: lg_gt_*; kernels in gt_match.hip).
// No model handle: the work depends on the keypoints and the homography alone.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lightglue_mi355x.h"
#include "kernels.h"

namespace lg {
int api_fail(int code, const char* msg);
}

namespace {
int fail(int code, const std::string& msg) { return lg::api_fail(code, msg.c_str()); }

// launch-grid and flat-index limits of gt_match.hip
bool shape_ok(int64_t B, int64_t M, int64_t N) {
  const int64_t lim = 0x7fffffffLL;
  return M * N <= lim && B * ((M + 63) / 64 + (N + 63) / 64) <= lim && B * ((M * N / 4 + 256) / 256) <= lim &&
         B * (M + N) <= lim * 128;
}
}  // namespace

extern "C" {

int lg_gt_homography_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || M < 0 || N < 0) return fail(LG_E_INVALID, "negative size");
  *bytes = lg::gt_homography_workspace_bytes(B, M, N);
  return LG_OK;
}

int lg_gt_matches_from_homography(const float* kp0, const float* kp1, const float* H, int32_t B, int32_t M, int32_t N,
                                  double pos_th, double neg_th, uint8_t* assignment_u8, float* reward_or_null,
                                  int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* proj_0to1,
                                  float* proj_1to0, void* workspace, size_t workspace_bytes, void* stream) {
  if (!kp0 || !kp1 || !H || !assignment_u8 || !matches0 || !matches1 || !scores0 || !scores1 || !proj_0to1 || !proj_1to0)
    return fail(LG_E_INVALID, "null argument");
  if (B < 0 || M < 0 || N < 0) return fail(LG_E_INVALID, "negative size");
  if (B == 0 || M == 0 || N == 0) return LG_OK;  // nothing to compare: the caller fills the empty-set outputs
  if (!shape_ok(B, M, N)) return fail(LG_E_INVALID, "shape too large: M * N must stay below 2^31");
  if (!workspace || workspace_bytes < lg::gt_homography_workspace_bytes(B, M, N))
    return fail(LG_E_INVALID, "workspace too small (lg_gt_homography_workspace_bytes)");
  if (reward_or_null && ((uintptr_t)reward_or_null & 3)) return fail(LG_E_INVALID, "reward is not 4-byte aligned");
  if (((uintptr_t)kp0 | (uintptr_t)kp1 | (uintptr_t)proj_0to1 | (uintptr_t)proj_1to0) & 7)
    return fail(LG_E_INVALID, "keypoints / projections are not 8-byte aligned");
  if (((uintptr_t)matches0 | (uintptr_t)matches1) & 7 || ((uintptr_t)scores0 | (uintptr_t)scores1 | (uintptr_t)H) & 3)
    return fail(LG_E_INVALID, "misaligned output");
  // the thresholds as the reference compares them: pos_th ** 2 in double, then against fp32 distances
  const float pos2 = (float)(pos_th * pos_th), neg2 = (float)(neg_th * neg_th);
  const hipError_t e = lg::gt_matches_from_homography(kp0, kp1, H, B, M, N, pos2, neg2, assignment_u8, reward_or_null,
                                                      matches0, matches1, scores0, scores1, proj_0to1, proj_1to0, workspace,
                                                      (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("gt_matches_from_homography: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
