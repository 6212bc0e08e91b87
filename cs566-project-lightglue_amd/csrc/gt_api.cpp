// C-ABI of the ground truth (include/lightglue_mi355x.h: lg_gt_*; kernels in gt_match.hip for homography
// pairs and gt_depth.hip for posed pairs with depth).  No model handle: the work depends on the
// keypoints and the pair's geometry alone.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

namespace {
// launch-grid and flat-index limits of gt_match.hip / gt_depth.hip
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

int lg_gt_depth_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || M < 0 || N < 0) return fail(LG_E_INVALID, "negative size");
  *bytes = lg::gt_depth_workspace_bytes(B, M, N);
  return LG_OK;
}

int lg_gt_matches_from_pose_depth(const float* kp0, const float* kp1, const float* depth0_or_null, int32_t H0, int32_t W0,
                                  const float* depth1_or_null, int32_t H1, int32_t W1, const float* cam0, const float* cam1,
                                  int32_t n_dist, const float* T_0to1, const float* T_1to0, int32_t B, int32_t M, int32_t N,
                                  double pos_th, double neg_th, double th_epi_or_nan, double th_consistency_or_nan,
                                  float* depth_keypoints0, float* depth_keypoints1, const uint8_t* valid_depth0_or_null,
                                  const uint8_t* valid_depth1_or_null, uint8_t* assignment_u8, float* reward_or_null,
                                  int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* proj_0to1,
                                  float* proj_1to0, uint8_t* visible0_u8, uint8_t* visible1_u8, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!kp0 || !kp1 || !cam0 || !cam1 || !T_0to1 || !T_1to0 || !depth_keypoints0 || !depth_keypoints1 || !assignment_u8 ||
      !matches0 || !matches1 || !scores0 || !scores1 || !proj_0to1 || !proj_1to0 || !visible0_u8 || !visible1_u8)
    return fail(LG_E_INVALID, "null argument");
  if (B < 0 || M < 0 || N < 0 || H0 < 0 || W0 < 0 || H1 < 0 || W1 < 0) return fail(LG_E_INVALID, "negative size");
  if (n_dist != 0 && n_dist != 2 && n_dist != 4)
    return fail(LG_E_INVALID, "n_dist must be 0, 2 (k1, k2) or 4 (k1, k2, p1, p2)");
  if ((valid_depth0_or_null == nullptr) != (valid_depth1_or_null == nullptr))
    return fail(LG_E_INVALID, "precomputed depths need both valid_depth0 and valid_depth1");
  const bool use_cc = th_consistency_or_nan == th_consistency_or_nan, use_epi = th_epi_or_nan == th_epi_or_nan;
  const bool sample = valid_depth0_or_null == nullptr;
  if ((sample || use_cc) && (!depth0_or_null || !depth1_or_null || H0 == 0 || W0 == 0 || H1 == 0 || W1 == 0))
    return fail(LG_E_INVALID, "depth maps are needed (no precomputed depths, or th_consistency set)");
  if (B == 0 || M == 0 || N == 0) return LG_OK;  // nothing to compare: the caller fills the empty-set outputs
  if (!shape_ok(B, M, N)) return fail(LG_E_INVALID, "shape too large: M * N must stay below 2^31");
  if ((int64_t)H0 * W0 > 0x7fffffffLL || (int64_t)H1 * W1 > 0x7fffffffLL)
    return fail(LG_E_INVALID, "depth map too large: H * W must stay below 2^31");
  if (!workspace || workspace_bytes < lg::gt_depth_workspace_bytes(B, M, N))
    return fail(LG_E_INVALID, "workspace too small (lg_gt_depth_workspace_bytes)");
  if ((uintptr_t)workspace & 15) return fail(LG_E_INVALID, "workspace is not 16-byte aligned");
  if (reward_or_null && ((uintptr_t)reward_or_null & 3)) return fail(LG_E_INVALID, "reward is not 4-byte aligned");
  if (((uintptr_t)kp0 | (uintptr_t)kp1 | (uintptr_t)proj_0to1 | (uintptr_t)proj_1to0) & 7)
    return fail(LG_E_INVALID, "keypoints / projections are not 8-byte aligned");
  if (((uintptr_t)matches0 | (uintptr_t)matches1) & 7 ||
      ((uintptr_t)scores0 | (uintptr_t)scores1 | (uintptr_t)cam0 | (uintptr_t)cam1 | (uintptr_t)T_0to1 | (uintptr_t)T_1to0 |
       (uintptr_t)depth0_or_null | (uintptr_t)depth1_or_null | (uintptr_t)depth_keypoints0 | (uintptr_t)depth_keypoints1) & 3)
    return fail(LG_E_INVALID, "misaligned pointer");
  lg::GtDepthCall c;
  c.kp0 = kp0, c.kp1 = kp1, c.depth0 = depth0_or_null, c.depth1 = depth1_or_null, c.cam0 = cam0, c.cam1 = cam1;
  c.T_0to1 = T_0to1, c.T_1to0 = T_1to0;
  c.H0 = H0, c.W0 = W0, c.H1 = H1, c.W1 = W1, c.n_dist = n_dist, c.B = B, c.M = M, c.N = N;
  // the thresholds as the reference compares them: a Python float against fp32 tensors
  c.pos2 = (float)(pos_th * pos_th), c.neg2 = (float)(neg_th * neg_th), c.negf = (float)neg_th;
  c.ccth = use_cc ? (float)th_consistency_or_nan : 0.f;
  c.use_epi = use_epi, c.use_cc = use_cc;
  c.dk0 = depth_keypoints0, c.dk1 = depth_keypoints1, c.valid_in0 = valid_depth0_or_null, c.valid_in1 = valid_depth1_or_null;
  c.assignment = assignment_u8, c.reward = reward_or_null, c.m0 = matches0, c.m1 = matches1, c.s0 = scores0, c.s1 = scores1;
  c.p01 = proj_0to1, c.p10 = proj_1to0, c.vis0 = visible0_u8, c.vis1 = visible1_u8;
  const hipError_t e = lg::gt_matches_from_pose_depth(c, workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("gt_matches_from_pose_depth: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
