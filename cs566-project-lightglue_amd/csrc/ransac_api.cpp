// C-ABI of the batched robust homography estimation (include/lightglue_mi355x.h: lg_ransac_homography;
// kernel in ransac_homography.hip).  No model handle, no workspace.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

extern "C" {

int32_t lg_ransac_lds_matches(void) { return lg::RH_LDS_MATCHES; }

int lg_ransac_homography(const float* kpts0, const float* kpts1, const int64_t* matches0_or_null, int32_t B, int32_t M,
                         int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null, const float* ransac_th,
                         int32_t max_iters, double confidence, uint64_t seed, double min_area,
                         const float* H_gt_or_null, const float* image_size0_or_null, float* H, uint8_t* inliers,
                         int32_t* info, float* m_kpts, float* H_error_or_null, void* stream) {
  if (!kpts0 || !kpts1 || !ransac_th || !H || !inliers || !info || !m_kpts) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || M < 0 || N < 0) return fail(LG_E_INVALID, "negative size");
  if (max_iters < 1 || max_iters > (1 << 30)) return fail(LG_E_INVALID, "max_iters must lie in [1, 2^30]");
  if (!(confidence > 0.0 && confidence < 1.0)) return fail(LG_E_INVALID, "confidence must lie in (0, 1)");
  if (!(min_area >= 0.0)) return fail(LG_E_INVALID, "min_area must not be negative");
  if ((num0_or_null == nullptr) != (num1_or_null == nullptr))
    return fail(LG_E_INVALID, "a ragged batch needs both num0 and num1");
  if (H_error_or_null && (!H_gt_or_null || !image_size0_or_null))
    return fail(LG_E_INVALID, "H_error needs H_gt and image_size0");
  if (!matches0_or_null && M != N) return fail(LG_E_INVALID, "matched points (matches0 null) need M == N");
  if ((uintptr_t)matches0_or_null & 7 || (uintptr_t)m_kpts & 15 ||
      ((uintptr_t)kpts0 | (uintptr_t)kpts1 | (uintptr_t)num0_or_null | (uintptr_t)num1_or_null | (uintptr_t)ransac_th |
       (uintptr_t)H_gt_or_null | (uintptr_t)image_size0_or_null | (uintptr_t)H | (uintptr_t)info |
       (uintptr_t)H_error_or_null) & 3)
    return fail(LG_E_INVALID, "misaligned pointer");
  if (B == 0 || M == 0) return LG_OK;  // no pair or no slot: the caller fills the empty-set outputs
  lg::RansacCall c;
  c.kp0 = kpts0, c.kp1 = kpts1, c.m0 = matches0_or_null;
  c.B = B, c.M = M, c.N = N;
  c.num0 = num0_or_null, c.num1 = num1_or_null;
  c.th = ransac_th, c.max_iters = max_iters, c.log_fail = std::log1p(-confidence), c.seed = seed, c.min_area = min_area;
  c.H_gt = H_gt_or_null, c.size0 = image_size0_or_null;
  c.H = H, c.inliers = inliers, c.info = info, c.m_kpts = m_kpts, c.H_err = H_error_or_null;
  const hipError_t e = lg::ransac_homography(c, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("ransac_homography: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
