// C-ABI of the batched robust homography estimation (include/lightglue_mi355x.h: lg_ransac_homography,
// kernel in ransac_homography.hip; lg_ransac_homography_lines, kernel in ransac_homography_lines.hip).
// No model handle, no workspace.
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

int lg_ransac_lines_lds_capacity(int32_t* points, int32_t* lines) {
  if (!points || !lines) return fail(LG_E_INVALID, "null argument");
  *points = lg::RL_LDS_POINTS, *lines = lg::RL_LDS_LINES;
  return LG_OK;
}

int lg_ransac_homography_lines(const float* kpts0, const float* kpts1, const int64_t* matches0_or_null, int32_t B,
                               int32_t M, int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null,
                               const float* lines0, const float* lines1, const int64_t* line_matches0_or_null, int32_t L0,
                               int32_t L1, const int32_t* num_lines0_or_null, const int32_t* num_lines1_or_null,
                               const float* ransac_th, int32_t max_iters, double confidence, uint64_t seed,
                               double min_line_length, const float* H_gt_or_null, const float* image_size0_or_null,
                               float* H, uint8_t* inliers, uint8_t* line_inliers, int32_t* info, float* m_kpts,
                               float* m_lines, float* H_error_or_null, void* stream) {
  if (B < 0 || M < 0 || N < 0 || L0 < 0 || L1 < 0) return fail(LG_E_INVALID, "negative size");
  if (!ransac_th || !H || !info) return fail(LG_E_INVALID, "null argument");
  if (M > 0 && (!kpts0 || !inliers || !m_kpts)) return fail(LG_E_INVALID, "null argument (points)");
  if (M > 0 && N > 0 && !kpts1) return fail(LG_E_INVALID, "null argument (points)");
  if (L0 > 0 && (!lines0 || !line_inliers || !m_lines)) return fail(LG_E_INVALID, "null argument (lines)");
  if (L0 > 0 && L1 > 0 && !lines1) return fail(LG_E_INVALID, "null argument (lines)");
  if (max_iters < 1 || max_iters > (1 << 30)) return fail(LG_E_INVALID, "max_iters must lie in [1, 2^30]");
  if (!(confidence > 0.0 && confidence < 1.0)) return fail(LG_E_INVALID, "confidence must lie in (0, 1)");
  if (!(min_line_length >= 0.0) || !std::isfinite(min_line_length))
    return fail(LG_E_INVALID, "min_line_length must be finite and not negative");
  if ((num0_or_null == nullptr) != (num1_or_null == nullptr))
    return fail(LG_E_INVALID, "a ragged batch needs both num0 and num1");
  if ((num_lines0_or_null == nullptr) != (num_lines1_or_null == nullptr))
    return fail(LG_E_INVALID, "a ragged batch needs both num_lines0 and num_lines1");
  if (H_error_or_null && (!H_gt_or_null || !image_size0_or_null))
    return fail(LG_E_INVALID, "H_error needs H_gt and image_size0");
  if (!matches0_or_null && M != N) return fail(LG_E_INVALID, "matched points (matches0 null) need M == N");
  if (!line_matches0_or_null && L0 != L1) return fail(LG_E_INVALID, "matched lines (line_matches0 null) need L0 == L1");
  if (((uintptr_t)matches0_or_null | (uintptr_t)line_matches0_or_null) & 7 ||
      ((uintptr_t)m_kpts | (uintptr_t)m_lines | (uintptr_t)lines0 | (uintptr_t)lines1) & 15 ||
      ((uintptr_t)kpts0 | (uintptr_t)kpts1 | (uintptr_t)num0_or_null | (uintptr_t)num1_or_null |
       (uintptr_t)num_lines0_or_null | (uintptr_t)num_lines1_or_null | (uintptr_t)ransac_th | (uintptr_t)H_gt_or_null |
       (uintptr_t)image_size0_or_null | (uintptr_t)H | (uintptr_t)info | (uintptr_t)H_error_or_null) & 3)
    return fail(LG_E_INVALID, "misaligned pointer");
  if (B == 0 || (M == 0 && L0 == 0)) return LG_OK;  // no pair or no slot: the caller fills the empty-set outputs
  lg::RansacLinesCall c;
  c.kp0 = kpts0, c.kp1 = kpts1, c.m0 = matches0_or_null;
  c.B = B, c.M = M, c.N = N;
  c.num0 = num0_or_null, c.num1 = num1_or_null;
  c.ln0 = lines0, c.ln1 = lines1, c.lm0 = line_matches0_or_null;
  c.L0 = L0, c.L1 = L1;
  c.nl0 = num_lines0_or_null, c.nl1 = num_lines1_or_null;
  c.th = ransac_th, c.max_iters = max_iters, c.log_fail = std::log1p(-confidence), c.seed = seed;
  c.min_len2 = min_line_length * min_line_length;
  c.H_gt = H_gt_or_null, c.size0 = image_size0_or_null;
  c.H = H, c.inliers = inliers, c.line_inliers = line_inliers, c.info = info, c.m_kpts = m_kpts, c.m_lines = m_lines;
  c.H_err = H_error_or_null;
  const hipError_t e = lg::ransac_homography_lines(c, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("ransac_homography_lines: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
