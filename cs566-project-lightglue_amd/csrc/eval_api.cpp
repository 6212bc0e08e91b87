// C-ABI of the batched match evaluation (include/lightglue_mi355x.h: lg_eval_matches; kernel in
// match_eval.hip).  No model handle, no workspace.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

extern "C" {

int lg_eval_matches(const float* kpts0, const float* kpts1, const int64_t* matches0, const float* scores0_or_null,
                    int32_t B, int32_t M, int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null,
                    const float* H_gt_or_null, const float* cam0_or_null, const float* cam1_or_null,
                    const float* T_0to1_or_null, const float* image_size0_or_null, int32_t flags,
                    int32_t* hom_counts_or_null, int32_t* epi_counts_or_null, float* H_dlt_or_null,
                    float* H_error_dlt_or_null, void* stream) {
  if (!kpts0 || !kpts1 || !matches0) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || M < 0 || N < 0) return fail(LG_E_INVALID, "negative size");
  if (flags & ~(LG_EVAL_HOMOGRAPHY | LG_EVAL_EPIPOLAR | LG_EVAL_DLT)) return fail(LG_E_INVALID, "unknown flag bits");
  if (!flags) return fail(LG_E_INVALID, "no metric flag set");
  if ((flags & LG_EVAL_HOMOGRAPHY) && (!H_gt_or_null || !hom_counts_or_null))
    return fail(LG_E_INVALID, "LG_EVAL_HOMOGRAPHY needs H_gt and hom_counts");
  if ((flags & LG_EVAL_EPIPOLAR) && (!cam0_or_null || !cam1_or_null || !T_0to1_or_null || !epi_counts_or_null))
    return fail(LG_E_INVALID, "LG_EVAL_EPIPOLAR needs cam0, cam1, T_0to1 and epi_counts");
  if ((flags & LG_EVAL_DLT) &&
      (!H_gt_or_null || !scores0_or_null || !image_size0_or_null || !H_dlt_or_null || !H_error_dlt_or_null))
    return fail(LG_E_INVALID, "LG_EVAL_DLT needs H_gt, scores0, image_size0, H_dlt and H_error_dlt");
  if ((num0_or_null == nullptr) != (num1_or_null == nullptr))
    return fail(LG_E_INVALID, "a ragged batch needs both num0 and num1");
  if ((uintptr_t)matches0 & 7 ||
      ((uintptr_t)kpts0 | (uintptr_t)kpts1 | (uintptr_t)scores0_or_null | (uintptr_t)num0_or_null |
       (uintptr_t)num1_or_null | (uintptr_t)H_gt_or_null | (uintptr_t)cam0_or_null | (uintptr_t)cam1_or_null |
       (uintptr_t)T_0to1_or_null | (uintptr_t)image_size0_or_null | (uintptr_t)hom_counts_or_null |
       (uintptr_t)epi_counts_or_null | (uintptr_t)H_dlt_or_null | (uintptr_t)H_error_dlt_or_null) & 3)
    return fail(LG_E_INVALID, "misaligned pointer");
  if (B == 0 || M == 0) return LG_OK;  // no pair or no query keypoint: the caller fills the empty-set outputs
  lg::EvalCall c;
  c.kp0 = kpts0, c.kp1 = kpts1, c.m0 = matches0, c.s0 = scores0_or_null;
  c.B = B, c.M = M, c.N = N, c.flags = flags;
  c.num0 = num0_or_null, c.num1 = num1_or_null;
  c.H = H_gt_or_null, c.cam0 = cam0_or_null, c.cam1 = cam1_or_null, c.T = T_0to1_or_null;
  c.size0 = image_size0_or_null;
  c.hom_counts = hom_counts_or_null, c.epi_counts = epi_counts_or_null;
  c.H_dlt = H_dlt_or_null, c.H_err = H_error_dlt_or_null;
  const hipError_t e = lg::eval_matches(c, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("eval_matches: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
