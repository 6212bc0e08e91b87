// C-ABI of the batched robust relative-pose estimation (include/lightglue_mi355x.h: lg_ransac_relpose,
// lg_essential_5pt; kernels in ransac_relpose.hip).  No model handle; the round's candidates live in a
// stream-ordered allocation freed before returning.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

extern "C" {

int lg_ransac_relpose(const float* kpts0, const float* kpts1, const int64_t* matches0_or_null, int32_t B, int32_t M,
                      int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null, const float* camera0,
                      const float* camera1, const float* ransac_th, int32_t max_iters, double confidence, uint64_t seed,
                      const float* T_gt_or_null, float* R, float* t, uint8_t* inliers, int32_t* info, float* m_kpts,
                      float* errors_or_null, void* stream) {
  if (!kpts0 || !kpts1 || !camera0 || !camera1 || !ransac_th || !R || !t || !inliers || !info || !m_kpts)
    return fail(LG_E_INVALID, "null argument");
  if (B < 0 || M < 0 || N < 0) return fail(LG_E_INVALID, "negative size");
  if (max_iters < 1 || max_iters > (1 << 30)) return fail(LG_E_INVALID, "max_iters must lie in [1, 2^30]");
  if (!(confidence > 0.0 && confidence < 1.0)) return fail(LG_E_INVALID, "confidence must lie in (0, 1)");
  if ((num0_or_null == nullptr) != (num1_or_null == nullptr))
    return fail(LG_E_INVALID, "a ragged batch needs both num0 and num1");
  if (errors_or_null && !T_gt_or_null) return fail(LG_E_INVALID, "errors need T_gt");
  if (!matches0_or_null && M != N) return fail(LG_E_INVALID, "matched points (matches0 null) need M == N");
  if ((uintptr_t)matches0_or_null & 7 || (uintptr_t)m_kpts & 15 ||
      ((uintptr_t)kpts0 | (uintptr_t)kpts1 | (uintptr_t)num0_or_null | (uintptr_t)num1_or_null | (uintptr_t)camera0 |
       (uintptr_t)camera1 | (uintptr_t)ransac_th | (uintptr_t)T_gt_or_null | (uintptr_t)R | (uintptr_t)t |
       (uintptr_t)info | (uintptr_t)errors_or_null) & 3)
    return fail(LG_E_INVALID, "misaligned pointer");
  if (B == 0 || M == 0) return LG_OK;  // no pair or no slot: the caller fills the empty-set outputs
  hipStream_t st = (hipStream_t)stream;
  lg::RelposeCall c;
  c.kp0 = kpts0, c.kp1 = kpts1, c.m0 = matches0_or_null;
  c.B = B, c.M = M, c.N = N;
  c.num0 = num0_or_null, c.num1 = num1_or_null;
  c.cam0 = camera0, c.cam1 = camera1;
  c.th = ransac_th, c.max_iters = max_iters, c.log_fail = std::log1p(-confidence), c.seed = seed;
  c.T_gt = T_gt_or_null;
  c.R = R, c.t = t, c.inliers = inliers, c.info = info, c.m_kpts = m_kpts, c.err = errors_or_null;
  c.ws = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&c.ws), lg::ransac_relpose_workspace_bytes(B), st);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("ransac_relpose workspace: ") + hipGetErrorString(e));
  e = lg::ransac_relpose(c, st);
  const hipError_t f = hipFreeAsync(c.ws, st);
  if (e == hipSuccess) e = f;
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("ransac_relpose: ") + hipGetErrorString(e));
  return LG_OK;
}

int lg_essential_5pt(const float* pts, int32_t S, double* E, int32_t* count, void* stream) {
  if (!pts || !E || !count) return fail(LG_E_INVALID, "null argument");
  if (S < 0) return fail(LG_E_INVALID, "negative size");
  if ((uintptr_t)E & 7 || ((uintptr_t)pts | (uintptr_t)count) & 3) return fail(LG_E_INVALID, "misaligned pointer");
  if (S == 0) return LG_OK;
  const hipError_t e = lg::essential_5pt(pts, S, E, count, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("essential_5pt: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
