// C-ABI of the line ground truth and the batched assignment solver (include/lightglue_mi355x.h:
// lg_gt_line_*, lg_linear_sum_assignment; kernels in gt_lines.hip).  No model handle.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

namespace {
const int64_t kLim = 0x7fffffffLL;

// flat-index and launch-grid limits of gt_lines.hip
const char* shape_error(int64_t B, int64_t n0, int64_t n1) {
  if (n0 * n1 > kLim) return "shape too large: n0 * n1 must stay below 2^31";
  if (B * ((n0 + 15) / 16) * ((n1 + 15) / 16) > kLim || (B * n0 * n1 + 255) / 256 > kLim || B * (n0 + n1) > kLim)
    return "shape too large: B * n0 * n1 exceeds the launch grid";
  return nullptr;
}
}  // namespace

extern "C" {

int lg_gt_line_thresholds(int32_t npts, double min_visibility_th, double overlap_th, int32_t* out_min_count,
                          int32_t* close_min_count) {
  if (!out_min_count || !close_min_count) return fail(LG_E_INVALID, "null argument");
  if (npts < 2 || npts > 255) return fail(LG_E_INVALID, "npts must be in 2..255");
  *out_min_count = lg::gt_line_count_threshold_visibility(npts, min_visibility_th);
  *close_min_count = lg::gt_line_count_threshold_overlap(npts, overlap_th);
  return LG_OK;
}

int lg_gt_line_counts_workspace_bytes(int32_t B, int32_t n0, int32_t n1, int32_t npts, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || n0 < 0 || n1 < 0) return fail(LG_E_INVALID, "negative size");
  if (npts < 2 || npts > 255) return fail(LG_E_INVALID, "npts must be in 2..255");
  *bytes = lg::gt_line_counts_workspace_bytes(B, n0, n1, npts);
  return LG_OK;
}

int lg_gt_line_counts_homography(const float* lines0, const float* lines1, const float* H, int32_t B, int32_t n0, int32_t n1,
                                 int32_t h0, int32_t w0, int32_t h1, int32_t w1, int32_t npts, double dist_th,
                                 double min_visibility_th, uint8_t* num_close_pts0, uint8_t* num_close_pts1_t,
                                 uint8_t* out_of0, uint8_t* out_of1, void* workspace, size_t workspace_bytes, void* stream) {
  if (!lines0 || !lines1 || !H || !num_close_pts0 || !num_close_pts1_t || !out_of0 || !out_of1)
    return fail(LG_E_INVALID, "null argument");
  if (B < 0 || n0 < 0 || n1 < 0 || h0 < 0 || w0 < 0 || h1 < 0 || w1 < 0) return fail(LG_E_INVALID, "negative size");
  if (npts < 2 || npts > 255) return fail(LG_E_INVALID, "npts must be in 2..255");
  if (B == 0 || n0 == 0 || n1 == 0) return LG_OK;  // nothing to compare: the caller fills the empty-set outputs
  if (const char* m = shape_error(B, n0, n1)) return fail(LG_E_INVALID, m);
  if (!workspace || workspace_bytes < lg::gt_line_counts_workspace_bytes(B, n0, n1, npts))
    return fail(LG_E_INVALID, "workspace too small (lg_gt_line_counts_workspace_bytes)");
  if ((uintptr_t)workspace & 15) return fail(LG_E_INVALID, "workspace is not 16-byte aligned");
  if (((uintptr_t)lines0 | (uintptr_t)lines1 | (uintptr_t)H) & 3) return fail(LG_E_INVALID, "lines / H are not 4-byte aligned");
  // dist_th as the reference compares it: a Python number against an fp32 tensor
  const hipError_t e = lg::gt_line_counts_homography(
      lines0, lines1, H, B, n0, n1, w0, h0, w1, h1, npts, (float)dist_th,
      lg::gt_line_count_threshold_visibility(npts, min_visibility_th), num_close_pts0, num_close_pts1_t, out_of0, out_of1,
      workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("gt_line_counts_homography: ") + hipGetErrorString(e));
  return LG_OK;
}

int lg_linear_sum_assignment_workspace_bytes(int32_t B, int32_t nr, int32_t nc, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || nr < 0 || nc < 0) return fail(LG_E_INVALID, "negative size");
  *bytes = lg::linear_sum_assignment_workspace_bytes(B, nr, nc);
  return LG_OK;
}

int lg_linear_sum_assignment(const double* cost, int32_t B, int32_t nr, int32_t nc, int64_t* row_ind, int64_t* col_ind,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!cost || !row_ind || !col_ind) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || nr < 0 || nc < 0) return fail(LG_E_INVALID, "negative size");
  if (B == 0 || nr == 0 || nc == 0) return LG_OK;
  if ((int64_t)nr * nc > kLim) return fail(LG_E_INVALID, "shape too large: nr * nc must stay below 2^31");
  const size_t need = lg::linear_sum_assignment_workspace_bytes(B, nr, nc);
  if (need && (!workspace || workspace_bytes < need))
    return fail(LG_E_INVALID, "workspace too small (lg_linear_sum_assignment_workspace_bytes)");
  if (need && ((uintptr_t)workspace & 15)) return fail(LG_E_INVALID, "workspace is not 16-byte aligned");
  if (((uintptr_t)cost | (uintptr_t)row_ind | (uintptr_t)col_ind) & 7) return fail(LG_E_INVALID, "misaligned pointer");
  const hipError_t e = lg::linear_sum_assignment(cost, B, nr, nc, row_ind, col_ind, workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("linear_sum_assignment: ") + hipGetErrorString(e));
  return LG_OK;
}

int lg_gt_line_labels_workspace_bytes(int32_t B, int32_t n0, int32_t n1, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || n0 < 0 || n1 < 0) return fail(LG_E_INVALID, "negative size");
  *bytes = lg::gt_line_labels_workspace_bytes(B, n0, n1);
  return LG_OK;
}

int lg_gt_line_labels(const uint8_t* num_close_pts0, const uint8_t* num_close_pts1_t, const uint8_t* out_of0,
                      const uint8_t* out_of1, const uint8_t* valid_lines0, const uint8_t* valid_lines1, int32_t B, int32_t n0,
                      int32_t n1, int32_t npts, double overlap_th, uint8_t* positive_u8, int64_t* line_matches0,
                      int64_t* line_matches1, void* workspace, size_t workspace_bytes, void* stream) {
  if (!num_close_pts0 || !num_close_pts1_t || !out_of0 || !out_of1 || !valid_lines0 || !valid_lines1 || !positive_u8 ||
      !line_matches0 || !line_matches1)
    return fail(LG_E_INVALID, "null argument");
  if (B < 0 || n0 < 0 || n1 < 0) return fail(LG_E_INVALID, "negative size");
  if (npts < 2 || npts > 255) return fail(LG_E_INVALID, "npts must be in 2..255");
  if (B == 0 || n0 == 0 || n1 == 0) return LG_OK;  // the caller fills the empty-set outputs
  if (const char* m = shape_error(B, n0, n1)) return fail(LG_E_INVALID, m);
  if (!workspace || workspace_bytes < lg::gt_line_labels_workspace_bytes(B, n0, n1))
    return fail(LG_E_INVALID, "workspace too small (lg_gt_line_labels_workspace_bytes)");
  if ((uintptr_t)workspace & 15) return fail(LG_E_INVALID, "workspace is not 16-byte aligned");
  if (((uintptr_t)line_matches0 | (uintptr_t)line_matches1) & 7) return fail(LG_E_INVALID, "matches are not 8-byte aligned");
  const hipError_t e = lg::gt_line_labels(num_close_pts0, num_close_pts1_t, out_of0, out_of1, valid_lines0, valid_lines1, B, n0,
                                          n1, lg::gt_line_count_threshold_overlap(npts, overlap_th), positive_u8,
                                          line_matches0, line_matches1, workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("gt_line_labels: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
