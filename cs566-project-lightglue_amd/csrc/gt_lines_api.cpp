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

int lg_gt_line_depth_thresholds(int32_t npts, double min_visibility_th, double overlap_th, int32_t* min_close,
                                int32_t* out_min_count, int32_t* valid_min_count) {
  if (!min_close || !out_min_count || !valid_min_count) return fail(LG_E_INVALID, "null argument");
  if (npts < 2 || npts > 255) return fail(LG_E_INVALID, "npts must be in 2..255");
  lg::gt_line_min_close_table(npts, overlap_th, min_close);
  *out_min_count = lg::gt_line_count_threshold_visibility(npts, min_visibility_th);
  *valid_min_count = lg::gt_line_count_threshold_valid_depth(npts, min_visibility_th);
  return LG_OK;
}

int lg_gt_line_counts_pose_depth_workspace_bytes(int32_t B, int32_t n0, int32_t n1, int32_t npts, size_t* bytes) {
  return lg_gt_line_counts_workspace_bytes(B, n0, n1, npts, bytes);  // the same records: segments and samples
}

int lg_gt_line_counts_pose_depth(const float* lines0, const float* lines1, const float* depth0, int32_t H0, int32_t W0,
                                 const float* depth1, int32_t H1, int32_t W1, int32_t image_h0, int32_t image_w0,
                                 int32_t image_h1, int32_t image_w1, const float* cam0, const float* cam1, int32_t n_dist,
                                 const float* T_0to1, const float* T_1to0, int32_t B, int32_t n0, int32_t n1, int32_t npts,
                                 double dist_th, double min_visibility_th, uint8_t* num_close_pts0, uint8_t* num_close_pts1_t,
                                 uint8_t* out_of0, uint8_t* out_of1, uint8_t* ignore_depth0, uint8_t* ignore_depth1,
                                 uint8_t* num_visible0, uint8_t* num_visible1, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (!lines0 || !lines1 || !depth0 || !depth1 || !cam0 || !cam1 || !T_0to1 || !T_1to0 || !num_close_pts0 ||
      !num_close_pts1_t || !out_of0 || !out_of1 || !ignore_depth0 || !ignore_depth1 || !num_visible0 || !num_visible1)
    return fail(LG_E_INVALID, "null argument");
  if (B < 0 || n0 < 0 || n1 < 0 || H0 < 0 || W0 < 0 || H1 < 0 || W1 < 0 || image_h0 < 0 || image_w0 < 0 || image_h1 < 0 ||
      image_w1 < 0)
    return fail(LG_E_INVALID, "negative size");
  if (npts < 2 || npts > 255) return fail(LG_E_INVALID, "npts must be in 2..255");
  if (n_dist != 0 && n_dist != 2 && n_dist != 4)
    return fail(LG_E_INVALID, "n_dist must be 0, 2 (k1, k2) or 4 (k1, k2, p1, p2)");
  if (B == 0 || n0 == 0 || n1 == 0) return LG_OK;  // nothing to compare: the caller fills the empty-set outputs
  if (H0 == 0 || W0 == 0 || H1 == 0 || W1 == 0) return fail(LG_E_INVALID, "empty depth map");
  if (const char* m = shape_error(B, n0, n1)) return fail(LG_E_INVALID, m);
  if ((int64_t)H0 * W0 > kLim || (int64_t)H1 * W1 > kLim)
    return fail(LG_E_INVALID, "depth map too large: H * W must stay below 2^31");
  if (!workspace || workspace_bytes < lg::gt_line_counts_workspace_bytes(B, n0, n1, npts))
    return fail(LG_E_INVALID, "workspace too small (lg_gt_line_counts_pose_depth_workspace_bytes)");
  if ((uintptr_t)workspace & 15) return fail(LG_E_INVALID, "workspace is not 16-byte aligned");
  if (((uintptr_t)lines0 | (uintptr_t)lines1 | (uintptr_t)depth0 | (uintptr_t)depth1 | (uintptr_t)cam0 | (uintptr_t)cam1 |
       (uintptr_t)T_0to1 | (uintptr_t)T_1to0) & 3)
    return fail(LG_E_INVALID, "lines / depth maps / cameras / poses are not 4-byte aligned");
  lg::GtLineDepthCall c;
  c.lines0 = lines0, c.lines1 = lines1, c.depth0 = depth0, c.depth1 = depth1, c.cam0 = cam0, c.cam1 = cam1;
  c.T_0to1 = T_0to1, c.T_1to0 = T_1to0;
  c.B = B, c.n0 = n0, c.n1 = n1, c.H0 = H0, c.W0 = W0, c.H1 = H1, c.W1 = W1;
  c.ih0 = image_h0, c.iw0 = image_w0, c.ih1 = image_h1, c.iw1 = image_w1, c.n_dist = n_dist, c.npts = npts;
  c.out_min = lg::gt_line_count_threshold_visibility(npts, min_visibility_th);
  c.valid_min = lg::gt_line_count_threshold_valid_depth(npts, min_visibility_th);
  c.dist_th = (float)dist_th;  // a Python number against an fp32 tensor
  c.cnt0 = num_close_pts0, c.cnt1t = num_close_pts1_t, c.out_of0 = out_of0, c.out_of1 = out_of1;
  c.ignore_depth0 = ignore_depth0, c.ignore_depth1 = ignore_depth1, c.num_visible0 = num_visible0, c.num_visible1 = num_visible1;
  const hipError_t e = lg::gt_line_counts_pose_depth(c, workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("gt_line_counts_pose_depth: ") + hipGetErrorString(e));
  return LG_OK;
}

int lg_gt_line_labels_visibility_workspace_bytes(int32_t B, int32_t n0, int32_t n1, size_t* bytes) {
  return lg_gt_line_labels_workspace_bytes(B, n0, n1, bytes);  // the same cost, assignment and flags
}

int lg_gt_line_labels_visibility(const uint8_t* num_close_pts0, const uint8_t* num_close_pts1_t, const uint8_t* out_of0,
                                 const uint8_t* out_of1, const uint8_t* ignore_depth0, const uint8_t* ignore_depth1,
                                 const uint8_t* num_visible0, const uint8_t* num_visible1, const uint8_t* valid_lines0,
                                 const uint8_t* valid_lines1, int32_t B, int32_t n0, int32_t n1, int32_t npts,
                                 double overlap_th, uint8_t* positive_u8, int64_t* line_matches0, int64_t* line_matches1,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!num_close_pts0 || !num_close_pts1_t || !out_of0 || !out_of1 || !ignore_depth0 || !ignore_depth1 || !num_visible0 ||
      !num_visible1 || !valid_lines0 || !valid_lines1 || !positive_u8 || !line_matches0 || !line_matches1)
    return fail(LG_E_INVALID, "null argument");
  if (B < 0 || n0 < 0 || n1 < 0) return fail(LG_E_INVALID, "negative size");
  if (npts < 2 || npts > 255) return fail(LG_E_INVALID, "npts must be in 2..255");
  if (B == 0 || n0 == 0 || n1 == 0) return LG_OK;  // the caller fills the empty-set outputs
  if (const char* m = shape_error(B, n0, n1)) return fail(LG_E_INVALID, m);
  if (!workspace || workspace_bytes < lg::gt_line_labels_workspace_bytes(B, n0, n1))
    return fail(LG_E_INVALID, "workspace too small (lg_gt_line_labels_visibility_workspace_bytes)");
  if ((uintptr_t)workspace & 15) return fail(LG_E_INVALID, "workspace is not 16-byte aligned");
  if (((uintptr_t)line_matches0 | (uintptr_t)line_matches1) & 7) return fail(LG_E_INVALID, "matches are not 8-byte aligned");
  int min_close[256];
  lg::gt_line_min_close_table(npts, overlap_th, min_close);
  const hipError_t e = lg::gt_line_labels_visibility(num_close_pts0, num_close_pts1_t, out_of0, out_of1, ignore_depth0,
                                                     ignore_depth1, num_visible0, num_visible1, valid_lines0, valid_lines1, B,
                                                     n0, n1, npts, min_close, positive_u8, line_matches0, line_matches1,
                                                     workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("gt_line_labels_visibility: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
