// C-ABI of the wireframe step (include/wireframe_mi355x.h: lg_wireframe_*, lg_sample_descriptors_corner;
// kernels in wireframe.hip).  No model handle: the step has no weights.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/wireframe_mi355x.h"
#include "api_common.h"
#include "kernels.h"

static_assert(2 * LG_WIREFRAME_MAX_LINES == lg::kWfMaxEndpoints, "header and kernel capacity differ");

namespace {
const char* map_error(int64_t B, int64_t Hc, int64_t Wc, int64_t D) {
  if (B < 0 || Hc < 1 || Wc < 1) return "the dense descriptor map needs Hc, Wc >= 1";
  if (D < 4 || D % 4 != 0 || D > LG_WIREFRAME_MAX_DIM) return "descriptor width must be a multiple of 4 in [4, 1024]";
  if (B * Hc * Wc * D > 0x7fffffffLL * 4) return "dense descriptor map too large";
  return nullptr;
}
bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
}  // namespace

extern "C" {

int lg_wireframe_workspace_bytes(int32_t B, int32_t L, int32_t K, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (B < 0 || L < 0 || K < 0) return fail(LG_E_INVALID, "negative size");
  if (L > LG_WIREFRAME_MAX_LINES) return fail(LG_E_INVALID, "too many lines per image (LG_WIREFRAME_MAX_LINES)");
  *bytes = lg::wireframe_workspace_bytes(B, L, K);
  return LG_OK;
}

int lg_wireframe_forward(const lg_wireframe_config_t* cfg, const lg_wireframe_inputs_t* in, lg_wireframe_outputs_t* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!cfg || !in || !out) return fail(LG_E_INVALID, "null argument");
  const int64_t B = in->B, L = in->L, K = in->K, J = in->J, D = in->D;
  if (B < 0 || L < 0 || K < 0 || J < 0) return fail(LG_E_INVALID, "negative size");
  if (L > LG_WIREFRAME_MAX_LINES) return fail(LG_E_INVALID, "too many lines per image (LG_WIREFRAME_MAX_LINES)");
  if (!(cfg->nms_radius >= 0.0) || cfg->s < 1) return fail(LG_E_INVALID, "nms_radius must be >= 0 and s >= 1");
  if (const char* e = map_error(B, in->Hc, in->Wc, D)) return fail(LG_E_INVALID, e);
  const bool fill_slots = cfg->force_num_lines && cfg->merge_line_endpoints;
  if (fill_slots ? J < 2 * L : J != 2 * L)
    return fail(LG_E_INVALID, "J must be >= 2 L with force_num_lines and merged endpoints, == 2 L otherwise");
  const int64_t N = J + K;
  if (B * N * D > 0x7fffffffLL * 4 || N > 0x7fff) return fail(LG_E_INVALID, "shape too large");
  if (B == 0) return LG_OK;
  if (!in->dense || !out->counts) return fail(LG_E_INVALID, "null argument");
  if (L > 0 && (!in->lines || !in->line_scores || !out->lines || !out->lines_junc_idx))
    return fail(LG_E_INVALID, "null line argument");
  if (K > 0 && (!in->keypoints || !in->keypoint_scores || !in->descriptors)) return fail(LG_E_INVALID, "null keypoint argument");
  if (N > 0 && (!out->points || !out->scores || !out->descriptors)) return fail(LG_E_INVALID, "null output");
  if (fill_slots && J > 0 && !in->fill_junctions) return fail(LG_E_INVALID, "force_num_lines needs fill_junctions");
  if (cfg->force_num_keypoints && cfg->merge_points && K > 0 && !in->fill_keypoints)
    return fail(LG_E_INVALID, "force_num_keypoints needs fill_keypoints");
  if (!workspace || workspace_bytes < lg::wireframe_workspace_bytes(B, L, K))
    return fail(LG_E_INVALID, "workspace too small (lg_wireframe_workspace_bytes)");
  if (misaligned(workspace, 256)) return fail(LG_E_INVALID, "workspace is not 256-byte aligned");
  if (misaligned(in->dense, 16) || misaligned(in->descriptors, 16) || misaligned(out->descriptors, 16))
    return fail(LG_E_INVALID, "descriptors are not 16-byte aligned");
  if (misaligned(in->lines, 8) || misaligned(in->keypoints, 8) || misaligned(in->fill_junctions, 8) ||
      misaligned(in->fill_keypoints, 8) || misaligned(out->points, 8) || misaligned(out->lines, 8) ||
      misaligned(out->lines_junc_idx, 8))
    return fail(LG_E_INVALID, "coordinates are not 8-byte aligned");
  if (misaligned(in->line_scores, 4) || misaligned(in->keypoint_scores, 4) || misaligned(out->scores, 4) ||
      misaligned(out->counts, 4))
    return fail(LG_E_INVALID, "misaligned argument");
  if (misaligned(out->connectivity, 16) || misaligned(out->pl_associativity, 16))
    return fail(LG_E_INVALID, "bool matrices are not 16-byte aligned");
  lg::WfCall c;
  c.B = in->B, c.L = in->L, c.K = in->K, c.J = in->J, c.D = in->D, c.Hc = in->Hc, c.Wc = in->Wc, c.s = cfg->s;
  c.merge_points = cfg->merge_points != 0, c.merge_endpoints = cfg->merge_line_endpoints != 0;
  c.force_kp = cfg->force_num_keypoints != 0, c.force_lines = cfg->force_num_lines != 0;
  c.eps = cfg->nms_radius;
  c.lines = in->lines, c.line_scores = in->line_scores, c.kp = in->keypoints, c.kp_scores = in->keypoint_scores;
  c.kp_desc = in->descriptors, c.dense = in->dense, c.fill_junc = in->fill_junctions, c.fill_kp = in->fill_keypoints;
  c.points = out->points, c.scores = out->scores, c.out_desc = out->descriptors, c.new_lines = out->lines;
  c.idx = out->lines_junc_idx, c.counts = out->counts;
  c.removed = out->removed, c.conn = out->connectivity, c.pl = out->pl_associativity;
  const hipError_t e = lg::wireframe_forward(c, workspace, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("wireframe_forward: ") + hipGetErrorString(e));
  return LG_OK;
}

int lg_wireframe_connectivity(const int64_t* lines_junc_idx, int32_t B, int32_t L, int32_t N, int32_t identity_only,
                              uint8_t* out, void* stream) {
  if (B < 0 || L < 0 || N < 0) return fail(LG_E_INVALID, "negative size");
  if (N > 0x7fff) return fail(LG_E_INVALID, "shape too large");
  if (B == 0 || N == 0) return LG_OK;
  if (!out || (!identity_only && L > 0 && !lines_junc_idx)) return fail(LG_E_INVALID, "null argument");
  if (misaligned(out, 16) || misaligned(lines_junc_idx, 8)) return fail(LG_E_INVALID, "misaligned argument");
  const hipError_t e = lg::wireframe_connectivity(lines_junc_idx, B, L, N, identity_only, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("wireframe_connectivity: ") + hipGetErrorString(e));
  return LG_OK;
}

int lg_sample_descriptors_corner(const float* points, const float* dense, int32_t B, int32_t P, int32_t Hc, int32_t Wc,
                                 int32_t D, int32_t s, float* out, void* stream) {
  if (P < 0 || s < 1) return fail(LG_E_INVALID, "P must be >= 0 and s >= 1");
  if (const char* e = map_error(B, Hc, Wc, D)) return fail(LG_E_INVALID, e);
  if ((int64_t)B * P * D > 0x7fffffffLL * 4) return fail(LG_E_INVALID, "shape too large");
  if (B == 0 || P == 0) return LG_OK;
  if (!points || !dense || !out) return fail(LG_E_INVALID, "null argument");
  if (misaligned(points, 8) || misaligned(dense, 16) || misaligned(out, 16))
    return fail(LG_E_INVALID, "descriptors are not 16-byte aligned (points 8-byte)");
  const hipError_t e = lg::sample_descriptors_corner(points, dense, B, P, Hc, Wc, D, s, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("sample_descriptors_corner: ") + hipGetErrorString(e));
  return LG_OK;
}

}  // extern "C"
