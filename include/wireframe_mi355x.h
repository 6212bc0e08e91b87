/* wireframe_mi355x.h -- C-ABI of the wireframe step in front of GlueStick (liblightglue_mi355x.so, gfx950).
 *
 * Replaces, on the device,
 *   gluefactory/models/lines/wireframe.py:8-19    sample_descriptors_corner_conv
 *   gluefactory/models/lines/wireframe.py:22-128  lines_to_wireframe (DBSCAN(min_samples=1) junction merge)
 *   gluefactory/models/lines/wireframe.py:185-305 WireframeExtractor._forward after the two extractors
 * The Python binding is lightglue_amd.wireframe.  Conventions as include/lightglue_mi355x.h: device
 * pointers, row-major fp32, stream-ordered and asynchronous, LG_* error codes, lg_last_error().
 * No handle: the step has no weights.
 *
 * Output layout.  Every image has J junction slots followed by K keypoint slots, N = J + K rows:
 *   rows [0, J)      junctions: the first counts[b] are the cluster means in sklearn's label order;
 *                    with force_num_lines the slots behind them take fill_junctions[b][j - counts[b]]
 *                    (score 0, descriptor sampled), without it they are left unwritten
 *   rows [J, J + K)  keypoints: with force_num_keypoints in place (a removed keypoint k takes
 *                    fill_keypoints[b][k], score 0, descriptor sampled); without it the survivors
 *                    compacted in order, counts[B + b] of them, the rows behind left unwritten
 * J must be >= 2 L with force_num_lines (2 * max_num_lines) and == 2 L without it.
 */
#ifndef WIREFRAME_MI355X_H
#define WIREFRAME_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_WIREFRAME_MAX_LINES 2048 /* endpoint coordinates and labels of one image live in LDS */
#define LG_WIREFRAME_MAX_DIM 1024   /* descriptor width: a multiple of 4 up to this */

typedef struct lg_wireframe_config_t {
  double nms_radius;            /* endpoints merge at distance <= it (fp64); keypoints go at < it (fp32) */
  int32_t merge_points;         /* remove keypoints that sit on an endpoint of the original lines */
  int32_t merge_line_endpoints; /* 0: every endpoint is its own junction */
  int32_t force_num_keypoints;  /* replace removed keypoints in place instead of compacting */
  int32_t force_num_lines;      /* fill the junction slots behind the true junctions */
  int32_t s;                    /* image pixels per cell of the dense descriptor map */
  int32_t reserved;
} lg_wireframe_config_t;

typedef struct lg_wireframe_inputs_t {
  int32_t B, L, K;             /* images, lines and keypoints per image (L, K may be 0) */
  int32_t J;                   /* junction slots per image in the outputs (see above) */
  int32_t D, Hc, Wc;           /* dense descriptor map [B][Hc][Wc][D] (NHWC) */
  int32_t reserved;
  const float* lines;          /* [B][L][2][2] */
  const float* line_scores;    /* [B][L] */
  const float* keypoints;      /* [B][K][2] */
  const float* keypoint_scores;/* [B][K] */
  const float* descriptors;    /* [B][K][D] the point extractor's descriptors */
  const float* dense;          /* [B][Hc][Wc][D] */
  const float* fill_junctions; /* [B][J][2], required with force_num_lines and merge_line_endpoints */
  const float* fill_keypoints; /* [B][K][2], required with force_num_keypoints and merge_points */
} lg_wireframe_inputs_t;

typedef struct lg_wireframe_outputs_t {
  float* points;               /* [B][J+K][2] */
  float* scores;               /* [B][J+K] */
  float* descriptors;          /* [B][J+K][D] */
  float* lines;                /* [B][L][2][2] endpoints moved to their junctions */
  int64_t* lines_junc_idx;     /* [B][L][2] */
  int32_t* counts;             /* [2][B]: true junctions, then keypoints kept */
  uint8_t* removed;            /* [B][K] 1 where a keypoint sat on an endpoint, or null */
  uint8_t* connectivity;       /* [B][J][J] bool or null */
  uint8_t* pl_associativity;   /* [B][J+K][J+K] bool or null */
} lg_wireframe_outputs_t;

int lg_wireframe_workspace_bytes(int32_t B, int32_t L, int32_t K, size_t* bytes);
/* the whole step; L above LG_WIREFRAME_MAX_LINES is refused with LG_E_INVALID */
int lg_wireframe_forward(const lg_wireframe_config_t* cfg, const lg_wireframe_inputs_t* in, lg_wireframe_outputs_t* out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* out [B][N][N] bool = identity, plus out[b][i][j] = out[b][j][i] = 1 for every line's junction pair
 * (i, j) = lines_junc_idx[b][l] unless identity_only; pairs outside [0, N) are skipped */
int lg_wireframe_connectivity(const int64_t* lines_junc_idx, int32_t B, int32_t L, int32_t N, int32_t identity_only,
                              uint8_t* out, void* stream);
/* sample_descriptors_corner_conv: bilinear (align_corners = False, zero padding) at x / s - 0.5,
 * y / s - 0.5 cells, then L2-normalised; points [B][P][2] pixels -> out [B][P][D] */
int lg_sample_descriptors_corner(const float* points, const float* dense, int32_t B, int32_t P, int32_t Hc, int32_t Wc,
                                 int32_t D, int32_t s, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
