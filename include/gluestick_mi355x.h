/* gluestick_mi355x.h -- C-ABI of the GlueStick point-and-line matcher (liblightglue_mi355x.so, gfx950).
 *
 * Replaces the reference's eval forward of
 *   gluefactory/models/matchers/gluestick.py:136-312  GlueStick._forward(data)
 *     :470-514  normalize_keypoints, KeypointEncoder, EndPtEncoder (MLPs with eval BatchNorm)
 *     :517-579  MultiHeadedAttention / AttentionalPropagation / GNNLayer (the SuperGlue trunk)
 *     :582-684  LineLayer (line_attention = False): endpoint MLP and the mean per junction
 *     :761-772  log_double_softmax
 *     :314-369  _get_matches / _get_line_matches
 * The Python binding (lightglue_amd.gluestick.GlueStick) mirrors the reference module tree, so a
 * reference state dict loads unchanged.  Conventions as include/superglue_mi355x.h: device pointers,
 * row-major fp32, stream-ordered and asynchronous, LG_* error codes, lg_last_error().
 *
 * Keypoints are [junction slots | other points]; lines_junc_idx names each line endpoint's junction
 * among them.  Indices outside [0, n_kpts) are the caller's error; the kernels clamp them, so
 * they never index out of bounds.
 */
#ifndef GLUESTICK_MI355X_H
#define GLUESTICK_MI355X_H

#include <stddef.h>
#include <stdint.h>

#include "superglue_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_GLUESTICK_MAX_LINE_ITERS 16

typedef struct sg_gluestick_config_t {
  int32_t descriptor_dim;              /* 256 (kernels are specialised) */
  int32_t n_layers;                    /* len(GNN_layers); n_layers / 2 line layers */
  int32_t layer_types[SG_MAX_LAYERS];  /* 0 "self", 1 "cross" */
  int32_t n_kenc;                      /* len(keypoint_encoder), shared by kenc and lenc */
  int32_t keypoint_encoder[SG_MAX_KENC];
  int32_t num_line_iterations;         /* line layer applications after every self layer */
  float filter_threshold;
} sg_gluestick_config_t;

typedef struct sg_gluestick_inputs_t {
  int32_t B, M, N;            /* pairs, keypoints per image */
  int32_t L0, L1;             /* lines per image (either 0: no line layers, no line head) */
  const float* keypoints0;    /* [B][M][2] pixels */
  const float* keypoints1;    /* [B][N][2] */
  const float* descriptors0;  /* [B][M][256] */
  const float* descriptors1;  /* [B][N][256] */
  const float* scores0;       /* [B][M] keypoint scores */
  const float* scores1;
  const float* image_size0;   /* [B][2] (w, h) or null: image_w0 / image_h0 (the image shape) */
  const float* image_size1;
  int32_t image_w0, image_h0, image_w1, image_h1;
  const float* lines0;              /* [B][L0][2][2] endpoints in pixels */
  const float* lines1;              /* [B][L1][2][2] */
  const int64_t* lines_junc_idx0;   /* [B][L0][2] junction (keypoint index) of each endpoint */
  const int64_t* lines_junc_idx1;   /* [B][L1][2] */
  const float* line_scores0;        /* [B][L0] */
  const float* line_scores1;        /* [B][L1] */
} sg_gluestick_inputs_t;

typedef struct sg_gluestick_outputs_t {
  int64_t* matches0;               /* [B][M] */
  int64_t* matches1;               /* [B][N] */
  float* matching_scores0;         /* [B][M] */
  float* matching_scores1;         /* [B][N] */
  float* log_assignment;           /* [B][M+1][N+1] or null */
  float* descriptors0;             /* [B][M][256] GNN output (input of final_proj) or null */
  float* descriptors1;
  /* the line head; written when L0 > 0 and L1 > 0 (then all required), untouched otherwise */
  float* line_log_assignment;      /* [B][L0+1][L1+1] */
  int64_t* line_matches0;          /* [B][L0] */
  int64_t* line_matches1;          /* [B][L1] */
  float* line_matching_scores0;    /* [B][L0] */
  float* line_matching_scores1;    /* [B][L1] */
  float* raw_line_scores;          /* [B][L0][L1] */
} sg_gluestick_outputs_t;

typedef struct sg_gluestick_handle sg_gluestick_handle_t;

int sg_gluestick_create(const sg_gluestick_config_t* cfg, int device, sg_gluestick_handle_t** out);
int sg_gluestick_destroy(sg_gluestick_handle_t* h);
/* the state-dict schema this configuration expects (BatchNorm num_batches_tracked excluded) */
int sg_gluestick_weight_count(const sg_gluestick_handle_t* h);
const char* sg_gluestick_weight_name(const sg_gluestick_handle_t* h, int i);
int64_t sg_gluestick_weight_numel(const sg_gluestick_handle_t* h, int i);
int sg_gluestick_load_weights(sg_gluestick_handle_t* h, int n, const char* const* names, const float* const* tensors,
                              const int64_t* numels, void* stream);
int sg_gluestick_workspace_bytes(const sg_gluestick_handle_t* h, int32_t B, int32_t M, int32_t N, int32_t L0,
                                 int32_t L1, size_t* bytes);
/* eval forward; M, N >= 1 (the caller handles the empty case, gluestick.py:156-188) */
int sg_gluestick_forward(sg_gluestick_handle_t* h, const sg_gluestick_inputs_t* in, sg_gluestick_outputs_t* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- the new kernels alone (kernel-level checks); scratch is allocated stream-ordered ---- */
/* One application of line layer `layer` (gnn.line_layers.<layer>) of a loaded handle to one image
 * set: X [B][n][256], line_enc [B][2L][256], idx [B][2L] -> out = X + mean-per-junction update. */
int sg_gluestick_line_update(sg_gluestick_handle_t* h, int32_t layer, const float* X, const float* line_enc,
                             const int64_t* idx, int32_t B, int32_t n, int32_t L, float* out, void* stream);
/* log_double_softmax: scores [B][M][N], bin -> out [B][M+1][N+1] */
int sg_gluestick_double_softmax(const float* scores, float bin, int32_t B, int32_t M, int32_t N, float* out,
                                void* stream);
/* raw line scores from projected descriptors md0 [B][n0][256], md1 [B][n1][256] and the endpoint
 * junctions idx0 [B][L0][2], idx1 [B][L1][2]: S = md0[idx0] md1[idx1]^T / 16, out [B][L0][L1] =
 * 0.5 max(S[a0,b0] + S[a1,b1], S[a0,b1] + S[a1,b0]) */
int sg_gluestick_line_scores(const float* md0, const float* md1, const int64_t* idx0, const int64_t* idx1, int32_t B,
                             int32_t n0, int32_t n1, int32_t L0, int32_t L1, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
