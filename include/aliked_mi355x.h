/*
 * aliked_mi355x.h — C-ABI of the MI355X-native ALIKED extractor (gfx950 HIP kernels), part of
 * liblightglue_mi355x.so.
 *
 * The reference exposes this path as a Python plugin, not an FFI:
 *   gluefactory/models/extractors/aliked.py:591-786  class ALIKED(BaseModel)
 *     _init(conf)            :646-730  -> sp_aliked_create + sp_aliked_load_weights
 *     _forward(data) -> dict :765-783  -> sp_aliked_workspace_bytes + sp_aliked_forward
 * The Python drop-in (lightglue_amd.aliked.ALIKED) binds it with ctypes.
 *
 * Conventions: as lightglue_mi355x.h (caller-owned device memory, stream-ordered work, int status
 * + lg_last_error(), one handle per device, not re-entrant).  fp32 in and out.  BatchNorm is folded
 * into the convolutions at load time (running statistics, eps 1e-5).
 */
#ifndef ALIKED_MI355X_H
#define ALIKED_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sp_aliked_handle sp_aliked_handle_t;

/* ALIKED.cfgs[model_name] (aliked.py:605-642; K = 3) and the selection keys of default_conf. */
typedef struct {
  int32_t c1, c2, c3, c4;      /* encoder widths, multiples of 8, <= 128 */
  int32_t dim;                 /* descriptor width = c4: 64 or 128 */
  int32_t M;                   /* sample positions per keypoint: 16 or 32 */
  int32_t nms_radius;          /* 2 (1..8): NMS, border and soft-argmax window radius */
  int32_t max_num_keypoints;   /* k; <= 0: no limit but n_limit_max = 20000 */
  float detection_threshold;   /* <= 0 with k > 0: top-k mode; else threshold mode (aliked.py:135-158) */
} sp_aliked_config_t;

typedef struct {
  int32_t B, H, W;             /* three channels; H, W >= 8 */
  const float* image;          /* device [B,3,H,W] */
  const float* image_size;     /* device [B,2] (w,h) or NULL: the far borders sit at the true size */
} sp_aliked_inputs_t;

/* Top-k mode writes exactly k = max_num_keypoints points per image, sorted by NMS score (ties:
 * lower pixel index first), and never synchronises.  Threshold mode writes counts[b] points in
 * row-major order (the n_limit best, sorted, when more pass), reads the counts back once, and
 * zero-fills the slots past counts[b]. */
typedef struct {
  float* score_map;            /* device [B,1,H,W] */
  int32_t capacity;            /* keypoint slots per image: >= k (top-k mode), >= min(n_limit, H*W) otherwise */
  float* keypoints;            /* device [B,capacity,2]: (w,h) * (k + 1) / 2, k the DKD position in [-1,1] */
  float* descriptors;          /* device [B,capacity,dim], L2-normalised */
  float* sampled_scores;       /* device [B,capacity]: score map sampled at the refined position */
  float* dispersity;           /* device [B,capacity]: soft-argmax dispersity (aliked.py:191-199) */
  int32_t* counts;             /* device [B] */
  int32_t* host_counts;        /* host [B] or NULL; threshold mode fills it (it synchronises anyway) */
} sp_aliked_outputs_t;

int sp_aliked_create(const sp_aliked_config_t* cfg, int device, sp_aliked_handle_t** out);
int sp_aliked_destroy(sp_aliked_handle_t* h);

/* The reference's state_dict without the int64 bn.num_batches_tracked counters: fp32 device
 * tensors by name (block1..4, conv1..4, score_head.{0,2,4,6}, desc_head.*).  The load is strict, as
 * lg_load_weights: an unexpected, duplicate, wrongly sized or missing key is LG_E_WEIGHTS. */
int sp_aliked_weight_count(const sp_aliked_handle_t* h);
const char* sp_aliked_weight_name(const sp_aliked_handle_t* h, int index);
int64_t sp_aliked_weight_numel(const sp_aliked_handle_t* h, int index);
int sp_aliked_load_weights(sp_aliked_handle_t* h, int n, const char* const* names, const float* const* tensors,
                           const int64_t* numels, void* stream);

int sp_aliked_workspace_bytes(const sp_aliked_handle_t* h, int32_t B, int32_t H, int32_t W, int32_t capacity,
                              size_t* bytes);
int sp_aliked_forward(sp_aliked_handle_t* h, const sp_aliked_inputs_t* in, sp_aliked_outputs_t* out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Measurement: with profiling on, a forward records an event at each stage boundary of its stream;
 * sp_aliked_stage_ms waits for the last one and returns the five stage times in milliseconds:
 * encoder (blocks 1-2), deformable blocks (3-4), aggregation + score head, DKD, SDDH. */
int sp_aliked_set_profile(sp_aliked_handle_t* h, int32_t on);
int sp_aliked_stage_ms(sp_aliked_handle_t* h, float* ms);

/* The deformable 3x3 convolution alone (torchvision.ops.deform_conv2d, stride 1, padding 1, one
 * offset group, no mask): x [B,Cin,H,W], offset [B,18,H,W] (channel 2k = dy, 2k+1 = dx of tap k,
 * taps row-major), weight [Cout,Cin,3,3], bias [Cout] or NULL -> y [B,Cout,H,W].  Cout a multiple
 * of 32 up to 128.  scratch: device, (9 Cin + 1) * Cout floats. */
int sp_aliked_deform_conv(const float* x, const float* offset, const float* weight, const float* bias, int32_t B,
                          int32_t Cin, int32_t Cout, int32_t H, int32_t W, float* y, float* scratch,
                          size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIKED_MI355X_H */
