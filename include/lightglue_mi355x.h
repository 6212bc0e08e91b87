/*
 * lightglue_mi355x.h — C-ABI of the MI355X-native LightGlue matcher (gfx950 HIP kernels).
 *
 * The reference exposes this path as a Python plugin, not an FFI:
 *   gluefactory/models/matchers/lightglue.py:340-666  class LightGlue(nn.Module)
 *     __init__(conf)            :367-430  -> lg_create + lg_load_weights
 *     forward(data) -> dict     :444-579  -> lg_workspace_bytes + lg_forward
 *     filter_matches(scores,th) :321-337  -> lg_filter_matches
 *   gluefactory_nonfree/superglue.py:181-201 log_optimal_transport(scores, alpha, iters)
 *                                         -> lg_log_optimal_transport
 *   training (gluefactory/train.py:450 `loss.backward()` through torch autograd):
 *     LightGlue.forward in training mode  -> lg_train_forward (activation-saving forward)
 *     its backward                         -> lg_train_backward
 *     MatchAssignment + log double softmax
 *       (+ losses.NLLLoss) backward        -> lg_head_backward
 * The binding a maintainer adds on the reference side is in INTEGRATION.md (ctypes).
 *
 * Conventions
 *   - Every pointer argument marked "device" is caller-allocated HIP device memory on the
 *     handle's device (torch CUDA tensors on ROCm); the library never frees caller memory.
 *   - All device work is stream-ordered on `stream` (a hipStream_t; NULL = default stream).
 *     lg_forward is fully asynchronous without pruning / early stop; with them every decision
 *     stays on the device and the stream is synchronised once, at the end, to return the kept
 *     counts as host outs.
 *   - Functions return 0 on success and a negative LG_E* code on failure; lg_last_error()
 *     returns a thread-local message for the last failure on the calling thread.
 *   - A handle belongs to one device; it is not re-entrant (one forward at a time), separate
 *     handles are independent.
 *   - fp32 everywhere; indices int64 (torch.long), -1 = unmatched (lightglue.py:335-336).
 */
#ifndef LIGHTGLUE_MI355X_H
#define LIGHTGLUE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_ABI_VERSION 12

enum {
  LG_OK = 0,
  LG_E_INVALID = -1,  /* bad argument / shape (reference: assert, lightglue.py:446,481-482,528) */
  LG_E_HIP = -2,      /* HIP runtime error */
  LG_E_WEIGHTS = -3,  /* missing / mis-shaped weight tensor */
  LG_E_WORKSPACE = -4, /* workspace too small */
  LG_E_INTERNAL = -5   /* internal consistency check failed (a library bug, not a caller error) */
};

typedef struct lg_handle lg_handle_t;

/* Mirrors LightGlue.default_conf (lightglue.py:341-361); training-only keys are host-side. */
typedef struct {
  int32_t input_dim;        /* 256 */
  int32_t descriptor_dim;   /* 256 (the kernels are specialised for 256) */
  int32_t n_layers;         /* 9 */
  int32_t num_heads;        /* 4 (head_dim must be 64) */
  int32_t add_scale_ori;    /* 0/1: positional input is (x,y) or (x,y,scale,ori) */
  double depth_confidence;  /* early stop; <= 0 disables (lightglue.py:502) */
  double width_confidence;  /* point pruning; <= 0 disables (lightglue.py:503) */
  double filter_threshold;  /* match threshold, strict '>' (lightglue.py:333) */
  /* doubles: the reference keeps these as Python floats and derives thresholds in double
   * (e.g. 1 - width_confidence, :590) before the fp32 comparison. */
  int32_t precision;        /* matrix-core operand format (no reference counterpart; both are
                             * fp32-accurate):
                             *   LG_PREC_AUTO  fp16x3; run-time operands are written scaled by a
                             *                 per-tensor power of two chosen on the device, so
                             *                 any fp32 magnitude is handled without a host check
                             *   LG_PREC_X6    bf16x6
                             * LG_PREC_AUTO may carry the flag LG_PREC_ATTN_F16 (the reference's
                             * `flash: true`, lightglue.py:139-145, :229-233): self- and cross-
                             * attention of lg_forward then run in half precision -- q, k, v and
                             * the probabilities rounded to fp16 once, one fp16 MFMA per product,
                             * fp32 accumulation and softmax statistics -- while the GEMMs and the
                             * assignment stay fp16x3.  Not fp32-accurate (DESIGN.md §5 "fp16
                             * attention").  The training entry points ignore the flag.
                             * LG_PREC_AUTO may also carry LG_PREC_GEMM_F16 (the reference's
                             * `mp: true`, autocast): input_proj and every linear of the
                             * transformer layers of lg_forward then form each product as one
                             * fp16 MFMA on the high pieces of the same plane images -- operands
                             * rounded to fp16 once, fp32 accumulation, epilogues and outputs
                             * unchanged -- and the attention runs as under LG_PREC_ATTN_F16
                             * (with or without that flag).  final_proj, the assignment and the
                             * residual stream stay fp32-class.  Not fp32-accurate (DESIGN.md §5
                             * "fp16 GEMMs").  The training entry points ignore the flag. */
} lg_config_t;

/* the flags OR with LG_PREC_AUTO (and with each other) only */
enum { LG_PREC_AUTO = 0, LG_PREC_X6 = 1, LG_PREC_ATTN_F16 = 0x100, LG_PREC_GEMM_F16 = 0x400 };

typedef struct {
  int32_t B, M, N;              /* pairs, keypoints in image 0 / image 1 */
  const float* keypoints0;      /* device [B,M,2] pixels (x,y) */
  const float* keypoints1;      /* device [B,N,2] */
  const float* descriptors0;    /* device [B,M,input_dim] */
  const float* descriptors1;    /* device [B,N,input_dim] */
  const float* image_size0;     /* device [B,2] (w,h) or NULL -> min/max fallback (lightglue.py:25-26) */
  const float* image_size1;     /* device [B,2] or NULL */
  const float* scales0;         /* device [B,M] when add_scale_ori, else NULL */
  const float* oris0;           /* device [B,M] */
  const float* scales1;         /* device [B,N] */
  const float* oris1;           /* device [B,N] */
  int32_t flags;                /* OR of LG_FWD_*: per-call options (no reference counterpart) */
  /* ABI 11 -- a ragged batch (no reference counterpart): pair b has num_keypoints0[b] <= M real
   * points in image 0 and num_keypoints1[b] <= N in image 1, stored first; the rest of each slot is
   * padding whose contents are arbitrary (NaN included) and never reach a result.  Pair b then
   * gives what it gives alone at M = num_keypoints0[b], N = num_keypoints1[b].  Both NULL (a
   * zeroed struct): every slot is full.  Give both or neither.  The counts are clamped to
   * [0, capacity] on the device and never read on the host; a pair with an empty image has no
   * matches.  Padded points: matches -1, scores 0, prune 0.  Without pruning / early stop the
   * forward stays asynchronous and log_assignment keeps its [B,M+1,N+1] shape: pair b's real block
   * at i < n0, j < n1, the dustbin column at N (i < n0), the dustbin row at M (j < n1), [M,N] = 0,
   * every other entry -inf.  With pruning / early stop the kept-block convention of `kept` holds.
   * Not supported by lg_train_forward / lg_train_backward. */
  const int32_t* num_keypoints0; /* device [B] or NULL */
  const int32_t* num_keypoints1; /* device [B] or NULL */
} lg_inputs_t;

/* lg_inputs_t.flags
 *   LG_FWD_TRAINING_GATE  the module is in training mode: early stop and point pruning are off
 *                         whatever the config says (lightglue.py:502-503 `... and not self.training`)
 *   LG_FWD_CHECKPOINTED   lg_train_forward / lg_train_backward: the reference's `checkpointed`
 *                         (lightglue.py:353,515-518, torch.utils.checkpoint per transformer layer):
 *                         `saved` keeps each layer's output only (lg_train_saved_bytes_ex) and the
 *                         backward recomputes a layer's activations before differentiating it.
 *                         Pass the same flags to both calls.  ABI 9. */
enum { LG_FWD_TRAINING_GATE = 1, LG_FWD_CHECKPOINTED = 2 };

typedef struct {
  int64_t* matches0;            /* device [B,M]  (required) */
  int64_t* matches1;            /* device [B,N]  (required) */
  float* matching_scores0;      /* device [B,M]  (required) */
  float* matching_scores1;      /* device [B,N]  (required) */
  float* log_assignment;        /* device [B,M+1,N+1] or NULL (with pruning: pair b's kept block, see kept) */
  float* ref_descriptors0;      /* device [B,M,256] or NULL: final descriptors (first M' rows valid);
                                 * without pruning / early stop and with both buffers 16-byte aligned
                                 * the last layer writes them in place (no copy) */
  float* ref_descriptors1;      /* device [B,N,256] or NULL */
  int64_t* prune0;              /* device [B,M] or NULL: layer count per point (lightglue.py:511,540,564) */
  int64_t* prune1;              /* device [B,N] or NULL */
  float* layer_descriptors0;    /* device [B,L,M,256] or NULL: descriptors after every layer (the
                                 * reference's training-mode ref_descriptors, lightglue.py:521-524,
                                 * torch.stack(all_desc0, 1) at :572); needs pruning / early stop off */
  float* layer_descriptors1;    /* device [B,L,N,256] or NULL */
  int32_t* kept;                /* device [2,B] or NULL: kept points per pair after width pruning
                                 * (row 0 image 0, row 1 image 1); pair b's outputs are the first
                                 * kept[.,b] rows of ref_descriptors*, and log_assignment holds its
                                 * [kept[0,b]+1, kept[1,b]+1] block at the [M+1, N+1] strides */
  int32_t* stop;                /* device [B] or NULL: last executed layer per pair (early stop) */
  int32_t stop_layer;           /* host out: last executed layer (of pair 0) */
  int32_t kept0, kept1;         /* host out: M', N' of pair 0 after width pruning (= M, N without) */
  int32_t precision_used;       /* host out: 0 = fp16x3, 1 = bf16x6 (LG_PREC_X6), LG_PREC_ATTN_F16 =
                                 * fp16x3 with fp16 attention; LG_PREC_GEMM_F16 (with or without
                                 * LG_PREC_ATTN_F16, as configured) = fp16 GEMMs and fp16 attention */
  float* similarity;            /* device [B,M,N] or NULL: md0 md1^T of the final assignment head, the
                                 * second output of MatchAssignment.forward (lightglue.py:311,315;
                                 * the input of a Sinkhorn head, configs[4]); with pruning pair b's
                                 * kept block at the [M, N] strides.  Requesting it materialises the
                                 * similarity (bf16x6 GEMM) instead of recomputing it in the fused
                                 * assignment passes */
} lg_outputs_t;

int lg_abi_version(void);
const char* lg_last_error(void);

int lg_create(const lg_config_t* cfg, int device, lg_handle_t** out);
int lg_destroy(lg_handle_t* h);

/* Number of tensors / name / numel of the expected state dict (reference key schema,
 * lightglue.py:367-398; old 'self_attn.{i}' names are renamed host-side, :425-429). */
int lg_weight_count(const lg_handle_t* h);
const char* lg_weight_name(const lg_handle_t* h, int index);
int64_t lg_weight_numel(const lg_handle_t* h, int index);

/* Copies + repacks weights from caller device buffers (fp32, contiguous, PyTorch layouts) into
 * the handle's kernel layouts.  `names[i]` must be a schema name; every schema tensor must be
 * present exactly once (strict load).  Stream-ordered; the sources may be freed after the
 * stream reaches this point. */
int lg_load_weights(lg_handle_t* h, int n, const char* const* names, const float* const* tensors,
                    const int64_t* numels, void* stream);

/* Device scratch needed by lg_forward for this shape (bytes, 256-B aligned pieces). */
int lg_workspace_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);

/* LightGlue.forward (lightglue.py:444-579), eval mode.  Pruning / early stop work for any B
 * (the reference asserts B == 1, lightglue.py:528,533; here every pair prunes and stops on its
 * own, with the counts kept on the device) and synchronise the stream once at the end. */
int lg_forward(lg_handle_t* h, const lg_inputs_t* in, lg_outputs_t* out, void* workspace,
               size_t workspace_bytes, void* stream);

/* MatchAssignment of layer `layer` (python-style: -1 = last) on caller descriptors desc0 [B,M,256],
 * desc1 [B,N,256] (lightglue.py:306-315 followed by sigmoid_log_double_softmax :284-296):
 * log_assignment [B,M+1,N+1] (required), similarity [B,M,N] (nullable).  token_logits0/1 [B,M] /
 * [B,N] (nullable; layers 0..L-2): the token_confidence Linear before its sigmoid, which
 * TokenConfidence.loss feeds to BCEWithLogits (:108-122).  LightGlue.loss (:614-663) evaluates
 * every layer's head this way.  Stream-ordered, asynchronous.  Workspace:
 * lg_assignment_workspace_bytes. */
int lg_assignment_workspace_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);
int lg_assignment_head(lg_handle_t* h, int32_t layer, const float* desc0, const float* desc1, int32_t B,
                       int32_t M, int32_t N, float* log_assignment, float* similarity, float* token_logits0,
                       float* token_logits1, void* workspace, size_t workspace_bytes, void* stream);

/* In-library kernel timing (no reference counterpart; the reference times whole forwards with
 * CUDA events, gluefactory/utils/benchmark.py:7-33).  While enabled, lg_forward brackets every
 * launch of the profiled kernel families with hipEvents on the forward's stream and accumulates
 * the ALGORITHMIC flops / bytes of each launch.  lg_profile_read synchronises on the recorded
 * events and returns totals since the last lg_profile_enable(h, 1). */
enum { LG_KERNEL_ATTENTION = 0, LG_KERNEL_GEMM = 1, LG_KERNEL_ASSIGN = 2, LG_KERNEL_COUNT = 3 };
/* enable: 0 = off, 1 = every family, or an OR of LG_PROFILE_ONLY(k) to time only those families
 * (fewer events inside a timed region). */
#define LG_PROFILE_ONLY(k) (1 << ((k) + 1))
int lg_profile_enable(lg_handle_t* h, int enable);
int lg_profile_read(lg_handle_t* h, int kernel, double* total_ms, int64_t* launches, double* flops,
                    double* bytes);

/* filter_matches (lightglue.py:321-337 == superglue.py:288-298) on a [B,M+1,N+1] log
 * assignment.  Workspace: lg_filter_workspace_bytes. */
int lg_filter_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes);
int lg_filter_matches(const float* scores, int32_t B, int32_t M, int32_t N, double threshold,
                      int64_t* matches0, int64_t* matches1, float* scores0, float* scores1,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same on a ragged batch: num0 / num1 are device int32 [B] (clamped on the device to [0, M] /
 * [0, N], never read on the host).  The argmaxes run over pair b's real block (i < num0[b],
 * j < num1[b]) of the fixed-shape scores; padded points get -1 / 0, and so does every point of a
 * pair with an empty image.  Both NULL: lg_filter_matches; one NULL: LG_E_INVALID.  Same workspace. */
int lg_filter_matches_ragged(const float* scores, int32_t B, int32_t M, int32_t N, double threshold,
                             const int32_t* num0, const int32_t* num1, int64_t* matches0, int64_t* matches1,
                             float* scores0, float* scores1, void* workspace, size_t workspace_bytes,
                             void* stream);

/* log_optimal_transport (superglue.py:181-201): Z [B,M+1,N+1] = log-domain Sinkhorn of
 * `scores` [B,M,N] with a dustbin of score `alpha`, `iters` iterations, multiplied by M+N.
 * N <= 4096: one read of the scores per iteration with scaled column sums; synchronises the
 * stream once (4-byte underflow flag) and reruns the exact running-max kernel if any column sum
 * left the fp32 range.  N > 4096: two reads per iteration, fully asynchronous. */
int lg_sinkhorn_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes);
int lg_log_optimal_transport(const float* scores, float alpha, int32_t B, int32_t M, int32_t N,
                             int32_t iters, float* Z, void* workspace, size_t workspace_bytes,
                             void* stream);
/* The same on a ragged batch (M, N >= 1 are the capacities): pair b has num0[b] <= M rows and
 * num1[b] <= N columns, stored first; the rest of its [M][N] slot is arbitrary (NaN allowed).  The
 * counts are device int32 [B], clamped on the device and never read on the host.  Pair b gets what
 * it gets alone at its own sizes (marginals from -log(num0 + num1)), inside the fixed-shape Z: real
 * block at i < num0, j < num1, dustbin column at N (i < num0), dustbin row at M (j < num1), corner
 * [M][N], every other entry -inf.  A pair with num0 == 0 or num1 == 0 is -inf except [M][N] = 0.
 * Padded columns neither raise the underflow flag nor enter a merge; the exact rerun is ragged too.
 * Both NULL: lg_log_optimal_transport; one NULL: LG_E_INVALID.  Same workspace. */
int lg_log_optimal_transport_ragged(const float* scores, float alpha, int32_t B, int32_t M, int32_t N,
                                    const int32_t* num0, const int32_t* num1, int32_t iters, float* Z,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* how often this process reran the exact kernel after the scaled one flagged an underflow */
int64_t lg_sinkhorn_rerun_count(void);
/* test instrumentation (process-wide): on != 0 makes N <= 4096 run the exact running-max kernels
 * alone, without the scaled pass and its flag read-back; returns the previous setting */
int lg_sinkhorn_force_exact(int on);

/* Homography ground truth: gt_matches_from_homography (gluefactory/geometry/gt_generation.py:109-161
 * with warp_points_torch, geometry/homography.py:161-180), what matchers.homography_matcher computes
 * for TwoViewPipeline.loss.  Added under ABI 12 (two new entries, nothing else changes).  No handle.
 * Device inputs kp0 [B,M,2], kp1 [B,N,2], H [B,3,3], fp32; pos_th / neg_th are the reference's
 * th_positive / th_negative in pixels (squared in double, then compared in fp32, as the reference).
 * Device outputs: assignment_u8 [B,M,N] 0/1 (a torch.bool tensor's bytes), reward_or_null [B,M,N]
 * fp32 (NULL: not computed), matches0 [B,M] / matches1 [B,N] int64 (-1 unmatched, -2 ignored),
 * scores0/1 = (matches > -1) as fp32, proj_0to1 [B,M,2] = kp0 through H, proj_1to0 [B,N,2] = kp1
 * through H^-1.  H^-1 is formed on the device: the adjugate over the determinant of the fp32 H in
 * fp64, rounded once to fp32; a singular H is outside the contract (results undefined, no error).
 * Equal minima resolve to the lowest index, as torch.min; no atomics, identical results run to run.
 * Nothing of size M*N is kept besides the outputs; workspace (lg_gt_homography_workspace_bytes) is
 * 12 bytes per keypoint.  Stream-ordered, asynchronous.  LG_E_INVALID: a null pointer, a negative
 * size, M * N >= 2^31, a short workspace, a pointer off its natural alignment (8 bytes for the
 * keypoints, projections and matches: one point / one index; 4 for the rest).  B, M or N == 0: LG_OK, nothing launched, no output
 * written. */
int lg_gt_homography_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes);
int lg_gt_matches_from_homography(const float* kp0, const float* kp1, const float* H, int32_t B, int32_t M, int32_t N,
                                  double pos_th, double neg_th, uint8_t* assignment_u8, float* reward_or_null,
                                  int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* proj_0to1,
                                  float* proj_1to0, void* workspace, size_t workspace_bytes, void* stream);

/* Pose-and-depth ground truth: gt_matches_from_pose_depth (gluefactory/geometry/gt_generation.py:13-106
 * with sample_depth / project, geometry/depth.py, the Camera / Pose rows of geometry/wrappers.py and
 * sym_epipolar_distance_all, geometry/epipolar.py:59-72), what matchers.depth_matcher computes.  Two
 * more entries under ABI 12.  No handle.  Device inputs, fp32: kp0 [B,M,2], kp1 [B,N,2]; depth0
 * [B,H0,W0], depth1 [B,H1,W1] (values <= 0 mean "no depth"); cam0 / cam1 [B, 6 + n_dist] rows
 * (w, h, fx, fy, cx, cy, then k1, k2 with n_dist >= 2, then p1, p2 with n_dist == 4); T_0to1 / T_1to0
 * [B,12] rows (R row-major, then t).  pos_th / neg_th: th_positive / th_negative in pixels.
 * th_epi_or_nan / th_consistency_or_nan: NaN means None.  th_epi only switches the epipolar step on
 * (the reference compares against neg_th there); th_consistency is compared with the squared
 * round-trip distance, as the reference does.
 * valid_depth0/1_or_null both null: depth_keypoints0/1 [B,M] / [B,N] are outputs, sampled from the
 * maps.  Both given (uint8 0/1): depth_keypoints0/1 and they are the caller's precomputed depths and
 * the maps may be null, unless th_consistency is set.
 * Device outputs: those of lg_gt_matches_from_homography plus visible0_u8 [B,M], visible1_u8 [B,N]
 * (torch.bool bytes).  reward = (dist < pos_th^2) - (epi > neg_th), dist masked by visibility.
 * F is formed on the device in fp64 from the fp32 rows and rounded once.  No atomics, identical
 * results run to run, nothing of size M*N besides the outputs; workspace
 * (lg_gt_depth_workspace_bytes) is about 34 bytes per keypoint and must be 16-byte aligned.
 * Stream-ordered, asynchronous.  LG_E_INVALID: a null pointer, a negative size, M * N >= 2^31, a
 * short workspace, a pointer off its natural alignment (as above), n_dist outside {0, 2, 4}, a null
 * or empty depth map where one is needed.  B, M or N == 0: LG_OK, nothing launched, no output written. */
int lg_gt_depth_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes);
int lg_gt_matches_from_pose_depth(const float* kp0, const float* kp1, const float* depth0_or_null, int32_t H0, int32_t W0,
                                  const float* depth1_or_null, int32_t H1, int32_t W1, const float* cam0, const float* cam1,
                                  int32_t n_dist, const float* T_0to1, const float* T_1to0, int32_t B, int32_t M, int32_t N,
                                  double pos_th, double neg_th, double th_epi_or_nan, double th_consistency_or_nan,
                                  float* depth_keypoints0, float* depth_keypoints1, const uint8_t* valid_depth0_or_null,
                                  const uint8_t* valid_depth1_or_null, uint8_t* assignment_u8, float* reward_or_null,
                                  int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* proj_0to1,
                                  float* proj_1to0, uint8_t* visible0_u8, uint8_t* visible1_u8, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Line ground truth from a homography: gt_line_matches_from_homography
 * (gluefactory/geometry/gt_generation.py:409-558 with sample_pts, torch_perp_dist and
 * warp_points_torch), what matchers.homography_matcher computes with use_lines.  Seven more entries
 * under ABI 12.  No handle.  Two stages, each with its own workspace; running lg_gt_line_labels on the
 * outputs of lg_gt_line_counts_homography gives the reference's (positive, m0, m1).
 *
 * Stage A, lg_gt_line_counts_homography.  Device inputs, fp32: lines0 [B,n0,4], lines1 [B,n1,4]
 * (x1, y1, x2, y2), H [B,3,3]; h0, w0, h1, w1: the image sizes in pixels.  Endpoints are clamped to
 * the image, npts samples per line are warped into the other image (H one way, H^-1 the other, formed
 * as in lg_gt_matches_from_homography) and tested against every segment there with the reference's CPU
 * fp32 arithmetic (segment length rounded to fp16, each product and sum rounded on its own; the
 * reference's CUDA branch, which casts the operands to fp16, is not reproduced).  Device outputs, all
 * uint8: num_close_pts0 [B,n0,n1] (samples of line j close to segment i of image 0), num_close_pts1_t
 * [B,n0,n1] (samples of line i close to segment j of image 1), out_of0 [B,n1] (line j of image 1
 * leaves image 0: mean(outside) >= 1 - min_visibility_th as the reference evaluates it in fp32),
 * out_of1 [B,n0].  Nothing of size n0 * n1 * npts is kept: the workspace holds the warped samples
 * (8 npts + 32 bytes per line).
 *
 * Stage B, lg_gt_line_labels.  Device inputs, uint8: the four outputs of stage A, valid_lines0 [B,n0],
 * valid_lines1 [B,n1] (torch.bool bytes); overlap_th enters as count > npts * overlap_th evaluated as
 * the reference does (fp32).  Device outputs: positive_u8 [B,n0,n1] 0/1, line_matches0 [B,n0] /
 * line_matches1 [B,n1] int64 (-1 unmatched, -2 ignored).  The fp64 cost [B,n0,n1] lives in the
 * workspace; the assignment is lg_linear_sum_assignment's solver.
 *
 * lg_gt_line_thresholds: the two integer thresholds the kernels compare counts with: the smallest
 * count of outside samples that makes a line "out" and the smallest count above npts * overlap_th
 * (npts + 1: no count qualifies).
 *
 * Stream-ordered, asynchronous, no atomics, identical results run to run.  LG_E_INVALID: a null
 * pointer, a negative size, npts outside 2..255, n0 * n1 >= 2^31, a short or misaligned (16 bytes)
 * workspace, a pointer off its natural alignment.  B, n0 or n1 == 0: LG_OK, nothing launched, no
 * output written. */
int lg_gt_line_thresholds(int32_t npts, double min_visibility_th, double overlap_th, int32_t* out_min_count,
                          int32_t* close_min_count);
int lg_gt_line_counts_workspace_bytes(int32_t B, int32_t n0, int32_t n1, int32_t npts, size_t* bytes);
int lg_gt_line_counts_homography(const float* lines0, const float* lines1, const float* H, int32_t B, int32_t n0, int32_t n1,
                                 int32_t h0, int32_t w0, int32_t h1, int32_t w1, int32_t npts, double dist_th,
                                 double min_visibility_th, uint8_t* num_close_pts0, uint8_t* num_close_pts1_t,
                                 uint8_t* out_of0, uint8_t* out_of1, void* workspace, size_t workspace_bytes, void* stream);
int lg_gt_line_labels_workspace_bytes(int32_t B, int32_t n0, int32_t n1, size_t* bytes);
int lg_gt_line_labels(const uint8_t* num_close_pts0, const uint8_t* num_close_pts1_t, const uint8_t* out_of0,
                      const uint8_t* out_of1, const uint8_t* valid_lines0, const uint8_t* valid_lines1, int32_t B, int32_t n0,
                      int32_t n1, int32_t npts, double overlap_th, uint8_t* positive_u8, int64_t* line_matches0,
                      int64_t* line_matches1, void* workspace, size_t workspace_bytes, void* stream);

/* Line ground truth from pose and depth: gt_line_matches_from_pose_depth
 * (gluefactory/geometry/gt_generation.py:207-406 with sample_pts, sample_depth, project and
 * torch_perp_dist), what matchers.depth_matcher computes with use_lines.  Five more entries under
 * ABI 12.  No handle.  Two stages as above; running lg_gt_line_labels_visibility on the outputs of
 * lg_gt_line_counts_pose_depth gives the reference's (positive, m0, m1).
 *
 * Stage A, lg_gt_line_counts_pose_depth.  Device inputs, fp32: lines0 [B,n0,4], lines1 [B,n1,4];
 * depth0 [B,H0,W0], depth1 [B,H1,W1]; cam0, cam1 [B, 6 + n_dist] and T_0to1, T_1to0 [B,12] as in
 * lg_gt_matches_from_pose_depth.  image_h0 .. image_w1: the image sizes the out-of-image test uses; the
 * endpoints are clamped to the depth maps' sizes.  Per sample: the depth (bilinear over the map with
 * values <= 0 as NaN, the nearest sample where that is NaN, zero padding), image2cam, times the depth,
 * T.transform, cam2image, without a consistency check; visible = valid depth & cam2image's valid.  A
 * sample without depth projects to NaN and is neither outside nor close to anything; a sample that is
 * not visible counts for nothing.  Device outputs, all uint8: num_close_pts0, num_close_pts1_t
 * [B,n0,n1] and out_of0 [B,n1], out_of1 [B,n0] as above; ignore_depth0 [B,n0], ignore_depth1 [B,n1]
 * (mean(valid depth) < min_visibility_th); num_visible0 [B,n0], num_visible1 [B,n1] (visible samples
 * of the line).  The workspace holds the projected samples (8 npts + 32 bytes per line).
 *
 * Stage B, lg_gt_line_labels_visibility.  Device inputs, uint8: the eight outputs of stage A and
 * valid_lines0 / valid_lines1.  mask_close compares num_close_pts1_t[i,j] with num_visible0[i] *
 * overlap_th and num_close_pts0[i,j] with num_visible1[j] * overlap_th (fp32, as the reference);
 * out_of only makes a line unmatched; a line is ignored when it is invalid or its ignore_depth is set.
 * Outputs and workspace as lg_gt_line_labels.
 *
 * lg_gt_line_depth_thresholds: the integer thresholds the kernels compare counts with: min_close
 * [npts + 1], min_close[v] the smallest count c with float(c) > float(v) * overlap_th (npts + 1: none);
 * the smallest count of outside samples that makes a line "out"; the smallest count of samples with
 * valid depth that is not ignored.
 *
 * Stream-ordered, asynchronous, no atomics, identical results run to run.  LG_E_INVALID as for the
 * entries above, and n_dist outside {0, 2, 4} or an empty depth map.  B, n0 or n1 == 0: LG_OK, nothing
 * launched, no output written. */
int lg_gt_line_depth_thresholds(int32_t npts, double min_visibility_th, double overlap_th, int32_t* min_close,
                                int32_t* out_min_count, int32_t* valid_min_count);
int lg_gt_line_counts_pose_depth_workspace_bytes(int32_t B, int32_t n0, int32_t n1, int32_t npts, size_t* bytes);
int lg_gt_line_counts_pose_depth(const float* lines0, const float* lines1, const float* depth0, int32_t H0, int32_t W0,
                                 const float* depth1, int32_t H1, int32_t W1, int32_t image_h0, int32_t image_w0,
                                 int32_t image_h1, int32_t image_w1, const float* cam0, const float* cam1, int32_t n_dist,
                                 const float* T_0to1, const float* T_1to0, int32_t B, int32_t n0, int32_t n1, int32_t npts,
                                 double dist_th, double min_visibility_th, uint8_t* num_close_pts0, uint8_t* num_close_pts1_t,
                                 uint8_t* out_of0, uint8_t* out_of1, uint8_t* ignore_depth0, uint8_t* ignore_depth1,
                                 uint8_t* num_visible0, uint8_t* num_visible1, void* workspace, size_t workspace_bytes,
                                 void* stream);
int lg_gt_line_labels_visibility_workspace_bytes(int32_t B, int32_t n0, int32_t n1, size_t* bytes);
int lg_gt_line_labels_visibility(const uint8_t* num_close_pts0, const uint8_t* num_close_pts1_t, const uint8_t* out_of0,
                                 const uint8_t* out_of1, const uint8_t* ignore_depth0, const uint8_t* ignore_depth1,
                                 const uint8_t* num_visible0, const uint8_t* num_visible1, const uint8_t* valid_lines0,
                                 const uint8_t* valid_lines1, int32_t B, int32_t n0, int32_t n1, int32_t npts,
                                 double overlap_th, uint8_t* positive_u8, int64_t* line_matches0, int64_t* line_matches1,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Batched linear sum assignment: SciPy's scipy.optimize.linear_sum_assignment (rectangular_lsap, the
 * shortest-augmenting-path solver) for every pair of a batch, one wave per pair.  Device input: cost
 * [B,nr,nc] fp64, finite.  Device outputs: row_ind, col_ind [B, min(nr,nc)] int64, row_ind ascending.
 * The result is SciPy's own among the optimal ones: the same scan order, the same tie rule, the same
 * fp64 reduced costs.  A pair without a finite assignment gets -1 in every slot (SciPy raises).  The
 * workspace is needed (lg_linear_sum_assignment_workspace_bytes > 0) only when a pair's state,
 * 28 bytes per column and 12 per row, exceeds 64 KiB of LDS.  Stream-ordered, asynchronous.
 * LG_E_INVALID: a null pointer, a negative size, nr * nc >= 2^31, a short workspace, a pointer off
 * 8 bytes.  B, nr or nc == 0: LG_OK, nothing launched. */
int lg_linear_sum_assignment_workspace_bytes(int32_t B, int32_t nr, int32_t nc, size_t* bytes);
int lg_linear_sum_assignment(const double* cost, int32_t B, int32_t nr, int32_t nc, int64_t* row_ind, int64_t* col_ind,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Nearest-neighbour matcher: what matchers.nearest_neighbor_matcher computes
 * (gluefactory/models/matchers/nearest_neighbor_matcher.py:16-72).  Two more entries under ABI 12.
 * No handle.  Device inputs, fp32: desc0 [B,M,D], desc1 [B,N,D], 1 <= D <= 512 (16-byte aligned
 * when D is a multiple of 32, 4-byte otherwise).  flags: LG_NN_RATIO / LG_NN_DISTANCE switch the two
 * tests of find_nn on (ratio2 / dist2 are ratio_thresh^2 / distance_thresh^2 in double; they are
 * compared as fp32, as the reference's Python floats are), LG_NN_MUTUAL the mutual check.
 * num0 / num1 (nullable, together): device int32 [B] per-pair counts of a ragged batch; padded
 * points never win a neighbour search, their matches are -1 and their scores 0.
 * Device outputs: matches0 [B,M] / matches1 [B,N] int64 (-1 = none; the lowest index on exact
 * ties), scores0 / scores1 fp32 = (match > -1); similarity [B,M,N] (nullable; 0 outside a ragged
 * pair's real block); log_assignment [B,M+1,N+1] (nullable) = log_softmax over columns +
 * log_softmax over rows, last row and column 0 (-inf outside a ragged pair's real block).  With
 * both dense outputs null nothing of size M*N is written.  The products run as fp16x3 on the matrix
 * cores (error <= 2.4e-7 sum_k |a_k b_k|).  No atomics on results, identical results run to run.
 * Stream-ordered, asynchronous.  Workspace: lg_nn_workspace_bytes, 256-byte aligned.
 * LG_E_INVALID: a null required pointer, a negative size, B*M*N >= 2^31, D outside [1, 512], the ratio
 * test with M or N == 1, one of num0 / num1 alone, a short, missing or misaligned workspace, a
 * misaligned pointer.  B, M or N == 0: LG_OK, nothing launched, no output written. */
enum { LG_NN_RATIO = 1, LG_NN_DISTANCE = 2, LG_NN_MUTUAL = 4 };
int lg_nn_workspace_bytes(int32_t B, int32_t M, int32_t N, int32_t D, int32_t flags, size_t* bytes);
int lg_nn_match(const float* desc0, const float* desc1, int32_t B, int32_t M, int32_t N, int32_t D, double ratio2,
                double dist2, int32_t flags, const int32_t* num0_or_null, const int32_t* num1_or_null,
                float* similarity_or_null, float* log_assignment_or_null, int64_t* matches0, int64_t* matches1,
                float* scores0, float* scores1, void* workspace, size_t workspace_bytes, void* stream);

/* Batched match evaluation: what eval_matches_homography, eval_matches_epipolar and
 * eval_homography_dlt (gluefactory/eval/utils.py:40-91,176-196) compute from a matcher's output, for
 * every pair of a batch in one launch.  One more entry under ABI 12.  No handle, no workspace.
 * Device inputs: kpts0 [B,M,2], kpts1 [B,N,2] fp32; matches0 [B,M] int64; scores0 [B,M] fp32 (the
 * DLT's weights).  num0 / num1 (nullable, together): device int32 [B] per-pair counts of a ragged
 * batch.  Match i of pair b is live when 0 <= matches0[b,i] < num1[b] (N without counts) and
 * i < num0[b]; nothing else of a row is read, so padding may hold anything.
 * flags selects the metrics; only what a set flag names is read or written:
 *   LG_EVAL_HOMOGRAPHY  H_gt [B,9] -> hom_counts [B,3] int32: live matches, those with a symmetric
 *                       transfer error (geometry/homography.py:314-323) below 1 px, below 3 px.  The
 *                       inverse is the 3x3 adjugate inverse.
 *   LG_EVAL_EPIPOLAR    cam0, cam1 [B,6] (w,h,fx,fy,cx,cy; no undistortion), T_0to1 [B,12] (R row-major,
 *                       t) -> epi_counts [B,4] int32: live matches, those with a symmetric epipolar
 *                       distance (geometry/epipolar.py:32-56, essential, not squared) below 1e-4,
 *                       5e-4, 1e-3.
 *   LG_EVAL_DLT         H_gt, scores0, image_size0 [B,2] (w,h) -> H_dlt [B,9] fp32, the score-weighted
 *                       DLT homography (Hartley-normalised, smallest eigenvector of A^T W A by cyclic
 *                       Jacobi, H[2,2] + 1e-8 = 1), and H_error_dlt [B] fp32, its mean corner error
 *                       against H_gt.  Fewer than 4 live matches: H_dlt all +inf, the error NaN.
 * All arithmetic is fp64 on the fp32 inputs; no atomics, identical results run to run.  Rows are
 * indexed in 64 bits, so no int32 shape is too large.  Stream-ordered, asynchronous.
 * LG_E_INVALID (checked before any device work): a null required pointer, a negative size, no or
 * unknown flag bits, a set flag with one of its inputs or outputs null, one of num0 / num1 alone, a
 * pointer off its natural alignment.  B == 0 or M == 0: LG_OK, nothing launched, no output written. */
enum { LG_EVAL_HOMOGRAPHY = 1, LG_EVAL_EPIPOLAR = 2, LG_EVAL_DLT = 4 };
int lg_eval_matches(const float* kpts0, const float* kpts1, const int64_t* matches0, const float* scores0_or_null,
                    int32_t B, int32_t M, int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null,
                    const float* H_gt_or_null, const float* cam0_or_null, const float* cam1_or_null,
                    const float* T_0to1_or_null, const float* image_size0_or_null, int32_t flags,
                    int32_t* hom_counts_or_null, int32_t* epi_counts_or_null, float* H_dlt_or_null,
                    float* H_error_dlt_or_null, void* stream);

/* Batched robust homography estimation: a deterministic LO-RANSAC in place of the
 * OpenCV / PoseLib estimators behind eval_homography_robust (gluefactory/eval/utils.py:132-173), for
 * every pair of a batch in one launch.  One more entry under ABI 12.  No handle, no workspace.
 * Device inputs: kpts0 [B,M,2], kpts1 [B,N,2] fp32; matches0 [B,M] int64, or null: M == N and slot i
 * matches slot i (the estimator's m_kpts0 / m_kpts1 form).  num0 / num1 (nullable, together): device
 * int32 [B] per-pair counts of a ragged batch.  Match i of pair b is live when i < num0[b] and
 * 0 <= matches0[b,i] < num1[b] (M and N without counts); nothing else of a row is read.
 * ransac_th [B] fp32: the inlier threshold of each pair in pixels (forward transfer error, r < th).
 * Hypothesis t draws its four matches from splitmix64(splitmix64(seed) + (t << 16) + d), d = 0, 1, ...
 * (repeats skipped, at most 64 draws), whatever the pair's place in the batch; a sample with a triple
 * spanning less than min_area px^2 (twice the triangle's area) in either image, or with mixed
 * orientations, is rejected.  Hypotheses run in rounds of 256 up to max_iters; after a round that
 * raised the best minimal inlier count, 8 unweighted Hartley-normalised DLT refits (thresholds 3, 2.5,
 * 2, 1.5, 1, 1, 1, 1 times th) polish it; the run stops when done * log1p(-(c/K)^4) <=
 * log1p(-confidence) for the best polished count c >= 4 of K matches.
 * Device outputs: H [B,9] fp32 (h33 = 1); inliers [B,M] uint8 in kpts0 slot order, the classification
 * of every live match under the returned fp32 matrix (evaluated in fp64); info [B,8] int32: success,
 * num_matches, num_inliers, best_t, best_minimal_count, rounds, valid_hypotheses, 0; m_kpts [B,M,4]
 * fp32, 16-byte aligned: rows [0, num_matches) are the live matches (x0, y0, x1, y1) in slot order
 * (get_matches_scores' points), the rest is not written; H_error [B] fp32 (nullable; needs H_gt [B,9]
 * and image_size0 [B,2] (w,h)): the mean corner error against H_gt, +inf where success is 0.
 * success is 0 with fewer than 4 matches, no valid hypothesis, fewer than 4 final inliers or a
 * vanishing h33; H is then the identity and the mask all zero.
 * All arithmetic is fp64; no atomics, identical results run to run.  Stream-ordered, asynchronous.
 * LG_E_INVALID (checked before any device work): a null required pointer, a negative size, max_iters
 * outside [1, 2^30], confidence outside (0, 1), a negative min_area, one of num0 / num1 alone, H_error
 * without H_gt and image_size0, matches0 null with M != N, a pointer off its natural alignment.
 * B == 0 or M == 0: LG_OK, nothing launched, no output written.
 * lg_ransac_lds_matches: the number of matches of a pair the kernel keeps in LDS; pairs with more run
 * the same arithmetic from m_kpts in global memory (same results, slower). */
int32_t lg_ransac_lds_matches(void);
int lg_ransac_homography(const float* kpts0, const float* kpts1, const int64_t* matches0_or_null, int32_t B, int32_t M,
                         int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null, const float* ransac_th,
                         int32_t max_iters, double confidence, uint64_t seed, double min_area,
                         const float* H_gt_or_null, const float* image_size0_or_null, float* H, uint8_t* inliers,
                         int32_t* info, float* m_kpts, float* H_error_or_null, void* stream);

/* Batched robust homography estimation from point and line matches: a deterministic hybrid LO-RANSAC
 *  in place of the reference's PointLineHomographyEstimator (robust_estimators/
 * homography/homography_est.py), which eval_homography_robust uses for the superpoint+lsd+gluestick
 * configs, for every pair of a batch in one launch.  Two more entries under ABI 12.  No handle, no
 * workspace.
 * Device inputs: the points and their counts are lg_ransac_homography's.  lines0 [B,L0,2,2], lines1
 * [B,L1,2,2] fp32, 16-byte aligned: the endpoints (x, y) of every segment; line_matches0 [B,L0] int64,
 * or null: L0 == L1 and slot i matches slot i.  num_lines0 / num_lines1 (nullable, together): device
 * int32 [B].  Line i of pair b is live when i < num_lines0[b], 0 <= line_matches0[b,i] < num_lines1[b]
 * and both segments are at least min_line_length px long.  Either set may be empty (M == 0 or
 * L0 == 0; its pointers may then be null).  K = live points + live lines; feature i is point i below
 * the number of live points, else a line.
 * One similarity per image (mean to the origin, mean distance sqrt 2, over the live points and both
 * endpoints of the live lines) is fixed for the whole run; the search runs in these coordinates with
 * th_n = s1 * th.  An image-1 segment enters only as its line (a, b, c), a^2 + b^2 = 1, whatever the
 * order of its endpoints; no endpoint correspondence is assumed.  Hypothesis t draws four features
 * with lg_ransac_homography's sampler over K; two points with two lines is rejected (degenerate);
 * the 8x9 system (two rows per point, one row per image-0 endpoint of a line) is reduced by
 * Gauss-Jordan with complete pivoting, a pivot not above 1e-12 of the largest entry rejects the
 * sample.  A point is an inlier by its forward transfer error, a line when both mapped image-0
 * endpoints lie within the threshold of the image-1 line; a line counts once.  Rounds, the 8 local
 * optimisation steps (unweighted DLT on the selected features in the fixed frame) and the stopping
 * rule are lg_ransac_homography's over K.
 * Device outputs: H [B,9] fp32 (h33 = 1); inliers [B,M], line_inliers [B,L0] uint8 in slot order, the
 * classification in pixels of every live feature under the returned fp32 matrix (evaluated in fp64);
 * info [B,12] int32: success, num_point_matches, num_line_matches, num_point_inliers,
 * num_line_inliers, best_t, best_minimal_count, rounds, valid_hypotheses, 0, 0, 0; m_kpts [B,M,4] as
 * lg_ransac_homography; m_lines [B,L0,8] fp32, 16-byte aligned: rows [0, num_line_matches) are the
 * live lines (a0, b0, a1, b1) in slot order, the rest is not written; H_error [B] as
 * lg_ransac_homography.  success is 0 with K < 4, no valid hypothesis, fewer than 4 final inliers in
 * total or a vanishing h33; H is then the identity and both masks all zero.
 * With L0 == 0 this is still the general solver without lg_ransac_homography's area test: the two
 * entries agree in what they find, not bit for bit.
 * All arithmetic is fp64; no atomics, identical results run to run.  Stream-ordered, asynchronous.
 * LG_E_INVALID (checked before any device work): a null required pointer (ransac_th, H, info; the
 * point arrays when M > 0, the line arrays when L0 > 0), a negative size, max_iters outside [1, 2^30],
 * confidence outside (0, 1), a negative or non-finite min_line_length, one of a pair of counts alone,
 * H_error without H_gt and image_size0, matches0 null with M != N, line_matches0 null with L0 != L1,
 * a pointer off its natural alignment.
 * B == 0 or M == L0 == 0: LG_OK, nothing launched, no output written.
 * lg_ransac_lines_lds_capacity: the numbers of point and of line matches of a pair the kernel keeps in
 * LDS; a set with more is read from m_kpts / m_lines in global memory (same results, slower). */
int lg_ransac_lines_lds_capacity(int32_t* points, int32_t* lines);
int lg_ransac_homography_lines(const float* kpts0, const float* kpts1, const int64_t* matches0_or_null, int32_t B,
                               int32_t M, int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null,
                               const float* lines0, const float* lines1, const int64_t* line_matches0_or_null, int32_t L0,
                               int32_t L1, const int32_t* num_lines0_or_null, const int32_t* num_lines1_or_null,
                               const float* ransac_th, int32_t max_iters, double confidence, uint64_t seed,
                               double min_line_length, const float* H_gt_or_null, const float* image_size0_or_null,
                               float* H, uint8_t* inliers, uint8_t* line_inliers, int32_t* info, float* m_kpts,
                               float* m_lines, float* H_error_or_null, void* stream);

/* Batched robust relative pose: a deterministic five-point LO-RANSAC in place of the
 * OpenCV / PoseLib / pycolmap estimators behind eval_relative_pose_robust (gluefactory/eval/utils.py:
 * 94-129), for every pair of a batch in one launch.  Two more entries under ABI 12.  No handle; the
 * call makes and frees a stream-ordered allocation of 180 KiB per pair.
 * kpts0, kpts1, matches0, num0 / num1, the live matches, their order, the sampler (five indices per
 * sample), max_iters, confidence and seed are lg_ransac_homography's.  camera0, camera1 [B,4] fp32:
 * fx, fy, cx, cy; a point is ((x - cx) / fx, (y - cy) / fy, 1), distortion is ignored.  ransac_th [B]
 * fp32 in pixels: the kernel compares Sampson distances in normalised coordinates with th_n = th /
 * mean(fx0, fy0, fx1, fy1).  Samples run in rounds of 256 up to max_iters: Nistér's five-point solver
 * gives up to 10 essential matrices per sample and every one is scored against every match; after a
 * round that raised the best minimal inlier count, 8 unweighted linear eight-point fits (thresholds 3,
 * 2.5, 2, 1.5, 1, 1, 1, 1 times th_n), each projected onto the essential manifold, polish it; the run
 * stops when done * log1p(-(c/K)^5) <= log1p(-confidence) for the best polished count c >= 5 of K.
 * The kept matrix is decomposed and the (R, t) with the most inliers in front of both cameras wins.
 * Device outputs: R [B,9], t [B,3] (unit norm) fp32; inliers [B,M] uint8 in kpts0 slot order: under
 * E = [t]x R of those fp32 values, evaluated in fp64, "Sampson inlier and both depths positive";
 * info [B,8] int32: success, num_matches, num_inliers, best_t, best_minimal_count, rounds,
 * valid_samples, candidates_scored; m_kpts [B,M,4] fp32, 16-byte aligned, as lg_ransac_homography;
 * errors [B,3] fp32 (nullable; needs T_gt [B,12], R row-major then t): t_err, r_err and their maximum
 * in degrees (geometry/epipolar.py:127-155), +inf where success is 0.
 * success is 0 with fewer than 5 matches, no candidate, fewer than 5 final inliers or no inlier in
 * front of both cameras; R is then the identity, t zero and the mask all zero.
 * All arithmetic is fp64; no atomics, identical results run to run.  Stream-ordered, asynchronous.
 * LG_E_INVALID (checked before any device work): a null required pointer, a negative size, max_iters
 * outside [1, 2^30], confidence outside (0, 1), one of num0 / num1 alone, errors without T_gt,
 * matches0 null with M != N, a pointer off its natural alignment.
 * B == 0 or M == 0: LG_OK, nothing launched, no output written.
 * lg_essential_5pt (kernel-level entry, tests): the solver alone, one sample per thread.  pts [S,5,4]
 * fp32 normalised (x0, y0, x1, y1); E [S,10,9] fp64: the sample's candidates (row-major, unit
 * Frobenius norm, ascending z), count [S] int32 of them; nothing past count is written. */
int lg_ransac_relpose(const float* kpts0, const float* kpts1, const int64_t* matches0_or_null, int32_t B, int32_t M,
                      int32_t N, const int32_t* num0_or_null, const int32_t* num1_or_null, const float* camera0,
                      const float* camera1, const float* ransac_th, int32_t max_iters, double confidence, uint64_t seed,
                      const float* T_gt_or_null, float* R, float* t, uint8_t* inliers, int32_t* info, float* m_kpts,
                      float* errors_or_null, void* stream);
int lg_essential_5pt(const float* pts, int32_t S, double* E, int32_t* count, void* stream);

/* Kernel-level entry (tests; the reference has no counterpart -- it is the SDPA call at
 * lightglue.py:139-149 in isolation): one launch of the forward's attention kernel.
 * q, k, v: fp32 head-major [B][H][Nq or Nk][64] device tensors, H * 64 == 256; ctx: fp32
 * [B][Nq][256] (column h*64 + d), softmax(scale * q k^T) v.  precision LG_PREC_AUTO runs the fp16x3
 * kernel (k and v range-scaled on the device), LG_PREC_X6 the bf16x6 one, LG_PREC_ATTN_F16 (alone or
 * with LG_PREC_AUTO) the fp16 attention on the fp16x3 kernel's planes.  Synchronises the
 * stream before returning.  Workspace: lg_attention_workspace_bytes. */
int lg_attention_workspace_bytes(int32_t B, int32_t H, int32_t Nq, int32_t Nk, size_t* bytes);
int lg_attention(const float* q, const float* k, const float* v, int32_t B, int32_t H, int32_t Nq,
                 int32_t Nk, float scale, int32_t precision, float* ctx, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Kernel-level entry (tests; the reference's counterpart is one nn.Linear with what the forward
 * fuses behind it): one launch of the inference linear GEMM -- gemm_h3 (fp16x3, LG_PREC_AUTO) or
 * gemm_x6 (bf16x6, LG_PREC_X6) -- on plain fp32 device tensors, prepared inside the workspace the
 * way the forward prepares them.
 *   Y = epilogue([A0 | A1] W^T + bias), A0 [R][K0] (row stride lda0), A1 [R][K-K0] (lda1; null when
 *   K0 == K), W [Nout][K] (PyTorch Linear layout), bias [Nout] (nullable for LG_LIN_STORE / LN).
 * fp16x3 preparation: a zeroed range table; max|A0|, max|A1| each into a slot of its own; each half
 * written as a plane image with its own range exponent; the weight planes as at load time (scaled
 * by 2^sw, max|W 2^sw| in [8, 16)); the output range bound from the weight's largest row L1 norm,
 * max|bias| and max|res| (LG_LIN_LN_GELU: the LayerNorm bound; QKV: keys one-sided, values
 * two-sided, as the forward builds them).
 * epi:
 *   LG_LIN_STORE      Y = relu?(res + (acc + bias) * out_scale); rows >= res2_row0 read res2 (when
 *                     set), rows >= y2_row0 go to Y2 (when set).  fp32 rows (Y) and / or a plane
 *                     image (want_planes: raw into yp, decoded into yp_rows).
 *   LG_LIN_LN_GELU    GELU(LayerNorm_512(acc + bias) * ln_g + ln_b) as a plane image (yp, yp_rows);
 *                     Nout == 512.  ln_route 0: the fused epilogue; 1: LG_LIN_STORE into fp32 and
 *                     the LayerNorm + GELU row kernel (which does not look at the row mask).
 *   LG_LIN_QKV_ROT    Nout == 768: q fp32 head-major [set][b][h][n][64] (rotary), k planes (rotary),
 *                     v planes; cosb / sinb [R][32] (both null: no rotary).
 *   LG_LIN_CROSS_QKV  Nout == 512: qk * qk_scale as planes (kp) and, when q is set, fp32 rows;
 *                     v planes.
 *   QKV: R == B * (M + N), H * 64 == 256, W and bias rows in the packed order c' = t*256 + h*64 + j,
 *   j < 32 -> dim 2j, j >= 32 -> dim 2(j-32)+1; kp / vp hold 2 fp16 planes (keys h, l*2^11; values
 *   h, l; times 2^exp) or 3 bf16 planes (h, m, l), pstride elements apart (>= R * 256).
 * Row mask (cnt non-null): segments {mask_B, mask_M0, mask_N0} with mask_B * (M0 + N0) == R, live
 * rows local < cnt[segment] and (sel null or sel[pair] == sel_eq).  Dead rows are never written.
 * poison: after the A plane images are built, their dead and padding rows are filled with finite
 * fp16 garbage of magnitude ~6e4 (stale workspace must not reach a live result).
 * LG_PREC_X6 has no plane images: yp is not written, yp_rows receives the fp32 result; ln_route and
 * poison are ignored, and the exponents come back 0.
 * Host outputs: the range exponents of the A0 / A1 images, the output planes and the value planes,
 * the recorded max |x| of the output / value planes, and bound_out (LG_LIN_LN_GELU: the LayerNorm
 * bound the output exponent was chosen from).
 * LG_E_INVALID (nothing launched, nothing written): Nout % 256, K % 32, K0 % 32, K0 <= 0 or > K,
 * A1 null with K0 < K, a missing required pointer, lda / ldr / ldy not a multiple of 4 or a pointer
 * off 16 bytes, an epilogue's shape rule.  LG_E_WORKSPACE: workspace smaller than
 * lg_linear_workspace_bytes.  Synchronises the stream before returning. */
enum { LG_LIN_STORE = 0, LG_LIN_QKV_ROT = 1, LG_LIN_CROSS_QKV = 2, LG_LIN_LN_GELU = 3 };
typedef struct {
  int32_t R, K0, K, Nout;
  const float* A0;
  int32_t lda0;
  const float* A1;
  int32_t lda1;
  const float* W;
  const float* bias;
  const float* res;             /* [.][ldr] or NULL */
  const float* res2;
  int32_t res2_row0, ldr;
  float out_scale;
  int32_t relu;
  int32_t precision;            /* LG_PREC_AUTO | LG_PREC_X6 | LG_PREC_GEMM_F16 (the fp16x3 preparation
                                 * and outputs, each product one fp16 MFMA on the high planes) */
  int32_t epi;                  /* LG_LIN_* */
  int32_t ln_route;
  const float* ln_g;            /* [512] */
  const float* ln_b;
  int32_t B, H, M, N;           /* head layout (QKV) */
  const float* cosb;
  const float* sinb;
  float qk_scale;
  int32_t mask_B, mask_M0, mask_N0;
  const int32_t* cnt;           /* device [2 * mask_B] or NULL: every row live */
  const int32_t* sel;           /* device [mask_B] or NULL */
  int32_t sel_eq;
  int32_t poison;
  int32_t want_planes;
  float* Y;                     /* [.][ldy] or NULL */
  float* Y2;
  int32_t y2_row0, ldy;
  void* yp;                     /* raw plane image: 2 planes [Nout / 32][rows_pad][32] fp16, rows_pad = R rounded up to 256 */
  float* yp_rows;               /* [R][Nout] or NULL: the plane image decoded */
  float* q;                     /* [R][256] head-major */
  void* kp;
  void* vp;
  int64_t pstride;
  int32_t exp_a0, exp_a1, exp_out, exp_out_v; /* host out */
  float max_out, max_out_v, bound_out;        /* host out */
} lg_linear_args_t;
int lg_linear_workspace_bytes(int32_t R, int32_t K0, int32_t K, int32_t Nout, size_t* bytes);
int lg_linear(lg_linear_args_t* args, void* workspace, size_t workspace_bytes, void* stream);
/* fp32 rows x [R][K] -> plane image (range exponent chosen on the device from max|x|, held to
 * 2^(15 - lshift); two_sided: small tensors are scaled up too) -> fp32 rows out [R][K].
 * *exponent (host): the exponent the planes were written with.  K % 32 == 0.  Allocates its own
 * scratch; synchronises the stream. */
int lg_plane_roundtrip(const float* x, int32_t R, int32_t K, int32_t lshift, int32_t two_sided, float* out,
                       int32_t* exponent, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel-level checks of the SuperPoint convolutions (tests; the reference's counterpart is one
 * nn.Conv2d(3x3, padding 1) + ReLU, the open model's BatchNorm as an affine, and max_pool2d(2)):
 * one launch of sp_conv3x3 -- or, with conv1a, of sp_conv1a -- on plain fp32 device tensors,
 * prepared inside the workspace the way sp_load_weights and sp_forward prepare them.  No handle.
 * Additive: the ABI version does not move.
 *   x           [B][H][W][Cin] (NHWC rows); conv1a: the image [B][Cin][H][W], Cin = 1 or 3 (RGB is
 *               reduced to gray first), and Cout == 64
 *   w           [Cout][Cin][3][3] (conv1a: [64][1][3][3]), bias [Cout]
 *   post_scale, post_shift  [Cout], both or neither: y = relu(conv + bias) * s + t before the pool
 *   pool        2x2 max-pool (floor) fused behind it (not for conv1a)
 * Preparation: a zeroed range table; max|x| into a slot; x as a plane image with a two-sided range
 * exponent chosen from it (rows past B*H*W zeroed: the taps outside the image read one of them); the
 * weight repacked to [Cout][9 Cin], split into planes of W * 2^sw (max|W 2^sw| in [8, 16)); the
 * output range bound g M[x] + max|bias| from the weight's largest row L1 norm g, with the affine
 * max|s| (g M[x] + max|bias|) + max|t|.  The route (halo tiles, or the per-tap gather under
 * LG_SP_CONV=gather) is the one sp_conv3x3 reads from the environment at launch.
 * Outputs: y_planes, the raw output image: 2 planes [Cout / 32][yrows_pad][32] fp16 (h, l * 2^11;
 * times 2^exp_out), rout live rows, both from sp_conv_layer_rows; y_rows [rout][Cout] (nullable), the
 * image decoded; on the host (nullable) the exponents the input and output images were written with
 * and the recorded max|y|.  Rows [rout, yrows_pad) of y_planes are never written.
 * LG_E_INVALID (nothing launched, nothing written): a null required pointer, a non-positive size,
 * Cin % 32, Cout % 64, pool with H < 2 or W < 2, post_scale without post_shift (or the reverse), a
 * pointer off 16 bytes; conv1a: Cin not 1 or 3, Cout != 64, pool.  LG_E_WORKSPACE: workspace smaller
 * than sp_conv_layer_workspace_bytes.  Synchronises the stream before returning. */
typedef struct {
  int32_t B, H, W, Cin, Cout;
  int32_t pool, conv1a;
  const float* x;
  const float* w;
  const float* bias;
  const float* post_scale;      /* [Cout] or NULL */
  const float* post_shift;
  float* y_rows;                /* [rout][Cout] or NULL */
  void* y_planes;               /* 2 * yrows_pad * Cout fp16 */
  int32_t* exp_in;              /* host out (nullable); conv1a: 0 */
  int32_t* exp_out;
  float* max_out;
} sp_conv_layer_args_t;
int sp_conv_layer_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pool,
                                  int32_t conv1a, size_t* bytes);
/* rows of the output image: *rout live ones, *yrows_pad allocated (a multiple of 256, > *rout) */
int sp_conv_layer_rows(int32_t B, int32_t H, int32_t W, int32_t pool, int64_t* rout, int32_t* yrows_pad);
int sp_conv_layer(const sp_conv_layer_args_t* args, void* workspace, size_t workspace_bytes, void* stream);
/* The two dense-head kernels alone (stream-ordered, asynchronous).
 * sp_head_scores: logits [B * Hc * Wc][ld] (ld >= 65, 65 used) -> softmax over the 65 without the
 * dustbin, unfolded: scores [B][8 Hc][8 Wc], scores[b][8y + dy][8x + dx] = p[cell (y, x)][8 dy + dx].
 * sp_head_normalize: rows of 256 -> x / max(|x|_2, 1e-12) (in place allowed). */
int sp_head_scores(const float* logits, int32_t ld, int32_t B, int32_t Hc, int32_t Wc, float* scores, void* stream);
int sp_head_normalize(const float* x, int32_t rows, float* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel-level checks of the assignment head (lightglue.py:284-296, 306-315, 321-337): the dual
 * softmax and the mutual filter alone, on the caller's matching descriptors md0 [B][M][256] /
 * md1 [B][N][256], matchability logits z0 [B][M] / z1 [B][N] and (nullable, device) per-pair counts.
 * No handle, no weights.  Additive: the ABI version does not move.
 * route:
 *   LG_ASSIGN_MATERIALISED  sim = md0 md1^T by the bf16x6 GEMM, then the streaming assignment kernels:
 *                           what lg_assignment_head and the pruned forward run.  With `sim` [B][M][N]
 *                           given the GEMM is skipped (md0 / md1 may be null) and the kernels read it.
 *   LG_ASSIGN_RECOMPUTED    the default eval route: md as the two-plane fp16 image the final_proj
 *                           epilogue writes (one range slot, held to 2^4; rows_pad = B (M + N) rounded
 *                           up to 256, plus 256), the similarity recomputed in two fp16x3 passes.  The
 *                           image's exponent comes from the MEASURED max |md| (the forward predicts a
 *                           bound from its weights instead, which is never smaller).  M % 16 == 0,
 *                           N % 16 == 0; counts only with `fixed`.
 * Counts (Mb, Nb [B], both or neither): clamped to [0, M] / [0, N]; an empty side empties the pair, as
 * the forward does for a ragged batch.  fixed = 1: la keeps the [M+1][N+1] shape (real block, dustbin
 * column at N, dustbin row at M, [M][N] = 0, everything else -inf); fixed = 0 (materialised only): la
 * holds pair b's [Mb+1][Nb+1] block at the capacity strides and nothing else is written.  Outputs of
 * rows >= Mb[b] / columns >= Nb[b] are never written.  raw_counts = 1 (counted materialised route
 * only): the counts are clamped but a one-sided zero is kept -- what width pruning can leave; such a
 * pair gets m = -1, s = 0 on its live side.  md rows past the counts must be finite (they are part
 * of the measured maximum); nothing else of them reaches a result.
 * poison: la / m0 / m1 / s0 / s1 are first filled with LG_ASSIGN_SENTINEL_F / _I; the plane-image rows
 * past B (M + N) and, with counts, past each pair's counts are overwritten with fp16 NaN / Inf bit
 * patterns before the launch (materialised from md with counts: the entries of sim outside each
 * pair's block).  la is nullable.  Host outputs: exp_md, the exponent the planes were written with,
 * and max_md (recomputed route; 0 otherwise).
 * LG_E_INVALID (nothing launched, nothing written): a null required pointer, a non-positive size,
 * B (M+1) (N+1) >= 2^31, Mb without Nb, fixed or raw_counts without counts, and on the recomputed
 * route M % 16, N % 16, counts without fixed, a given sim.  LG_E_WORKSPACE: workspace smaller than
 * lg_assign_workspace_bytes.  Synchronises the stream before returning. */
enum { LG_ASSIGN_MATERIALISED = 0, LG_ASSIGN_RECOMPUTED = 1 };
#define LG_ASSIGN_SENTINEL_F (-123.456f)
#define LG_ASSIGN_SENTINEL_I (-77)
typedef struct {
  int32_t B, M, N;
  const float* md0;
  const float* md1;
  const float* sim;             /* [B][M][N] or NULL */
  const float* z0;
  const float* z1;
  const int32_t* Mb;            /* device [B] or NULL */
  const int32_t* Nb;
  int32_t fixed;
  int32_t raw_counts;
  float threshold;
  int32_t route;                /* LG_ASSIGN_* */
  int32_t poison;
  float* la;                    /* [B][M+1][N+1] or NULL */
  int64_t* m0;                  /* [B][M] */
  int64_t* m1;                  /* [B][N] */
  float* s0;
  float* s1;
  int32_t exp_md;               /* host out */
  float max_md;                 /* host out */
} lg_assign_args_t;
int lg_assign_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes);
int lg_assign(lg_assign_args_t* args, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training: the backward pass of LightGlue (the reference differentiates its forward with torch
 * autograd: gluefactory/train.py:436-450 over lightglue.py:444-579 and :614-663).  No reference
 * counterpart as an interface; these entry points are what a torch.autograd.Function binds.
 *
 * Parameters are passed as raw fp32 device pointers in the state-dict schema order
 * (lg_weight_name(h, i), i < lg_weight_count(h)) in the reference's own layouts (Wqkv
 * [768,256] with rows h*192 + d*3 + t, lightglue.py:185, ...), and gradients come back in the same
 * order and layouts: `grads[i]` (device, numel lg_weight_numel(h, i)) is overwritten when non-null;
 * entries a call does not own are left untouched.  All arithmetic is fp32 (f32-input matrix cores).
 *
 * lg_train_forward: the training-mode forward (no pruning / early stop, :502-503) that keeps every
 * activation its backward needs in `saved` (lg_train_saved_bytes; caller-owned, pass the same
 * buffer to lg_train_backward) and writes every layer's descriptors to
 * layer_descriptors0/1 [B,L,M,256] / [B,L,N,256] (the training-mode ref_descriptors, :521-524,572).
 * lg_train_backward: given d(loss)/d(layer_descriptors0/1) (nullable: zero), writes the gradients of
 * input_proj.*, posenc.*, transformers.* (grads) and of the input descriptors grad_desc0/1
 * [B,M,input_dim] / [B,N,input_dim] (nullable).  Scratch: lg_train_scratch_bytes.  Both are
 * stream-ordered and asynchronous; the dQ sums of the attention backward use float atomics, so
 * repeated calls may differ in the last bits.
 */
int lg_train_saved_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);
/* the same for the lg_inputs_t.flags a training call will get (LG_FWD_CHECKPOINTED: ~one layer's
 * activations plus one [B*(M+N),256] output per layer instead of every layer's).  ABI 9. */
int lg_train_saved_bytes_ex(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, int32_t flags, size_t* bytes);
/* Data-parallel training (gluefactory/train.py:307-309, DistributedDataParallel): the backward
 * reports when gradients are final, so a caller can start each gradient bucket's all-reduce
 * while the rest of the backward still runs (DDP's overlap).  `fn` is called on the calling
 * thread, from inside lg_train_backward, right after the kernels that finish layer `layer`'s
 * gradients (transformers.<layer>.*) are enqueued on `stream` -- layers count down L-1 .. 0 --
 * and once more with layer = -1 after the rest (input_proj.*, posenc.*).  Work the callback
 * enqueues must be ordered after `stream`'s work so far (record an event on it).  fn = NULL
 * removes the hook.  ABI 8. */
typedef void (*lg_grad_ready_fn)(void* ctx, int32_t layer, void* stream);
int lg_set_grad_ready_hook(lg_handle_t* h, lg_grad_ready_fn fn, void* ctx);
int lg_train_scratch_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);
int lg_train_forward(lg_handle_t* h, const float* const* params, const lg_inputs_t* in, float* layer_descriptors0,
                     float* layer_descriptors1, void* saved, size_t saved_bytes, void* stream);
int lg_train_backward(lg_handle_t* h, const float* const* params, const lg_inputs_t* in, const void* saved,
                      size_t saved_bytes, const float* grad_layer_descriptors0, const float* grad_layer_descriptors1,
                      float* const* grads, float* grad_desc0, float* grad_desc1, void* scratch, size_t scratch_bytes,
                      void* stream);

/* Backward of MatchAssignment `layer` (python-style index) on desc0 [B,M,256] / desc1 [B,N,256]
 * (lightglue.py:306-315 and sigmoid_log_double_softmax :284-296), recomputing what it needs.
 * The gradient of the log assignment is `la_grad` [B,M+1,N+1] scaled per pair: s_in[b] on the
 * inner block, s_dust[b] on the dustbin row / column (s_in / s_dust nullable = 1; the corner is
 * ignored).  Plain autograd passes d(loss)/d(log_assignment) with both null; the fused NLL backward
 * (losses.py:6-58: nll = bal * nll_pos + (1 - bal) * nll_neg, linear in la) passes the NLLLoss
 * weights [B,M+1,N+1] with s_in = -g bal / num_pos, s_dust = -g (1 - bal) / (num_neg0 + num_neg1),
 * so no dense gradient tensor is formed.  grad_similarity [B,M,N] (nullable) adds
 * d(loss)/d(similarity) for callers that use MatchAssignment's second output.  grad_token0/1
 * [B,M] / [B,N] (nullable; layers 0..L-2): d(loss)/d(token_confidence logits); TokenConfidence.loss
 * detaches its inputs (:109-110), so they reach only token_confidence.<layer>.token.0.*.
 * Writes the grads of log_assignment.<layer>.* (and token_confidence.<layer>.* when grad_token* is
 * given) and grad_desc0/1 (nullable).  Scratch: lg_head_scratch_bytes.  Asynchronous. */
int lg_head_scratch_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);
/* The same head's forward on raw parameters, fp32 (f32 matrix cores): log_assignment [B,M+1,N+1],
 * similarity [B,M,N] (nullable), token_logits0/1 (nullable) -- lg_assignment_head's outputs without
 * the handle's packed weights (the training path never uploads them).  Scratch:
 * lg_head_scratch_bytes.  Asynchronous. */
int lg_head_forward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0, const float* desc1,
                    int32_t B, int32_t M, int32_t N, float* log_assignment, float* similarity, float* token_logits0,
                    float* token_logits1, void* scratch, size_t scratch_bytes, void* stream);
int lg_head_backward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0, const float* desc1,
                     int32_t B, int32_t M, int32_t N, const float* la_grad, const float* s_in, const float* s_dust,
                     const float* grad_similarity, const float* grad_token0, const float* grad_token1,
                     float* const* grads, float* grad_desc0, float* grad_desc1, void* scratch, size_t scratch_bytes,
                     void* stream);
/* A loss head (LightGlue.loss, lightglue.py:614-663) without its log assignment in memory: the
 * NLL terms out[5][B] of lg_head_forward's log assignment against the ground truth (exactly
 * sg_nll_loss's layout, modes and fp64 sums: nll, nll_pos, nll_neg, num_matchable,
 * num_unmatchable; mode 1 needs M == N) and its argmaxes -- argmax0 [B,M] (int64) over the N + 1
 * columns of rows < M, argmax1 [B,N] over the M + 1 rows of columns < N, first maximum on ties,
 * what TokenConfidence.loss takes (:108-122) -- plus the token logits (nullable).  Leaves md / z /
 * similarity / LSEs in `scratch` like lg_head_forward (lg_head_backward_from_forward reads them).
 * N <= 4096.  ABI 9. */
int lg_head_nll_forward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0, const float* desc1,
                        int32_t B, int32_t M, int32_t N, const uint8_t* gt_assignment, const int64_t* gt_matches0,
                        const int64_t* gt_matches1, int32_t mode, float balancing, float* out, int64_t* argmax0,
                        int64_t* argmax1, float* token_logits0, float* token_logits1, void* scratch, size_t scratch_bytes,
                        void* stream);
/* lg_head_backward without the recompute: `scratch` is the buffer the matching lg_head_forward
 * call used (same handle, params, layer, desc0/1, B, M, N; similarity == NULL there), left
 * untouched since -- it still holds md, z, the similarity and its row / column log-sum-exps,
 * which the backward then reads instead of recomputing (the autograd semantics of a saved
 * activation).  ABI 9. */
int lg_head_backward_from_forward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0,
                                  const float* desc1, int32_t B, int32_t M, int32_t N, const float* la_grad,
                                  const float* s_in, const float* s_dust, const float* grad_similarity,
                                  const float* grad_token0, const float* grad_token1, float* const* grads,
                                  float* grad_desc0, float* grad_desc1, void* scratch, size_t scratch_bytes,
                                  void* stream);

/* The fused NLL backward of a loss head with the loss weights taken from the ground truth
 * itself (losses.py:62-73 -- inner weights gt_assignment, dustbin column gt_matches0 == -1,
 * dustbin row gt_matches1 == -1) instead of a dense [B,M+1,N+1] weight tensor: lg_head_backward
 * with la_grad = those weights, grad_similarity = NULL, and the same results bit for bit.
 * gt_assignment [B,M,N] uint8 0/1, gt_matches0/1 [B,M] / [B,N] int64; s_in / s_dust required;
 * M == N (the reference's weights exist only then).  from_forward != 0: `scratch` holds the
 * matching lg_head_forward / lg_head_nll_forward's saved activations
 * (lg_head_backward_from_forward); 0: they are recomputed.  ABI 10. */
int lg_head_nll_backward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0,
                         const float* desc1, int32_t B, int32_t M, int32_t N, const uint8_t* gt_assignment,
                         const int64_t* gt_matches0, const int64_t* gt_matches1, const float* s_in, const float* s_dust,
                         const float* grad_token0, const float* grad_token1, float* const* grads, float* grad_desc0,
                         float* grad_desc1, int32_t from_forward, void* scratch, size_t scratch_bytes, void* stream);

/* Kernel-level entries of the training kernels (tests; no reference counterpart).
 * lg_train_gemm: C[b] = alpha (op(A[b]) op(B[b]) + bias) + beta C[b] in fp32 with fp32
 *   accumulation, op(A)(m,k) = ta ? A[k*lda+m] : A[m*lda+k], op(B)(k,n) = tb ? B[n*ldb+k] : B[k*ldb+n].
 *   The route follows from shape and alignment alone: bf16x6 on the bf16 matrix cores (each fp32
 *   operand split into three bf16 pieces; error per product ~2^-24) for ta = 0 with K % 16 == 0,
 *   16-byte-aligned operands and beta in {0, 1} (beta = 0 when batch > 1; tb = 1 when batch > 1),
 *   and for every weight gradient (ta = 1, tb = 0);
 *   the f32 matrix cores for the remaining shapes.
 *   workspace: lg_train_gemm_workspace_bytes (split-k partials with their column-sum partials, or
 *   the transposed B of a (0, 0) product on the bf16x6 route; 0 is allowed, then no split and
 *   (0, 0) on the f32 matrix cores).
 * lg_train_gemm_ex: the same with the operands only the library's own calls pass (all nullable,
 *   batch 1): A1 / lda1 / K0 (ta = 0, tb = 1 on the bf16x6 route: op(A)(m,k) = A1[m*lda1 + k - K0]
 *   for k >= K0), B1 / ldb1 / N0 (ta = 1, tb = 0, N0 % 128 == 0, 16-byte-aligned operands:
 *   op(B)(k,n) = B1[k*ldb1 + n - N0] for n >= N0), R / ldr (the beta term reads R instead of C;
 *   R is not written) and colsumA [M] = sum_k op(A)(m,k) (ta = 1, tb = 0; ignored otherwise).
 *   LG_E_INVALID, with nothing launched, when no route takes the operands.  ABI 12.
 * lg_train_attention / _backward: the fp32 training attention on fp32 head-major-in-columns
 *   tensors [B*Nq or B*Nk, 256] (head h at columns 64h..): O, lse [B*H*Nq] (log2 units); the
 *   backward writes dQ (zeroed first), dK, dV; delta_ws [B*H*Nq] floats.  Synchronise. */
int lg_train_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t batch, size_t* bytes);
int lg_train_gemm(const float* A, const float* Bm, float* C, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA,
                  int64_t sB, int64_t sC, int32_t M, int32_t N, int32_t K, int32_t batch, float alpha, float beta,
                  const float* bias, int32_t ta, int32_t tb, void* workspace, size_t workspace_bytes, void* stream);
int lg_train_gemm_ex(const float* A, const float* Bm, float* C, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA,
                     int64_t sB, int64_t sC, int32_t M, int32_t N, int32_t K, int32_t batch, float alpha, float beta,
                     const float* bias, int32_t ta, int32_t tb, const float* A1, int64_t lda1, int32_t K0, const float* B1,
                     int64_t ldb1, int32_t N0, const float* R, int64_t ldr, float* colsumA, void* workspace,
                     size_t workspace_bytes, void* stream);
int lg_train_attention(const float* q, const float* k, const float* v, int32_t B, int32_t H, int32_t Nq, int32_t Nk,
                       float scale, float* o, float* lse, void* stream);
int lg_train_attention_backward(const float* q, const float* k, const float* v, const float* o, const float* lse,
                                const float* grad_o, int32_t B, int32_t H, int32_t Nq, int32_t Nk, float scale,
                                float* grad_q, float* grad_k, float* grad_v, float* delta_ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGLUE_MI355X_H */
