/* superglue_mi355x.h -- C-ABI of the SuperGlue matcher (liblightglue_mi355x.so, gfx950).
 *
 * Replaces the reference's eval forward and losses of
 *   gluefactory_nonfree/superglue.py:253-307  SuperGlue._forward(data)
 *     :75-104   normalize_keypoints + KeypointEncoder (MLP with eval BatchNorm)
 *     :107-170  MultiHeadedAttention / AttentionalPropagation / AttentionalGNN ("self" / "cross")
 *     :173-201  log_optimal_transport (the same Sinkhorn kernel as lg_log_optimal_transport)
 *     :283-298  match extraction (mutual NN + exp(max) > filter_threshold)
 *   gluefactory_nonfree/superglue.py:309-339  SuperGlue.loss       -> sg_nll_loss(mode 0)
 *   gluefactory/models/utils/losses.py:6-73    NLLLoss (LightGlue)  -> sg_nll_loss(mode 1)
 * The Python binding (lightglue_amd.superglue.SuperGlue) mirrors the reference module tree, so a
 * reference state dict loads unchanged.  Conventions as include/lightglue_mi355x.h: device
 * pointers, row-major fp32, stream-ordered and asynchronous, LG_* error codes, lg_last_error().
 */
#ifndef SUPERGLUE_MI355X_H
#define SUPERGLUE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_MAX_LAYERS 64
#define SG_MAX_KENC 7

typedef struct sg_config_t {
  int32_t descriptor_dim;              /* 256 (kernels are specialised) */
  int32_t n_layers;                    /* len(GNN_layers) */
  int32_t layer_types[SG_MAX_LAYERS];  /* 0 "self", 1 "cross" */
  int32_t n_kenc;                      /* len(keypoint_encoder) */
  int32_t keypoint_encoder[SG_MAX_KENC];
  int32_t use_scores;
  int32_t sinkhorn_iterations;
  float filter_threshold;
} sg_config_t;

typedef struct sg_inputs_t {
  int32_t B, M, N;
  const float* keypoints0;    /* [B][M][2] pixels */
  const float* keypoints1;    /* [B][N][2] */
  const float* descriptors0;  /* [B][M][256] */
  const float* descriptors1;  /* [B][N][256] */
  const float* scores0;       /* [B][M] keypoint scores (use_scores) */
  const float* scores1;
  const float* image_size0;   /* [B][2] (w, h) or null: image_w0 / image_h0 (the image shape) */
  const float* image_size1;
  int32_t image_w0, image_h0, image_w1, image_h1;
} sg_inputs_t;

typedef struct sg_outputs_t {
  int64_t* matches0;          /* [B][M] */
  int64_t* matches1;          /* [B][N] */
  float* matching_scores0;    /* [B][M] */
  float* matching_scores1;    /* [B][N] */
  float* sinkhorn_cost;       /* [B][M][N] or null */
  float* log_assignment;      /* [B][M+1][N+1] or null */
  float* descriptors0;        /* [B][M][256] GNN output (input of final_proj) or null */
  float* descriptors1;
} sg_outputs_t;

typedef struct sg_handle sg_handle_t;

int sg_create(const sg_config_t* cfg, int device, sg_handle_t** out);
int sg_destroy(sg_handle_t* h);
/* the state-dict schema (names / element counts) this configuration expects; BatchNorm
 * num_batches_tracked buffers are not part of it */
int sg_weight_count(const sg_handle_t* h);
const char* sg_weight_name(const sg_handle_t* h, int i);
int64_t sg_weight_numel(const sg_handle_t* h, int i);
/* device fp32 tensors keyed like the reference state dict; repacked on `stream` (one read-back of
 * bin_score and the range statistics) */
int sg_load_weights(sg_handle_t* h, int n, const char* const* names, const float* const* tensors, const int64_t* numels,
                    void* stream);
int sg_workspace_bytes(const sg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);
/* eval forward; M, N >= 1 (the caller handles the empty case, superglue.py:257-264) */
int sg_forward(sg_handle_t* h, const sg_inputs_t* in, sg_outputs_t* out, void* workspace, size_t workspace_bytes,
               void* stream);
/* The eval forward on a ragged batch: pair b has num_keypoints0[b] <= M and num_keypoints1[b] <= N
 * real points, stored first; the rest of each slot is arbitrary (NaN allowed) in keypoints,
 * descriptors and scores.  Counts are device int32 [B], clamped on the device to [0, capacity] and
 * never read on the host.  Pair b gets what it gets alone at its own sizes, in the capacity layout:
 * matches -1 / scores 0 on padded points, sinkhorn_cost 0 and descriptors 0 outside the real block,
 * log_assignment as lg_log_optimal_transport_ragged lays it out.  A pair with an empty image has no
 * matches and runs nothing.  Both NULL: sg_forward; one NULL: LG_E_INVALID.  Same workspace. */
int sg_forward_ragged(sg_handle_t* h, const sg_inputs_t* in, const int32_t* num_keypoints0,
                      const int32_t* num_keypoints1, sg_outputs_t* out, void* workspace, size_t workspace_bytes,
                      void* stream);
/* NLL of a log assignment [B][M+1][N+1]; gt_assignment [B][M][N] (0/1 bytes), gt_matches [B][M] /
 * [B][N] (-1 = unmatched).  out [5][B]: nll, nll_pos, nll_neg, num_matchable, num_unmatchable.
 * mode 0: SuperGlue.loss; mode 1: NLLLoss (requires M == N, as the reference's indexing does) */
int sg_nll_loss(const float* log_assignment, int32_t B, int32_t M, int32_t N, const uint8_t* gt_assignment,
                const int64_t* gt_matches0, const int64_t* gt_matches1, int32_t mode, float nll_balancing, float* out,
                void* stream);
/* The same with a caller-owned workspace of sg_nll_workspace_bytes(B, M) bytes (the fp64 partial
 * sums; sg_nll_loss allocates and frees them stream-ordered on every call).  ABI 8. */
int sg_nll_workspace_bytes(int32_t B, int32_t M, size_t* bytes);
int sg_nll_loss_ws(const float* log_assignment, int32_t B, int32_t M, int32_t N, const uint8_t* gt_assignment,
                   const int64_t* gt_matches0, const int64_t* gt_matches1, int32_t mode, float nll_balancing,
                   float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training: SuperGlue's training step as torch autograd runs it in the reference
 * (gluefactory/train.py:436-450 over superglue.py:253-339).  No reference counterpart as an
 * interface; these entry points are what a torch.autograd.Function binds.
 *
 * `params` are raw fp32 device pointers in the schema order (sg_weight_name(h, i)) and the
 * reference layouts (Conv1d weights [out][in][1]); gradients come back in the same order and
 * layouts (`grads[i]` overwritten when non-null; BatchNorm running statistics take none).  All
 * arithmetic is fp32 (f32-input matrix cores).
 *
 * sg_train_forward: the training-mode forward (superglue.py:253-307 with self.training): BatchNorm
 * with batch statistics per image set, the Sinkhorn iterates kept for the backward in `saved`
 * (sg_train_saved_bytes; caller-owned, pass it to sg_train_backward).  out->log_assignment is
 * required; sinkhorn_cost, the matches / scores and descriptors0/1 are written when non-null.
 * Updates the BatchNorm running statistics IN PLACE (params[] entries running_mean / running_var,
 * momentum 0.1, unbiased variance), once per image set -- the reference's count.
 * sg_train_backward: from d(loss)/d(log_assignment) [B][M+1][N+1] and d(loss)/d(sinkhorn_cost)
 * [B][M][N] (each nullable: zero), writes every parameter gradient (bin_score included) and
 * grad_desc0/1 [B][M][256] / [B][N][256] (nullable).  It also applies the GNN BatchNorms' second
 * running-statistics update that the reference's torch.utils.checkpoint recomputation makes
 * (superglue.py:151-155).  Scratch: sg_train_scratch_bytes.  Both asynchronous; the attention
 * backward's dQ sums use float atomics (last-bit differences between calls).
 * sg_nll_backward: d(loss)/d(log_assignment) of sg_nll_loss (mode 0 SuperGlue.loss, 1 NLLLoss)
 * from d(loss)/d(nll, nll_pos, nll_neg) [B] each (nullable) and the forward's out [5][B].
 */
int sg_train_saved_bytes(const sg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);
/* Where sg_train_forward keeps the ReLU output that follows BatchNorm `name` (reference module
 * name: "kenc.encoder.<3i+1>" or "gnn.layers.<l>.mlp.1") inside `saved`: byte offset and element
 * count of the fp32 [B*M + B*N, C] rows (image-0 rows first).  Its sign pattern is the forward's
 * ReLU decision per unit, which the backward differentiates; the GPU tests hand it to the float64
 * oracle so both differentiate the same piece of the piecewise-linear function.  ABI 9. */
int sg_train_saved_tensor(const sg_handle_t* h, int32_t B, int32_t M, int32_t N, const char* name, size_t* offset,
                          size_t* numel);
/* Data-parallel training (gluefactory/train.py:307-309: SyncBatchNorm + DistributedDataParallel).
 * sg_set_collective: `fn(ctx, n, stream)` must SUM the first n floats of `buf` (a caller-owned
 * device buffer of `capacity` >= sg_collective_floats() floats) over the ranks, in place and
 * ordered on `stream` (e.g. torch.distributed.all_reduce of a tensor over that memory on the
 * current stream); it returns 0 on success.  With a collective set, every BatchNorm of
 * sg_train_forward / sg_train_backward uses the statistics of the GLOBAL batch, as
 * torch.nn.SyncBatchNorm does: the per-channel sums and centred sums of squares (forward) and the
 * two per-channel sums of the backward are all-reduced, the running statistics take the global
 * unbiased variance, gamma / beta gradients stay local sums (DDP averages them).  fn = NULL
 * restores per-rank statistics.
 * sg_set_grad_ready_hook: as lg_set_grad_ready_hook; layer = L (final_proj.*, bin_score) first,
 * then each GNN layer L-1 .. 0 (gnn.layers.<layer>.*), then -1 (kenc.*).  ABI 8. */
typedef int (*sg_collective_fn)(void* ctx, int64_t n, void* stream);
size_t sg_collective_floats(void);
int sg_set_collective(sg_handle_t* h, sg_collective_fn fn, void* ctx, float* buf, int64_t capacity);
typedef void (*sg_grad_ready_fn)(void* ctx, int32_t layer, void* stream);
int sg_set_grad_ready_hook(sg_handle_t* h, sg_grad_ready_fn fn, void* ctx);
int sg_train_scratch_bytes(const sg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes);
int sg_train_forward(sg_handle_t* h, float* const* params, const sg_inputs_t* in, sg_outputs_t* out, void* saved,
                     size_t saved_bytes, void* stream);
int sg_train_backward(sg_handle_t* h, float* const* params, const sg_inputs_t* in, const void* saved, size_t saved_bytes,
                      const float* grad_log_assignment, const float* grad_cost, float* const* grads, float* grad_desc0,
                      float* grad_desc1, void* scratch, size_t scratch_bytes, void* stream);
int sg_nll_backward(const float* stats, const float* grad_nll, const float* grad_nll_pos, const float* grad_nll_neg,
                    int32_t B, int32_t M, int32_t N, const uint8_t* gt_assignment, const int64_t* gt_matches0,
                    const int64_t* gt_matches1, int32_t mode, float nll_balancing, float* grad_log_assignment,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
