// Host-visible launch wrappers of the training (autograd) kernels in train.hip (internal to
// liblightglue_mi355x.so).  Every kernel takes and returns fp32 and accumulates in fp32, with the
// full fp32 range, so gradients of any magnitude need no range scaling.  The route of a product
// follows from its shape and alignment alone:
//   * bf16x6 (common.h: each fp32 operand split into three bf16 pieces, six v_mfma_f32_32x32x16_bf16
//     per block; error per product ~2^-24 like an f32 fma chain, at the bf16 rate): tgemm's
//     k-contiguous products (ta = 0) with K % 16 == 0 and 16-byte-aligned operands, every weight
//     gradient (ta = 1, tb = 0), and the attention's S, P V, dP, dV and dK;
//   * f32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32: exact fp32 products): tgemm's remaining shapes
//     (K % 16 != 0, unaligned operands, beta outside {0, 1}, a beta term with batch > 1, an input
//     gradient with batch > 1, ta && tb) and the attention backward's dQ, whose dS
//     operand is already in LDS as fp32.
// Reductions are deterministic (fixed-order partial sums) except the attention backward's dQ, which
// is summed with float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace lg {

// C[b] = alpha * (op(A[b]) op(B[b]) + bias) + beta * C[b]    (b < batch; bias [N] or null)
//   op(A)(m,k) = ta ? A[k*lda + m] : A[m*lda + k]      (M x K)
//   op(B)(k,n) = tb ? B[n*ldb + k] : B[k*ldb + n]      (K x N)
// A linear layer y = x W^T + b is (ta=0, tb=1); its input gradient dx = dy W is (0, 0); its weight
// gradient dW = dy^T x is (1, 0) -- K = rows, split over workgroups when the output has few tiles
// (fixed-order partial sums in `ws`, tgemm_ws_floats).
struct TGemm {
  const float* A;
  const float* B;
  float* C;
  long long lda, ldb, ldc;
  long long sA, sB, sC;  // batch strides (elements)
  int M, N, K, batch;
  float alpha, beta;
  const float* bias;
  // ta = 1 only: also out[b][m] = sum_k A[b][k][m] (the column sums of the k-major A: a linear
  // layer's bias gradient beside its weight gradient, from the same read of dY) -- honoured for
  // ta && !tb, otherwise ignored
  float* colsumA = nullptr;
  // R (ldr): the beta term reads R instead of C, C = alpha (op(A) op(B) + bias) + beta R -- a
  // residual added on the way out (batch 1), without first copying it into C
  const float* R = nullptr;
  long long ldr = 0;
  // Two-source operands (batch 1):
  //   A1 (ta = 0, tb = 1: the bf16x6 A B^T route): op(A)(m, k) = k < K0 ? A[m lda + k] : A1[m lda1 + k - K0]
  //   B1 (ta = 1, tb = 0: the vectorised bf16x6 weight-gradient route; N0 % 128 == 0):
  //      op(B)(k, n) = n < N0 ? B[k ldb + n] : B1[k ldb1 + n - N0]
  // -- a concatenated [X | message] operand read from its two halves instead of being copied together.
  // tgemm returns hipErrorInvalidValue if the route cannot take them.
  const float* A1 = nullptr;
  long long lda1 = 0;
  int K0 = 0;
  const float* B1 = nullptr;
  long long ldb1 = 0;
  int N0 = 0;
};
size_t tgemm_ws_floats(int M, int N, int K, int batch);
hipError_t tgemm(const TGemm& g, bool ta, bool tb, float* ws, size_t ws_floats, hipStream_t st);

// Attention on row-major fp32 tensors (row stride ld*, head h at columns [64h, 64h+64)); item
// (b, h): queries rows [b*Nq, (b+1)*Nq) of Q, keys / values rows [b*Nk, (b+1)*Nk) of K / V.
//   forward:  O = softmax(scale Q K^T) V, lse = log2 sum exp2(c Q K^T) per (item, query), c = scale log2 e
//   backward: with delta = rowsum(dO * O) per (item, query) (attn_delta):
//             dQ += scale dS K (float atomics: dQ must hold its initial value),
//             dK (+)= scale dS^T Q, dV (+)= P^T dO (accum_kv: add to what dK / dV hold)
struct TAttn {
  const float* Q;
  const float* K;
  const float* V;
  float* O;
  float* lse;  // [B*H][Nq]
  const float* dO;
  const float* delta;  // [B*H][Nq]
  float* dQ;
  float* dK;
  float* dV;
  int ldq, ldk, ldv, ldo;
  int B, H, Nq, Nk;
  float scale;
  int accum_kv;
};
hipError_t tattn_forward(const TAttn& a, hipStream_t st);
hipError_t tattn_backward(const TAttn& a, hipStream_t st);
// delta[(b*H + h)*Nq + q] = sum_d dO[(b*Nq+q)*ldo + 64h + d] * O[same]
hipError_t attn_delta(const float* O, const float* dO, int ldo, int B, int H, int Nq, float* delta, hipStream_t st);

// SelfBlock qkv split + rotary (lightglue.py:184-188): qkv [R][768] in the reference layout
// (column h*192 + d*3 + t, :185) -> Q, K rotated by (cos, sin) [R][32], V; [R][256] each.
hipError_t rotary_split(const float* qkv, const float* cosb, const float* sinb, int R, int H, float* Q, float* K,
                        float* V, hipStream_t st);
// its backward: gQKV [R][768] from gQ, gK, gV and the rotated Q, K; gcos / gsin [R][32] +=.
hipError_t rotary_split_bwd(const float* gQ, const float* gK, const float* gV, const float* Q, const float* K,
                            const float* cosb, const float* sinb, int R, int H, float* gQKV, float* gcos, float* gsin,
                            hipStream_t st);

// Positional encoding of one image set (lightglue.py:21-33,63-77): x [rows][4] (normalised
// position, scale, ori) and cos / sin [rows][32]; `size` [B][2] (w, h) is required (callers run
// kpt_extent for the min/max fallback).
struct TPE {
  const float* kpts;
  const float* size;
  const float* scales;
  const float* oris;
  const float* Wr;  // [32][m_in]
  const float* Wc;  // [32]
  const float* bc;  // [32]
  int B, n, m_in;
  float* x;
  float* cosb;
  float* sinb;
};
hipError_t pe_train(const TPE& p, hipStream_t st);
// d(loss)/d(Wr, Wc, bc) from gcos / gsin [R][32] over both image sets (rows < R0 have count n0,
// the rest n1): partial sums per row block in `part` (pe_bwd_part_floats), then one ordered pass.
size_t pe_bwd_part_floats(int R);
hipError_t pe_backward(const float* x, const float* cosb, const float* sinb, const float* gcos, const float* gsin,
                       int R, int R0, float n0, float n1, int m_in, float* part, float* gWr, float* gWc, float* gbc,
                       hipStream_t st);

// ffn.1 LayerNorm(512, eps 1e-5) + ffn.2 GELU(erf) (lightglue.py:171-176): out = GELU(LN(h));
// stats [R][2] = (mean, rstd).  Backward: gh from gout; dgamma / dbeta through per-block partials.
hipError_t lngelu_fwd(const float* h, const float* gamma, const float* beta, int R, float* out, float* stats,
                      hipStream_t st);
size_t lngelu_bwd_part_floats(int R);
hipError_t lngelu_bwd(const float* gout, const float* h, const float* stats, const float* gamma, const float* beta,
                      int R, float* gh, float* part, float* dgamma, float* dbeta, hipStream_t st);

// out[c] = sum_r s[r] * G[r*ld + c] (s null: 1), c < cols; fixed-order two-pass reduction.
size_t colsum_part_floats(int rows, int cols);
hipError_t colsum(const float* G, long long ld, int rows, int cols, const float* s, float* part, float* out,
                  hipStream_t st);

// The weight / bias gradients of up to two Linear(256 -> 1) on X [rows][256] (256-float rows,
// 16-byte aligned) in one read of X: gw0 = X^T s0, gb0 = sum s0, gw1 / gb1 likewise with s1
// (nullable, then gw1 / gb1 are not written); any output pointer nullable.
size_t head_vec_grads_part_floats(int rows);
hipError_t head_vec_grads(const float* X, int rows, const float* s0, const float* s1, float* part, float* gw0, float* gb0,
                          float* gw1, float* gb1, hipStream_t st);
// y[r] = x[r] . w + b (256 wide; Linear(256 -> 1), matchability / token confidence)
hipError_t gemv256(const float* x, int rows, const float* w, const float* b, float* y, hipStream_t st);
// G[r][c] += s[r] * w[c] (256 wide)
hipError_t rank1_add256(float* G, int rows, const float* s, const float* w, hipStream_t st);
// C[i] = A[i] + B[i] over rows x 256 with row strides lda / ldb / ldc
hipError_t add_rows256(const float* A, long long lda, const float* B, long long ldb, float* C, long long ldc, int rows,
                       hipStream_t st);

// GX rows += the layer-`layer` slices of g0 [B][L][M][256] (image-0 rows) / g1 [B][L][N][256]
hipError_t add_layer_rows(float* GX, const float* g0, const float* g1, int B, int M, int N, int L, int layer,
                          hipStream_t st);

// ---- assignment head backward (MatchAssignment + sigmoid_log_double_softmax, lightglue.py:284-315)
// sim [B][M][N]: lser [B*M], lsec [B*N] natural-log row / column logsumexp
size_t sim_lse_part_floats(int B, int M, int N);
hipError_t sim_lse(const float* sim, int B, int M, int N, float* lser, float* lsec, float* part, hipStream_t st);
// Gradient of the log assignment T [B][M+1][N+1] scaled per pair (s_in for the inner block,
// s_dust for the dustbins; null = 1): rs [B*M] / cs [B*N] = scaled inner row / column sums,
// gd0 [B*M] / gd1 [B*N] = scaled dustbin entries.
size_t la_grad_sums_part_floats(int B, int M, int N);
hipError_t la_grad_sums(const float* T, const float* s_in, const float* s_dust, int B, int M, int N, float* rs,
                        float* cs, float* gd0, float* gd1, float* part, hipStream_t st);
// In place: sim -> d(loss)/d(sim) = 2 g - softmax_row * rs - softmax_col * cs (+ gsim_ext);
// gz0 [B*M] / gz1 [B*N] = d/d(matchability logits).
hipError_t la_grad_sim(float* sim, const float* T, const float* s_in, const float* lser, const float* lsec,
                       const float* rs, const float* cs, const float* gsim_ext, int B, int M, int N, hipStream_t st);
hipError_t la_grad_z(const float* z, const float* rs, const float* gd, int rows, float* gz, hipStream_t st);
// dst [batch][cols][rows] = src [batch][rows][cols] transposed
hipError_t transpose_batched(const float* src, int rows, int cols, int batch, float* dst, hipStream_t st);
// la_grad_sums + la_grad_sim for the NLL weights of a ground truth (losses.py:62-73) without the
// dense weight tensor: gta [B][M][N] uint8 0/1, gt0 [B*M] / gt1 [B*N] int64 (-1 = unmatchable);
// s_in / s_dust required; M == N as the reference's weights need.  Bit-identical to the dense
// path on nll_weights.  part: la_grad_gt_part_floats.
size_t la_grad_gt_part_floats(int B, int M, int N);
hipError_t la_grad_gt(float* sim, const uint8_t* gta, const int64_t* gt0, const int64_t* gt1, const float* s_in,
                      const float* s_dust, const float* lser, const float* lsec, int B, int M, int N, float* rs, float* cs,
                      float* gd0, float* gd1, float* part, hipStream_t st);
// sigmoid_log_double_softmax forward: la [B][M+1][N+1] from sim, its row / column LSE and z0 / z1
hipError_t la_forward(const float* sim, const float* lser, const float* lsec, const float* z0, const float* z1, int B, int M,
                      int N, float* la, hipStream_t st);
// A loss head's NLL terms out[5][B] (sg_nll_loss's layout and arithmetic) and its log assignment's
// row / column argmaxes am0 [B*M] / am1 [B*N] (int64; rows < M over N + 1 columns, columns < N over
// M + 1 rows; first maximum) without storing the log assignment.  N <= 4096.  part:
// la_nll_part_floats(B, M, N) floats.
size_t la_nll_part_floats(int B, int M, int N);
hipError_t la_nll(const float* sim, const float* lser, const float* lsec, const float* z0, const float* z1, int B, int M,
                  int N, const uint8_t* gta, const int64_t* gt0, const int64_t* gt1, int mode, float bal, float* out,
                  int64_t* am0, int64_t* am1, float* part, hipStream_t st);

// ---- SuperGlue training (sg_train.hip; superglue.py:63-201 in training mode)
// BatchNorm1d with batch statistics over `rows` rows of C channels (C % 4 == 0, C <= 1024,
// rows >= 2) followed by ReLU: Y = relu(gamma (X - mean) rstd + beta); stats [3][C] = (mean, rstd,
// unbiased variance).  Backward: dX from dY (the gradient of the ReLU output); dgamma / dbeta
// written (accum 0) or added (accum 1).  part: bn_part_floats(rows, C).
size_t bn_part_floats(int rows, int C);
hipError_t bn_train_fwd(const float* X, long long ldx, int rows, int C, const float* gamma, const float* beta, float* Y,
                        long long ldy, float* stats, float* part, hipStream_t st);
hipError_t bn_train_bwd(const float* X, long long ldx, const float* dY, long long ldy, int rows, int C, const float* stats,
                        const float* gamma, const float* beta, float* dX, long long lddx, float* dgamma, float* dbeta,
                        int accum, float* part, hipStream_t st);
// SyncBatchNorm (data-parallel training, train.py:307-309; sg_set_collective): fn(ctx, n, stream)
// sums buf[0..n) over the ranks in place, ordered on the stream, and returns 0 on success.
struct BnSync {
  int (*fn)(void* ctx, int64_t n, void* stream) = nullptr;
  void* ctx = nullptr;
  float* buf = nullptr;
  int64_t cap = 0;
};
size_t bn_sync_floats();  // the collective buffer a BnSync needs (C <= 1024, two image sets)
// Both image sets of one BatchNorm call site: rows [0, rows[0]) and [rows[0], rows[0] + rows[1])
// of X / Y / dY / dX, stats [2][3][C].  sync == null: each set on its own (bn_train_fwd /
// bn_train_bwd per set, bit for bit); otherwise every set's statistics are its GLOBAL batch's
// (one collective per pass for both sets: sums and counts, then centred sums of squares; in the
// backward the two per-channel sums), as torch.nn.SyncBatchNorm computes them.  A failing
// collective returns hipErrorUnknown.
hipError_t bn_train_fwd_sets(const float* X, long long ldx, const int* rows, int C, const float* gamma,
                             const float* beta, float* Y, long long ldy, float* stats, float* part, const BnSync* sync,
                             hipStream_t st);
hipError_t bn_train_bwd_sets(const float* X, long long ldx, const float* dY, long long ldy, const int* rows, int C,
                             const float* stats, const float* gamma, const float* beta, float* dX, long long lddx,
                             float* dgamma, float* dbeta, float* part, const BnSync* sync, hipStream_t st);
// running = (1 - momentum) running + momentum (mean, unbiased var) of stats
hipError_t bn_running_update(float* rm, float* rv, const float* stats, int C, float momentum, hipStream_t st);
// normalize_keypoints + [x, y(, score)] rows: out [B*n][cin]; size [B][2] (w, h) or null -> (w, h)
hipError_t kenc_input(const float* kpts, const float* scores, const float* size, float w, float h, int B, int n, int cin,
                      float* out, hipStream_t st);
// head-major <-> reference channel order of MultiHeadedAttention (channel d*4 + h, :121-127):
// dst[r][c] = src[perm(r)][c] (by_cols: src[r][perm(c)]), perm(h*64 + d) = d*4 + h; inverse: perm^-1
hipError_t head_gather(const float* src, int rows, int cols, bool by_cols, bool inverse, float* dst, hipStream_t st);
struct HeadGather {
  const float* src;
  float* dst;
  int rows, cols, by_cols, inverse;
};
struct HeadGathers {  // by value as a kernel argument
  HeadGather e[8];
  int n = 0;
  void add(const float* src, int rows, int cols, bool by_cols, bool inverse, float* dst) {
    e[n++] = {src, dst, rows, cols, (int)by_cols, (int)inverse};
  }
};
hipError_t head_gather_multi(const HeadGathers& g, hipStream_t st);
// log_optimal_transport (:181-201) keeping every iterate: Cc [B][M+1][N+1] couplings, U [iters][B][M+1]
// (u_1..u_T), V [iters+1][B][N+1] (v_0 = 0 .. v_T), Z (already + log(M+N)).  alpha: device scalar.
// part: sk_train_part_floats (column-pass partials)
size_t sk_train_part_floats(int B, int M, int N);
// floats of slack every couplings-shaped buffer (Cc, and the gC scratch) needs past its end: the
// fused passes read whole rows of 64 * 33 floats from each row start without bounds checks
size_t sk_train_row_slack_floats();
hipError_t sk_train_forward(const float* cost, const float* alpha, int B, int M, int N, int iters, float* Cc, float* U,
                            float* V, float* Z, float* part, hipStream_t st);
// its backward: d/d cost [B][M][N] (= inner block of d/d Cc, + gext when non-null) and d/d alpha
// (scalar, overwritten; nullable) from gZ.  ws: sk_train_scratch_floats.
size_t sk_train_scratch_floats(int B, int M, int N, int iters);
hipError_t sk_train_backward(const float* Cc, const float* U, const float* V, const float* gZ, const float* gext, int B,
                             int M, int N, int iters, float* gcost, float* galpha, float* ws, hipStream_t st);
// d/d log_assignment of the NLL (mode 0 SuperGlue.loss, 1 NLLLoss) from d/d (nll, nll_pos, nll_neg)
// (nullable rows) and the forward's out [5][B]
hipError_t sg_nll_grad(const uint8_t* gta, const int64_t* gt0, const int64_t* gt1, const float* stats, const float* g_nll,
                       const float* g_pos, const float* g_neg, int B, int M, int N, int mode, float bal, float* gla,
                       hipStream_t st);

}  // namespace lg
