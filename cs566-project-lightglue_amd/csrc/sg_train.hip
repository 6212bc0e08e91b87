// SuperGlue training kernels for gfx950: the batch-statistics BatchNorm + ReLU of the MLPs
// (reference gluefactory_nonfree/superglue.py:63-72 with nn.BatchNorm1d in training mode), the
// keypoint-encoder input (:75-86,100-104) and the log-domain Sinkhorn with its backward
// (:174-201 differentiated by torch autograd in gluefactory/train.py:450).  The GNN's matrix
// products and attention run on the training GEMM / attention kernels of train.hip.
//
// Every reduction is a fixed-order two-pass sum (per-block partials, then one ordered pass), so
// repeated calls give identical bits.  BatchNorm tensors are row-major [rows][C] over the rows of
// one image set (the reference's [b, C, n] batch statistics over (b, n)).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "train.h"

namespace lg {

namespace {

constexpr float kBnEps = 1e-5f;  // torch.nn.BatchNorm1d default
constexpr int BN_RB = 128;        // rows per partial block
constexpr int BN_U = 4;           // rows per thread whose loads bn_part_kernel issues together

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// the forward's normalised value and its activation; the backward recomputes both identically
__device__ __forceinline__ float bn_xhat(float x, float mu, float rs) { return (x - mu) * rs; }
__device__ __forceinline__ float bn_y(float xh, float g, float b) { return g * xh + b; }

// Partial column sums over rows [blk*BN_RB, ...): thread t owns columns 4 (t % tpr) .. +3 of row
// lane t / tpr (tpr = C / 4).  mode 0: sum x; 1: sum (x - mean)^2; 2 (backward, dy' = dY masked by
// ReLU(y) > 0): sum dy' -> part0, sum dy' xhat -> part1.
__global__ __launch_bounds__(256) void bn_part_kernel(const float* X, long long ldx, int rows, int C, int mode,
                                                      const float* mean, const float* rstd, const float* gamma,
                                                      const float* beta, const float* dY, long long ldy, float* part0,
                                                      float* part1) {
  __shared__ float s0[256 * 4], s1[256 * 4];
  const int tpr = C >> 2, rl = 256 / tpr;
  const int t = threadIdx.x, c4 = t % tpr, lr = t / tpr;
  const int r0 = blockIdx.x * BN_RB, r1 = min(rows, r0 + BN_RB);
  float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
  if (lr < rl) {
    const int c = 4 * c4;
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, rs = mu, g = mu, b = mu;
    if (mode >= 1) mu = ld4(mean + c);
    if (mode == 2) {
      rs = ld4(rstd + c);
      g = ld4(gamma + c);
      b = ld4(beta + c);
    }
    // the thread's rows r0 + lr, r0 + lr + rl, ... accumulated in that order; BN_U rows' loads
    // are issued together ahead of their adds (the same sums, more memory in flight)
    auto acc = [&](const f32x4& x, const f32x4& dy) {
      if (mode == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a0[e] += x[e];
      } else if (mode == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = x[e] - mu[e];
          a0[e] = fmaf(d, d, a0[e]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = bn_xhat(x[e], mu[e], rs[e]);
          const float d = bn_y(xh, g[e], b[e]) > 0.f ? dy[e] : 0.f;
          a0[e] += d;
          a1[e] = fmaf(d, xh, a1[e]);
        }
      }
    };
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    int r = r0 + lr;
    for (; r + (BN_U - 1) * rl < r1; r += BN_U * rl) {
      f32x4 x[BN_U], dy[BN_U];
#pragma unroll
      for (int u = 0; u < BN_U; ++u) {
        x[u] = ld4(X + (long long)(r + u * rl) * ldx + c);
        dy[u] = mode == 2 ? ld4(dY + (long long)(r + u * rl) * ldy + c) : z4;
      }
#pragma unroll
      for (int u = 0; u < BN_U; ++u) acc(x[u], dy[u]);
    }
    for (; r < r1; r += rl) acc(ld4(X + (long long)r * ldx + c), mode == 2 ? ld4(dY + (long long)r * ldy + c) : z4);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s0[4 * t + e] = a0[e];
    s1[4 * t + e] = a1[e];
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    float v0 = 0.f, v1 = 0.f;
    for (int l = 0; l < rl; ++l) {  // fixed order over the row lanes
      const int k = 4 * (l * tpr + (c >> 2)) + (c & 3);
      v0 += s0[k];
      v1 += s1[k];
    }
    part0[(long long)blockIdx.x * C + c] = v0;
    if (mode == 2) part1[(long long)blockIdx.x * C + c] = v1;
  }
}

// Ordered sum of the partials: a workgroup = 16 columns x 16 partial groups (group g sums partials
// g, g + 16, ...; the groups combine in order).  mode 0: mean; 1: rstd = 1 / sqrt(var + eps) and
// the unbiased variance (running statistics); 2: s0 = sum dy', s1 = sum dy' xhat, dbeta / dgamma
// (+)= them; 3 (SyncBatchNorm): s0 = the raw sum, *cnt = rows (the rank's share of the collective).
__global__ __launch_bounds__(256) void bn_final_kernel(const float* part0, const float* part1, int nb, int C, int rows,
                                                       int mode, float* mean, float* rstd, float* varu, float* s0,
                                                       float* s1, float* dgamma, float* dbeta, int accum,
                                                       float* cnt = nullptr) {
  __shared__ float r0[16][16], r1[16][16];
  const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float a = 0.f, b = 0.f;
  if (c < C) {  // partials g, g + 16, ... in order; eight loads in flight ahead of their adds
    int i = g;
    for (; i + 7 * 16 < nb; i += 8 * 16) {
      float ta[8], tb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        ta[u] = part0[(long long)(i + 16 * u) * C + c];
        tb[u] = mode == 2 ? part1[(long long)(i + 16 * u) * C + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        a += ta[u];
        if (mode == 2) b += tb[u];
      }
    }
    for (; i < nb; i += 16) {
      a += part0[(long long)i * C + c];
      if (mode == 2) b += part1[(long long)i * C + c];
    }
  }
  r0[g][cl] = a;
  r1[g][cl] = b;
  __syncthreads();
  if (g != 0 || c >= C) return;
  a = 0.f;
  b = 0.f;
  for (int q = 0; q < 16; ++q) {
    a += r0[q][cl];
    b += r1[q][cl];
  }
  if (cnt && c == 0) *cnt = (float)rows;
  if (mode == 0) {
    mean[c] = a / (float)rows;
  } else if (mode == 3) {
    s0[c] = a;
  } else if (mode == 1) {
    rstd[c] = 1.f / sqrtf(a / (float)rows + kBnEps);
    varu[c] = a / (float)(rows - 1);
  } else {
    s0[c] = a;
    s1[c] = b;
    if (dbeta) dbeta[c] = accum ? dbeta[c] + a : a;
    if (dgamma) dgamma[c] = accum ? dgamma[c] + b : b;
  }
}

__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(const float* X, long long ldx, int rows, int C,
                                                           const float* mean, const float* rstd, const float* gamma,
                                                           const float* beta, float* Y, long long ldy) {
  const int tpr = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)rows * tpr) return;
  const int r = (int)(i / tpr), c = 4 * (int)(i - (long long)r * tpr);
  const f32x4 x = ld4(X + (long long)r * ldx + c), mu = ld4(mean + c), rs = ld4(rstd + c), g = ld4(gamma + c),
              b = ld4(beta + c);
  f32x4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = fmaxf(bn_y(bn_xhat(x[e], mu[e], rs[e]), g[e], b[e]), 0.f);
  *reinterpret_cast<f32x4*>(Y + (long long)r * ldy + c) = y;
}

// dx = gamma rstd (dy' - s0 / n - xhat s1 / n); n = rows, or the global count *nglob (SyncBatchNorm)
__global__ __launch_bounds__(256) void bn_apply_bwd_kernel(const float* X, long long ldx, const float* dY, long long ldy,
                                                           int rows, int C, const float* mean, const float* rstd,
                                                           const float* gamma, const float* beta, const float* s0,
                                                           const float* s1, float* dX, long long lddx,
                                                           const float* nglob = nullptr) {
  const int tpr = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)rows * tpr) return;
  const int r = (int)(i / tpr), c = 4 * (int)(i - (long long)r * tpr);
  const float inv_n = 1.f / (nglob ? *nglob : (float)rows);
  const f32x4 x = ld4(X + (long long)r * ldx + c), dy = ld4(dY + (long long)r * ldy + c), mu = ld4(mean + c),
              rs = ld4(rstd + c), g = ld4(gamma + c), b = ld4(beta + c), a0 = ld4(s0 + c), a1 = ld4(s1 + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float xh = bn_xhat(x[e], mu[e], rs[e]);
    const float d = bn_y(xh, g[e], b[e]) > 0.f ? dy[e] : 0.f;
    o[e] = g[e] * rs[e] * (d - a0[e] * inv_n - xh * (a1[e] * inv_n));
  }
  *reinterpret_cast<f32x4*>(dX + (long long)r * lddx + c) = o;
}

// SyncBatchNorm: the statistics of set `set` from the all-reduced sums buf[set][C] and count
// buf[2C + set] -- the same expressions as bn_final_kernel's modes 0 / 1 with the global count
// (one rank: bit-identical to them)
__global__ void bn_sync_finish_kernel(const float* buf, int C, int set, int mode, float* mean, float* rstd,
                                      float* varu) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float a = buf[set * C + c], n = buf[2 * C + set];
  if (mode == 0) {
    mean[c] = a / n;
  } else {
    rstd[c] = 1.f / sqrtf(a / n + kBnEps);
    varu[c] = a / (n - 1.f);
  }
}

// running = (1 - momentum) running + momentum batch (torch.nn.functional.batch_norm, unbiased var)
__global__ void bn_running_kernel(float* rm, float* rv, const float* mean, const float* varu, int C, float momentum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  rm[c] = (1.f - momentum) * rm[c] + momentum * mean[c];
  rv[c] = (1.f - momentum) * rv[c] + momentum * varu[c];
}

// normalize_keypoints (:75-86) + the encoder input [x, y(, score)] (:100-104), one row per keypoint
__global__ void kenc_input_kernel(const float* kpts, const float* scores, const float* size, float w, float h, int B,
                                  int n, int cin, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * n) return;
  const int b = i / n;
  const float sw = size ? size[2 * b] : w, sh = size ? size[2 * b + 1] : h;
  const float scale = fmaxf(sw, sh) * 0.7f;
  out[(long long)i * cin] = (kpts[2 * i] - sw / 2.f) / scale;
  out[(long long)i * cin + 1] = (kpts[2 * i + 1] - sh / 2.f) / scale;
  if (cin == 3) out[(long long)i * cin + 2] = scores[i];
}

// dst row r = src row perm(r), perm(h*64 + d) = d*4 + h (MultiHeadedAttention's view(b, dim, h, n),
// :121-127, gathered head-major); cols: the same on columns (merge's input channels)
__global__ void head_gather_kernel(const float* src, int rows, int cols, int by_cols, int inverse, float* dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  const int r = i / cols, c = i - r * cols;
  auto perm = [](int k) { return (k & 63) * 4 + (k >> 6); };      // head-major -> reference
  auto iperm = [](int k) { return (k & 3) * 64 + (k >> 2); };     // reference -> head-major
  int sr = r, sc = c;
  if (by_cols) sc = inverse ? iperm(c) : perm(c);
  else sr = inverse ? iperm(r) : perm(r);
  dst[i] = src[(long long)sr * cols + sc];
}

// ---------------------------------------------------------------- Sinkhorn (training)
// couplings [B][M+1][N+1]: the cost with the dustbin score alpha (:185-192)
__global__ __launch_bounds__(256) void sk_couplings_kernel(const float* cost, const float* alpha, int B, int M, int N,
                                                           float* Cc) {
  const int row = blockIdx.x, b = row / (M + 1), i = row - b * (M + 1);  // one workgroup per row
  float* out = Cc + (long long)row * (N + 1);
  const float a = alpha[0];
  if (i < M) {
    const float* c = cost + ((long long)b * M + i) * N;
    for (int j = threadIdx.x; j < N; j += 256) out[j] = c[j];
    if (threadIdx.x == 0) out[N] = a;
  } else {
    for (int j = threadIdx.x; j <= N; j += 256) out[j] = a;
  }
}

// exp on the hardware exp2 (v_exp_f32): the passes' arguments are <= 0 up to rounding (log-domain
// values minus a running max or a normaliser), where the product's rounding (|x| log2 e 2^-24
// relative) only touches terms that are already tiny; expf's range fix-ups cost ~10 VALU per value
__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// (max, sum exp(x - max)) of a lane, reduced over the wave
__device__ __forceinline__ float lse_wave(float m, float s) {
  const float mx = wave_max(m);
  const float t = mx == -INFINITY ? 0.f : s * expf(m - mx);
  return mx + logf(wave_sum(t));
}

// u[b][i] = lmu_i - logsumexp_j (C[b][i][j] + v[b][j])          (:176, one wave per row)
// mode 1 (backward): gu[b][i] = base[b][i] - sum_j g[b][j] exp(C + u_i + v_j - lnu_j)
// mode 2: rowsum[b][i] = sum_j C[b][i][j] (the gradient's row sums)
__global__ __launch_bounds__(256) void sk_row_kernel(const float* Cc, int B, int M1, int N1, const float* u,
                                                     const float* v, const float* g, const float* base, float norm,
                                                     float lmu_last, float lnu_last, int mode, float* out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= B * M1) return;
  const int b = row / M1, i = row - b * M1;
  const float* c = Cc + (long long)row * N1;
  const float* vb = v ? v + (long long)b * N1 : nullptr;
  if (mode == 0) {
    // chunks of 8 values per lane: the chunk max first, then one exponential per value
    float m = -INFINITY, s = 0.f;
    for (int j0 = 0; j0 < N1; j0 += 512) {
      float x[8];
      float cm = -INFINITY;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int j = j0 + l + 64 * q;
        x[q] = j < N1 ? c[j] + vb[j] : -INFINITY;
        cm = fmaxf(cm, x[q]);
      }
      if (cm == -INFINITY) continue;
      const float mn = fmaxf(m, cm);
      float t = s * exp_fast(m - mn);  // s == 0 while m == -inf
#pragma unroll
      for (int q = 0; q < 8; ++q) t += exp_fast(x[q] - mn);
      m = mn;
      s = t;
    }
    const float lse = lse_wave(m, s);
    if (l == 0) out[row] = (i < M1 - 1 ? norm : lmu_last) - lse;
    return;
  }
  float acc = 0.f;
  if (mode == 1) {
    const float ui = u[row];
    const float* gb = g + (long long)b * N1;
    for (int j = l; j < N1; j += 64) acc = fmaf(gb[j], exp_fast(c[j] + ui + vb[j] - (j < N1 - 1 ? norm : lnu_last)), acc);
  } else {
    for (int j = l; j < N1; j += 64) acc += c[j];
  }
  acc = wave_sum(acc);
  if (l == 0) out[row] = mode == 1 ? (base ? base[row] : 0.f) - acc : acc;
}

// v[b][j] = lnu_j - logsumexp_i (C[b][i][j] + u[b][i])          (:177)
// mode 1 (backward of step t): with u = u_t, v = v_t, vp = v_{t-1}, gu = d/d u_t, gv = d/d v_t:
//   pr = exp(C + vp_j + u_i - lmu_i) (u_t's softmax), pc = exp(C + u_i + v_j - lnu_j) (v_t's)
//   out[j] = d/d v_{t-1} = -sum_i gu_i pr;  gC -= gv_j pc + gu_i pr  (in place)
// mode 2: colsum[b][j] = sum_i C[b][i][j]
// Pass 1: a workgroup = 64 columns x SK_CH rows of one pair (4 row groups of 64 lanes), so a launch
// has (N+1)/64 x (M+1)/SK_CH x B workgroups; it writes one (max, sum) or sum per column and chunk.
// Pass 2 combines the chunks of a column in order.
constexpr int SK_CH = 128;

__global__ __launch_bounds__(256) void sk_col_part_kernel(const float* Cc, int B, int M1, int N1, const float* u,
                                                          const float* v, const float* vp, const float* gu,
                                                          const float* gv, float* gC, float norm, float lmu_last,
                                                          float lnu_last, int mode, float* part) {
  __shared__ float sm[4][64], ss[4][64];
  const int b = blockIdx.z, ch = blockIdx.y, j = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
  const bool ok = j < N1;
  const long long base = (long long)b * M1 * N1;
  const int i0 = ch * SK_CH, i1 = min(M1, i0 + SK_CH);
  float m = -INFINITY, s = 0.f;
  if (ok) {
    if (mode == 0) {
      const float* ub = u + (long long)b * M1;
      for (int i = i0 + grp; i < i1; i += 32) {  // chunks of 8 rows per thread
        float x[8];
        float cm = -INFINITY;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int r = i + 4 * q;
          x[q] = r < i1 ? Cc[base + (long long)r * N1 + j] + ub[r] : -INFINITY;
          cm = fmaxf(cm, x[q]);
        }
        if (cm == -INFINITY) continue;
        const float mn = fmaxf(m, cm);
        float t = s * exp_fast(m - mn);
#pragma unroll
        for (int q = 0; q < 8; ++q) t += exp_fast(x[q] - mn);
        m = mn;
        s = t;
      }
    } else if (mode == 1) {
      const float* ub = u + (long long)b * M1;
      const float* gub = gu + (long long)b * M1;
      const float vj = v[(long long)b * N1 + j], gvj = gv[(long long)b * N1 + j];
      const float vpj = vp ? vp[(long long)b * N1 + j] : 0.f;
      const float lnu = j < N1 - 1 ? norm : lnu_last;
      float acc = 0.f;
      for (int i = i0 + grp; i < i1; i += 4) {
        const long long k = base + (long long)i * N1 + j;
        const float cij = Cc[k], ui = ub[i], gui = gub[i];
        const float pr = exp_fast(cij + vpj + ui - (i < M1 - 1 ? norm : lmu_last));
        const float pc = exp_fast(cij + ui + vj - lnu);
        acc = fmaf(gui, pr, acc);
        gC[k] -= fmaf(gvj, pc, gui * pr);
      }
      s = -acc;
    } else {
      for (int i = i0 + grp; i < i1; i += 4) s += Cc[base + (long long)i * N1 + j];
    }
  }
  sm[grp][threadIdx.x & 63] = m;
  ss[grp][threadIdx.x & 63] = s;
  __syncthreads();
  if (grp != 0 || !ok) return;
  const int c = threadIdx.x & 63;
  float mo = -INFINITY, so;
  if (mode == 0) {
    for (int q = 0; q < 4; ++q) mo = fmaxf(mo, sm[q][c]);
    so = 0.f;
    for (int q = 0; q < 4; ++q) so += mo == -INFINITY ? 0.f : ss[q][c] * expf(sm[q][c] - mo);
  } else {
    so = ((ss[0][c] + ss[1][c]) + ss[2][c]) + ss[3][c];
  }
  const long long o = ((long long)b * gridDim.y + ch) * N1 + j;
  part[2 * o] = mo;
  part[2 * o + 1] = so;
}

__global__ void sk_col_final_kernel(const float* part, int B, int N1, int nch, float norm, float lnu_last, int mode,
                                    float* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)B * N1) return;
  const int b = (int)(t / N1), j = (int)(t - (long long)b * N1);
  const float* p = part + 2 * ((long long)b * nch * N1 + j);
  if (mode == 0) {
    float mx = -INFINITY;
    for (int c = 0; c < nch; ++c) mx = fmaxf(mx, p[2 * (long long)c * N1]);
    float sum = 0.f;
    for (int c = 0; c < nch; ++c) {
      const float mc = p[2 * (long long)c * N1];
      sum += mc == -INFINITY ? 0.f : p[2 * (long long)c * N1 + 1] * expf(mc - mx);
    }
    out[t] = (j < N1 - 1 ? norm : lnu_last) - (mx + logf(sum));
  } else {
    float sum = 0.f;
    for (int c = 0; c < nch; ++c) sum += p[2 * (long long)c * N1 + 1];
    out[t] = sum;
  }
}

// One backward step t in ONE read of C (N1 <= 64 SKF_Q): a workgroup owns SKF_R rows of one pair,
// a wave one row at a time held in registers (lane: columns l + 64 q).  The row's
// gu_i = base_i - sum_j gv_j pc_ij (pc = v_t's softmax weights, kept in registers) is
// sk_row_kernel mode 1's sum in the same order; with gu_i known the same registers give
// pr_ij (u_t's weights), the in-place gC -= gv_j pc + gu_i pr, and the wave's column sums of
// gu_i pr, combined over the four waves in order and written per workgroup: d/d v_{t-1} is then
// minus the ordered sum of the partials (sk_bwd_colsum_kernel).  Against the row + column pair of
// passes: C is read once instead of twice per step.  The C and gC rows are loaded unconditionally
// (columns past N1 read the next row or the 64 * SKF_Q floats of slack every couplings-shaped buffer
// carries, and are never used) so all 66 loads are in flight at once; pc is recomputed rather
// than kept, which holds the kernel at two waves per SIMD.
// DEFER: the step leaves gC alone (it only forms d/d u_t and the partials of d/d v_{t-1}); every
// step's gC term is added afterwards in one pass (sk_bwd_accum_kernel), in the same order and with
// the same expressions, so gC is bit-identical and the steps read C only.
// The four waves' column sums are combined through ONE LDS row, wave by wave in order
// (((w0 + w1) + w2) + w3, the order of the former four-row buffer): 34 KB of LDS instead of 59 KB,
// four workgroups per CU instead of two.
constexpr int SKF_Q = 33, SKF_R = 32;

template <bool DEFER>
__global__ __launch_bounds__(256) void sk_bwd_fused_kernel(const float* Cc, int M1, int N1, const float* u,
                                                           const float* v, const float* vp, const float* gv,
                                                           const float* base, float* gC, float norm, float lmu_last,
                                                           float lnu_last, float* gu_out, float* part) {
  __shared__ float v_s[64 * SKF_Q], vp_s[64 * SKF_Q], gv_s[64 * SKF_Q];
  __shared__ float red[64 * SKF_Q];
  const int b = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const long long pb = (long long)b * N1;
  for (int j = threadIdx.x; j < N1; j += 256) {
    v_s[j] = v[pb + j];
    vp_s[j] = vp ? vp[pb + j] : 0.f;
    gv_s[j] = gv[pb + j];
  }
  __syncthreads();
  float cs[SKF_Q];
#pragma unroll
  for (int q = 0; q < SKF_Q; ++q) cs[q] = 0.f;
  const int i0 = blockIdx.x * SKF_R, i1 = min(M1, i0 + SKF_R);
  for (int i = i0 + w; i < i1; i += 4) {
    const long long row = (long long)b * M1 + i;
    const float* c = Cc + row * N1;
    float* g = gC + row * N1;
    const float ui = u[row], lmu = i < M1 - 1 ? norm : lmu_last;
    float x[SKF_Q], gx[SKF_Q];  // the gC row is read with C (its latency under the sums)
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < SKF_Q; ++q) {  // unconditional loads (one base, immediate offsets): all in flight
      x[q] = c[l + 64 * q];             // past the row end: the next row / the buffers' 64-float slack,
      if (!DEFER) gx[q] = g[l + 64 * q];  // never used
    }
#pragma unroll
    for (int q = 0; q < SKF_Q; ++q) {
      const int j = l + 64 * q;
      if (j < N1) acc = fmaf(gv_s[j], exp_fast(x[q] + ui + v_s[j] - (j < N1 - 1 ? norm : lnu_last)), acc);
    }
    acc = wave_sum(acc);
    const float gui = (base ? base[row] : 0.f) - acc;
    if (l == 0) gu_out[row] = gui;
#pragma unroll
    for (int q = 0; q < SKF_Q; ++q) {
      const int j = l + 64 * q;
      if (j < N1) {
        const float pr = exp_fast(x[q] + vp_s[j] + ui - lmu);
        cs[q] = fmaf(gui, pr, cs[q]);
        if (!DEFER) {
          const float pc = exp_fast(x[q] + ui + v_s[j] - (j < N1 - 1 ? norm : lnu_last));  // recomputed: registers
          g[j] = gx[q] - fmaf(gv_s[j], pc, gui * pr);
        }
      }
    }
  }
  for (int k = 0; k < 4; ++k) {  // ((w0 + w1) + w2) + w3 through one LDS row
    if (w == k) {
#pragma unroll
      for (int q = 0; q < SKF_Q; ++q) red[l + 64 * q] = k == 0 ? cs[q] : red[l + 64 * q] + cs[q];
    }
    __syncthreads();
  }
  float* pp = part + ((long long)b * gridDim.x + blockIdx.x) * N1;
  for (int j = threadIdx.x; j < N1; j += 256) pp[j] = red[j];
}

// gC_ij -= sum over t = T .. 1 of (gv_t,j pc_t,ij + gu_t,i pr_t,ij): the deferred terms of the
// DEFER steps, each formed exactly as sk_bwd_fused_kernel<false> forms it and subtracted in the
// same order.  A workgroup = 32 rows x 256 columns of one pair, a thread one column (its 32 gC and
// C values in registers); the rows' u_t, gu_t of every step staged in LDS once.
constexpr int SKA_R = 32, SKA_TMAX = 128;
__global__ __launch_bounds__(256) void sk_bwd_accum_kernel(const float* Cc, int B, int M1, int N1, int T, const float* U,
                                                           const float* V, const float* GU, const float* GV, float* gC,
                                                           float norm, float lmu_last, float lnu_last) {
  __shared__ float u_s[SKA_TMAX][SKA_R], gu_s[SKA_TMAX][SKA_R];
  const int b = blockIdx.z, i0 = blockIdx.y * SKA_R, j = blockIdx.x * 256 + threadIdx.x;
  const int nr = min(SKA_R, M1 - i0);
  for (int k = threadIdx.x; k < T * SKA_R; k += 256) {
    const int t = k / SKA_R, r = k - t * SKA_R;
    const long long o = ((long long)t * B + b) * M1 + i0 + r;
    u_s[t][r] = r < nr ? U[o] : 0.f;
    gu_s[t][r] = r < nr ? GU[o] : 0.f;
  }
  __syncthreads();
  if (j >= N1) return;
  const long long base = ((long long)b * M1 + i0) * N1 + j;
  float x[SKA_R], g[SKA_R];
#pragma unroll
  for (int r = 0; r < SKA_R; ++r) {
    x[r] = r < nr ? Cc[base + (long long)r * N1] : 0.f;
    g[r] = r < nr ? gC[base + (long long)r * N1] : 0.f;
  }
  const float lnu = j < N1 - 1 ? norm : lnu_last;
  for (int t = T; t >= 1; --t) {
    const float v = V[((long long)t * B + b) * N1 + j];
    const float vp = t > 1 ? V[((long long)(t - 1) * B + b) * N1 + j] : 0.f;
    const float gv = GV[((long long)(t - 1) * B + b) * N1 + j];
#pragma unroll
    for (int r = 0; r < SKA_R; ++r) {
      const float ui = u_s[t - 1][r], gui = gu_s[t - 1][r];
      const float lmu = i0 + r < M1 - 1 ? norm : lmu_last;
      const float pr = exp_fast(x[r] + vp + ui - lmu);
      const float pc = exp_fast(x[r] + ui + v - lnu);
      g[r] = g[r] - fmaf(gv, pc, gui * pr);
    }
  }
#pragma unroll
  for (int r = 0; r < SKA_R; ++r)
    if (r < nr) gC[base + (long long)r * N1] = g[r];
}

// One forward iteration in ONE read of C (N1 <= 64 SKF_Q; the eval path's scaled column
// statistics, sinkhorn.hip): a wave holds row i of C + v_{t-1} in registers, takes its max m_i and
// s_i = sum_j e_ij with e_ij = exp(C_ij + v_{t-1,j} - m_i) <= 1 and writes
// u_i = lmu_i - (m_i + log s_i); with a_i = exp(lmu_i) / s_i, e_ij a_i = exp(C_ij + u_i + v_{t-1,j}),
// so the column statistic is the plain sum S_j = sum_i e_ij a_i (no per-column max, no second
// exponential) and v_j = lnu_j + v_{t-1,j} - log S_j.  e_ij a_i <= exp(lmu_i) never overflows; a
// column whose S_j falls below 1e-20 (underflowed terms could matter) is recomputed exactly by
// sk_fwd_colfinal_kernel.  Partials per workgroup as in the backward.
__global__ __launch_bounds__(256) void sk_fwd_fused_kernel(const float* Cc, int M1, int N1, const float* vprev,
                                                           float norm, float lmu_last, float* u_out, float* part) {
  __shared__ float v_s[64 * SKF_Q];
  __shared__ float red[64 * SKF_Q];
  const int b = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const long long pb = (long long)b * N1;
  for (int j = threadIdx.x; j < N1; j += 256) v_s[j] = vprev[pb + j];
  __syncthreads();
  float cs[SKF_Q];
#pragma unroll
  for (int q = 0; q < SKF_Q; ++q) cs[q] = 0.f;
  const int i0 = blockIdx.x * SKF_R, i1 = min(M1, i0 + SKF_R);
  for (int i = i0 + w; i < i1; i += 4) {
    const long long row = (long long)b * M1 + i;
    const float* c = Cc + row * N1;
    const float lmu = i < M1 - 1 ? norm : lmu_last;
    float x[SKF_Q];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < SKF_Q; ++q) x[q] = c[l + 64 * q];  // unconditional (slack past the end), all in flight
#pragma unroll
    for (int q = 0; q < SKF_Q; ++q) {
      const int j = l + 64 * q;
      x[q] = j < N1 ? x[q] + v_s[j] : -INFINITY;
      m = fmaxf(m, x[q]);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < SKF_Q; ++q) {
      x[q] = exp_fast(x[q] - m);  // 0 on the padding
      sum += x[q];
    }
    sum = wave_sum(sum);
    if (l == 0) u_out[row] = lmu - (m + logf(sum));
    const float a = expf(lmu) / sum;
#pragma unroll
    for (int q = 0; q < SKF_Q; ++q) cs[q] = fmaf(x[q], a, cs[q]);
  }
  for (int k = 0; k < 4; ++k) {  // ((w0 + w1) + w2) + w3 through one LDS row
    if (w == k) {
#pragma unroll
      for (int q = 0; q < SKF_Q; ++q) red[l + 64 * q] = k == 0 ? cs[q] : red[l + 64 * q] + cs[q];
    }
    __syncthreads();
  }
  float* pp = part + ((long long)b * gridDim.x + blockIdx.x) * N1;
  for (int j = threadIdx.x; j < N1; j += 256) pp[j] = red[j];
}

// s += p[k * ld] for k = 0 .. n-1 in order, eight loads in flight ahead of their adds
__device__ __forceinline__ float ordered_sum(const float* p, long long ld, int n) {
  float s = 0.f;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = p[(long long)(k + u) * ld];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += t[u];
  }
  for (; k < n; ++k) s += p[(long long)k * ld];
  return s;
}

// v_j = lnu_j + v_{t-1,j} - log(ordered sum of the partials); exact two-pass LSE_i(C_ij + u_i) over
// the column when that sum is below thr (1e-20; LG_SKF_EXACT=1 in the environment: every column,
// which is how the tests reach this path -- the dustbin row keeps S_j near 1 / (M + N) in practice)
__global__ void sk_fwd_colfinal_kernel(const float* part, const float* Cc, const float* u, const float* vprev, int B,
                                       int M1, int N1, int nwg, float norm, float lnu_last, float thr, float* v) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)B * N1) return;
  const int b = (int)(t / N1), j = (int)(t - (long long)b * N1);
  const float S = ordered_sum(part + (long long)b * nwg * N1 + j, N1, nwg);
  const float lnu = j < N1 - 1 ? norm : lnu_last;
  if (S >= thr) {
    v[t] = lnu + vprev[t] - logf(S);
    return;
  }
  const float* c = Cc + (long long)b * M1 * N1 + j;
  const float* ub = u + (long long)b * M1;
  float mx = -INFINITY;
  for (int i = 0; i < M1; ++i) mx = fmaxf(mx, c[(long long)i * N1] + ub[i]);
  float s = 0.f;
  for (int i = 0; i < M1; ++i) s += expf(c[(long long)i * N1] + ub[i] - mx);
  v[t] = lnu - (mx + logf(s));
}

// d/d v_{t-1}[b][j] = -(ordered sum over the workgroups' partials)
__global__ void sk_bwd_colsum_kernel(const float* part, int B, int N1, int nwg, float* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)B * N1) return;
  const int b = (int)(t / N1), j = (int)(t - (long long)b * N1);
  out[t] = -ordered_sum(part + (long long)b * nwg * N1 + j, N1, nwg);
}

// Z = C + u_i + v_j - norm (:178,200), one workgroup per row
__global__ __launch_bounds__(256) void sk_out_kernel(const float* Cc, const float* u, const float* v, int B, int M1, int N1,
                                                     float norm, float* Z) {
  const int row = blockIdx.x, b = row / M1;
  const float ui = u[row];
  const float* vb = v + (long long)b * N1;
  const float* c = Cc + (long long)row * N1;
  float* z = Z + (long long)row * N1;
  for (int j = threadIdx.x; j < N1; j += 256) z[j] = c[j] + ui + vb[j] - norm;
}

// d/d cost = gC's inner block (+ gext); part[b] = sum of gC over pair b's dustbin entries
__global__ __launch_bounds__(256) void sk_finish_kernel(const float* gC, const float* gext, int M, int N, float* gcost,
                                                        float* part) {
  __shared__ float red[256];
  const int b = blockIdx.y;
  const long long M1 = M + 1, N1 = N + 1;
  const float* g = gC + (long long)b * M1 * N1;
  if (blockIdx.x > 0) {  // inner block copy
    const long long per = (long long)M * N;
    for (long long e = (long long)(blockIdx.x - 1) * 256 + threadIdx.x; e < per; e += (long long)(gridDim.x - 1) * 256) {
      const long long r = e / N, c = e - r * N;
      float x = g[r * N1 + c];
      if (gext) x += gext[(long long)b * per + e];
      gcost[(long long)b * per + e] = x;
    }
    return;
  }
  float s = 0.f;
  for (long long r = threadIdx.x; r < M; r += 256) s += g[r * N1 + N];
  for (long long c = threadIdx.x; c <= N; c += 256) s += g[M * N1 + c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[b] = red[0];
}

__global__ void sk_alpha_kernel(const float* part, int B, float* galpha) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += part[b];
  galpha[0] = s;
}

// d/d log_assignment of SuperGlue.loss (mode 0, superglue.py:309-339) or NLLLoss (mode 1,
// losses.py:26-73) from d/d (nll, nll_pos, nll_neg) [3][B] (rows nullable) and the forward's
// out [5][B] (num_matchable, num_unmatchable).  Linear in la: gLA = -(c_in * positive) on the
// inner block, -(c_dust * negative) on the dustbins (NLLLoss: the column dustbin written at
// [:, -1, :m], losses.py:72), 0 elsewhere.
__global__ __launch_bounds__(256) void sg_nll_grad_kernel(const uint8_t* gta, const int64_t* gt0, const int64_t* gt1,
                                                          const float* stats, const float* g_nll, const float* g_pos,
                                                          const float* g_neg, int B, int M, int N, int mode, float bal,
                                                          float* gla) {
  const int row = blockIdx.x, b = row / (M + 1), r = row - b * (M + 1);  // one workgroup per row
  const float gn = g_nll ? g_nll[b] : 0.f;
  const float num_pos = stats[3 * B + b];
  const float num_neg = mode == 0 ? stats[4 * B + b] : 2.f * stats[4 * B + b];
  const float c_in = (bal * gn + (g_pos ? g_pos[b] : 0.f)) / num_pos;
  const float c_dust = ((1.f - bal) * gn + (g_neg ? g_neg[b] : 0.f)) / num_neg;
  float* out = gla + (long long)row * (N + 1);
  if (r < M) {
    const uint8_t* a = gta + ((long long)b * M + r) * N;
    for (int c = threadIdx.x; c < N; c += 256) out[c] = a[c] ? -c_in : -0.f;
    if (threadIdx.x == 0) out[N] = gt0[(long long)b * M + r] == -1 ? -c_dust : -0.f;
  } else {
    // NLLLoss writes the column dustbins at [:, -1, :m] from gt_matches1 (M == N there)
    for (int c = threadIdx.x; c < N; c += 256) out[c] = gt1[(long long)b * N + c] == -1 ? -c_dust : -0.f;
    if (threadIdx.x == 0) out[N] = -0.f;
  }
}

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }


// column pass (pass 1 + pass 2); part: sk_col_part_floats
size_t sk_col_part_floats(int B, int M, int N) { return 2 * (size_t)B * cdiv(M + 1, SK_CH) * (N + 1); }

void sk_col(const float* Cc, int B, int M1, int N1, const float* u, const float* v, const float* vp, const float* gu,
            const float* gv, float* gC, float norm, float lmu_last, float lnu_last, int mode, float* part, float* out,
            hipStream_t st) {
  const int nch = cdiv(M1, SK_CH);
  hipLaunchKernelGGL(sk_col_part_kernel, dim3(cdiv(N1, 64), nch, B), dim3(256), 0, st, Cc, B, M1, N1, u, v, vp, gu, gv,
                     gC, norm, lmu_last, lnu_last, mode, part);
  hipLaunchKernelGGL(sk_col_final_kernel, dim3(cdiv((long long)B * N1, 256)), dim3(256), 0, st, part, B, N1, nch, norm,
                     lnu_last, mode, out);
}

}  // namespace

// ------------------------------------------------------------------ launchers
size_t bn_part_floats(int rows, int C) { return 2 * (size_t)cdiv(rows, BN_RB) * C + 2 * (size_t)C; }

hipError_t bn_train_fwd(const float* X, long long ldx, int rows, int C, const float* gamma, const float* beta,
                        float* Y, long long ldy, float* stats, float* part, hipStream_t st) {
  if (C % 4 || C > 1024 || rows < 2) return hipErrorInvalidValue;
  const int nb = cdiv(rows, BN_RB);
  float *mean = stats, *rstd = stats + C, *varu = stats + 2 * C;
  hipLaunchKernelGGL(bn_part_kernel, dim3(nb), dim3(256), 0, st, X, ldx, rows, C, 0, nullptr, nullptr, nullptr, nullptr,
                     nullptr, 0ll, part, nullptr);
  hipLaunchKernelGGL(bn_final_kernel, dim3(cdiv(C, 16)), dim3(256), 0, st, part, nullptr, nb, C, rows, 0, mean, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  hipLaunchKernelGGL(bn_part_kernel, dim3(nb), dim3(256), 0, st, X, ldx, rows, C, 1, mean, nullptr, nullptr, nullptr,
                     nullptr, 0ll, part, nullptr);
  hipLaunchKernelGGL(bn_final_kernel, dim3(cdiv(C, 16)), dim3(256), 0, st, part, nullptr, nb, C, rows, 1, nullptr, rstd,
                     varu, nullptr, nullptr, nullptr, nullptr, 0);
  hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(cdiv((long long)rows * (C / 4), 256)), dim3(256), 0, st, X, ldx, rows, C,
                     mean, rstd, gamma, beta, Y, ldy);
  return hipGetLastError();
}

hipError_t bn_train_bwd(const float* X, long long ldx, const float* dY, long long ldy, int rows, int C,
                        const float* stats, const float* gamma, const float* beta, float* dX, long long lddx,
                        float* dgamma, float* dbeta, int accum, float* part, hipStream_t st) {
  if (C % 4 || C > 1024 || rows < 2) return hipErrorInvalidValue;
  const int nb = cdiv(rows, BN_RB);
  const float *mean = stats, *rstd = stats + C;
  float* p0 = part;
  float* p1 = part + (size_t)nb * C;
  float* s01 = part + 2 * (size_t)nb * C;  // [2][C]: sum dy', sum dy' xhat
  hipLaunchKernelGGL(bn_part_kernel, dim3(nb), dim3(256), 0, st, X, ldx, rows, C, 2, mean, rstd, gamma, beta, dY, ldy, p0,
                     p1);
  hipLaunchKernelGGL(bn_final_kernel, dim3(cdiv(C, 16)), dim3(256), 0, st, p0, p1, nb, C, rows, 2, nullptr, nullptr,
                     nullptr, s01, s01 + C, dgamma, dbeta, accum);
  hipLaunchKernelGGL(bn_apply_bwd_kernel, dim3(cdiv((long long)rows * (C / 4), 256)), dim3(256), 0, st, X, ldx, dY, ldy,
                     rows, C, mean, rstd, gamma, beta, s01, s01 + C, dX, lddx);
  return hipGetLastError();
}

size_t bn_sync_floats() { return 4 * 1024 + 2; }

hipError_t bn_train_fwd_sets(const float* X, long long ldx, const int* rows, int C, const float* gamma,
                             const float* beta, float* Y, long long ldy, float* stats, float* part, const BnSync* sync,
                             hipStream_t st) {
  const long long off[2] = {0, (long long)rows[0]};
  if (!sync || !sync->fn) {
    for (int set = 0; set < 2; ++set) {
      const hipError_t e = bn_train_fwd(X + off[set] * ldx, ldx, rows[set], C, gamma, beta, Y + off[set] * ldy, ldy,
                                        stats + set * 3 * C, part, st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  if (C % 4 || C > 1024 || rows[0] < 1 || rows[1] < 1 || sync->cap < (int64_t)bn_sync_floats()) return hipErrorInvalidValue;
  float* buf = sync->buf;
  // pass 1: sums -> global mean; pass 2: centred sums of squares about it -> global variance
  for (int pass = 0; pass < 2; ++pass) {
    for (int set = 0; set < 2; ++set) {
      const int nb = cdiv(rows[set], BN_RB);
      float* mean = stats + set * 3 * C;
      hipLaunchKernelGGL(bn_part_kernel, dim3(nb), dim3(256), 0, st, X + off[set] * ldx, ldx, rows[set], C, pass,
                         pass ? mean : nullptr, nullptr, nullptr, nullptr, nullptr, 0ll, part, nullptr);
      hipLaunchKernelGGL(bn_final_kernel, dim3(cdiv(C, 16)), dim3(256), 0, st, part, nullptr, nb, C, rows[set], 3, nullptr,
                         nullptr, nullptr, buf + set * C, nullptr, nullptr, nullptr, 0, buf + 2 * C + set);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sync->fn(sync->ctx, 2 * (int64_t)C + 2, st) != 0) return hipErrorUnknown;
    for (int set = 0; set < 2; ++set) {
      float* s3 = stats + set * 3 * C;
      hipLaunchKernelGGL(bn_sync_finish_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, buf, C, set, pass, s3, s3 + C,
                         s3 + 2 * C);
    }
  }
  for (int set = 0; set < 2; ++set) {
    const float* s3 = stats + set * 3 * C;
    hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(cdiv((long long)rows[set] * (C / 4), 256)), dim3(256), 0, st,
                       X + off[set] * ldx, ldx, rows[set], C, s3, s3 + C, gamma, beta, Y + off[set] * ldy, ldy);
  }
  return hipGetLastError();
}

hipError_t bn_train_bwd_sets(const float* X, long long ldx, const float* dY, long long ldy, const int* rows, int C,
                             const float* stats, const float* gamma, const float* beta, float* dX, long long lddx,
                             float* dgamma, float* dbeta, float* part, const BnSync* sync, hipStream_t st) {
  const long long off[2] = {0, (long long)rows[0]};
  if (!sync || !sync->fn) {
    for (int set = 0; set < 2; ++set) {
      const hipError_t e = bn_train_bwd(X + off[set] * ldx, ldx, dY + off[set] * ldy, ldy, rows[set], C,
                                        stats + set * 3 * C, gamma, beta, dX + off[set] * lddx, lddx, dgamma, dbeta, set,
                                        part, st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  if (C % 4 || C > 1024 || rows[0] < 1 || rows[1] < 1 || sync->cap < (int64_t)bn_sync_floats()) return hipErrorInvalidValue;
  // buf: [set][sum dy' | sum dy' xhat] [2][2][C], counts at 4C + set.  gamma / beta take the
  // rank's own sums (the data-parallel gradient average sums them over the ranks)
  float* buf = sync->buf;
  for (int set = 0; set < 2; ++set) {
    const int nb = cdiv(rows[set], BN_RB);
    const float* s3 = stats + set * 3 * C;
    float* p0 = part;
    float* p1 = part + (size_t)nb * C;
    hipLaunchKernelGGL(bn_part_kernel, dim3(nb), dim3(256), 0, st, X + off[set] * ldx, ldx, rows[set], C, 2, s3, s3 + C,
                       gamma, beta, dY + off[set] * ldy, ldy, p0, p1);
    hipLaunchKernelGGL(bn_final_kernel, dim3(cdiv(C, 16)), dim3(256), 0, st, p0, p1, nb, C, rows[set], 2, nullptr,
                       nullptr, nullptr, buf + set * 2 * C, buf + set * 2 * C + C, dgamma, dbeta, set,
                       buf + 4 * C + set);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (sync->fn(sync->ctx, 4 * (int64_t)C + 2, st) != 0) return hipErrorUnknown;
  for (int set = 0; set < 2; ++set) {
    const float* s3 = stats + set * 3 * C;
    hipLaunchKernelGGL(bn_apply_bwd_kernel, dim3(cdiv((long long)rows[set] * (C / 4), 256)), dim3(256), 0, st,
                       X + off[set] * ldx, ldx, dY + off[set] * ldy, ldy, rows[set], C, s3, s3 + C, gamma, beta,
                       buf + set * 2 * C, buf + set * 2 * C + C, dX + off[set] * lddx, lddx, buf + 4 * C + set);
  }
  return hipGetLastError();
}

hipError_t bn_running_update(float* rm, float* rv, const float* stats, int C, float momentum, hipStream_t st) {
  hipLaunchKernelGGL(bn_running_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, rm, rv, stats, stats + 2 * C, C, momentum);
  return hipGetLastError();
}

hipError_t kenc_input(const float* kpts, const float* scores, const float* size, float w, float h, int B, int n, int cin,
                      float* out, hipStream_t st) {
  hipLaunchKernelGGL(kenc_input_kernel, dim3(cdiv((long long)B * n, 256)), dim3(256), 0, st, kpts, scores, size, w, h, B, n,
                     cin, out);
  return hipGetLastError();
}

// up to 8 gathers in one launch (blockIdx.y = the gather): a layer's q / k / v / merge weights and biases
__global__ void head_gather_multi_kernel(HeadGathers g) {
  const HeadGather& e = g.e[blockIdx.y];
  const int n = e.rows * e.cols;
  auto perm = [](int k) { return (k & 63) * 4 + (k >> 6); };
  auto iperm = [](int k) { return (k & 3) * 64 + (k >> 2); };
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int r = i / e.cols, c = i - r * e.cols;
    int sr = r, sc = c;
    if (e.by_cols) sc = e.inverse ? iperm(c) : perm(c);
    else sr = e.inverse ? iperm(r) : perm(r);
    e.dst[i] = e.src[(long long)sr * e.cols + sc];
  }
}
hipError_t head_gather_multi(const HeadGathers& g, hipStream_t st) {
  if (g.n <= 0) return hipSuccess;
  if (g.n > 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(head_gather_multi_kernel, dim3(64, g.n), dim3(256), 0, st, g);
  return hipGetLastError();
}

hipError_t head_gather(const float* src, int rows, int cols, bool by_cols, bool inverse, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(head_gather_kernel, dim3(cdiv((long long)rows * cols, 256)), dim3(256), 0, st, src, rows, cols,
                     (int)by_cols, (int)inverse, dst);
  return hipGetLastError();
}

static bool skf_ok(int N1) { return N1 <= 64 * SKF_Q; }
static size_t skf_part_floats(int B, int M, int N) { return (size_t)B * cdiv(M + 1, SKF_R) * (N + 1); }

size_t sk_train_part_floats(int B, int M, int N) { return std::max(sk_col_part_floats(B, M, N), skf_part_floats(B, M, N)); }

hipError_t sk_train_forward(const float* cost, const float* alpha, int B, int M, int N, int iters, float* Cc, float* U,
                            float* V, float* Z, float* part, hipStream_t st) {
  const int M1 = M + 1, N1 = N + 1;
  const float norm = -logf((float)(M + N)), lmu_last = logf((float)N) + norm, lnu_last = logf((float)M) + norm;
    hipLaunchKernelGGL(sk_couplings_kernel, dim3(B * M1), dim3(256), 0, st, cost, alpha, B, M, N, Cc);
  hipError_t e = hipMemsetAsync(V, 0, (size_t)B * N1 * sizeof(float), st);  // v_0 = 0 (:175)
  if (e != hipSuccess) return e;
  const char* ex = getenv("LG_SKF_EXACT");
  const float thr = ex && atoi(ex) ? INFINITY : 1e-20f;
  for (int t = 1; t <= iters; ++t) {
    float* u = U + (size_t)(t - 1) * B * M1;
    const float* vprev = V + (size_t)(t - 1) * B * N1;
    float* v = V + (size_t)t * B * N1;
    if (skf_ok(N1)) {  // both halves of the iteration in one pass over C
      const unsigned nwg = cdiv(M1, SKF_R);
      hipLaunchKernelGGL(sk_fwd_fused_kernel, dim3(nwg, B), dim3(256), 0, st, Cc, M1, N1, vprev, norm, lmu_last, u, part);
      hipLaunchKernelGGL(sk_fwd_colfinal_kernel, dim3(cdiv((long long)B * N1, 256)), dim3(256), 0, st, part, Cc, u, vprev,
                         B, M1, N1, (int)nwg, norm, lnu_last, thr, v);
      continue;
    }
    hipLaunchKernelGGL(sk_row_kernel, dim3(cdiv((long long)B * M1, 4)), dim3(256), 0, st, Cc, B, M1, N1, nullptr, vprev,
                       nullptr, nullptr, norm, lmu_last, lnu_last, 0, u);
    sk_col(Cc, B, M1, N1, u, nullptr, nullptr, nullptr, nullptr, nullptr, norm, lmu_last, lnu_last, 0, part, v, st);
  }
  const float* uT = iters > 0 ? U + (size_t)(iters - 1) * B * M1 : nullptr;
  if (!uT) {  // no iterations: u = v = 0
    e = hipMemsetAsync(U, 0, (size_t)B * M1 * sizeof(float), st);
    if (e != hipSuccess) return e;
    uT = U;
  }
  hipLaunchKernelGGL(sk_out_kernel, dim3(B * M1), dim3(256), 0, st, Cc, uT, V + (size_t)iters * B * N1, B, M1, N1, norm,
                     Z);
  return hipGetLastError();
}

size_t sk_train_row_slack_floats() { return 64 * SKF_Q; }

// the Sinkhorn backward's gC terms in one pass after the steps (sk_bwd_accum_kernel) where the fused
// step and the accumulation kernel take the shape
static bool sk_defer(int N1, int iters) { return skf_ok(N1) && iters >= 1 && iters <= SKA_TMAX; }

size_t sk_train_scratch_floats(int B, int M, int N, int iters) {
  // + every step's d/d u_t [T][B][M+1] and d/d v_t [T][B][N+1] for the deferred gC pass
  return (size_t)B * (M + 1) * (N + 1) + sk_train_row_slack_floats() + 4 * (size_t)B * (M + N + 2) + B +
         std::max(sk_col_part_floats(B, M, N), skf_part_floats(B, M, N)) + 256 +
         (size_t)std::max(iters, 0) * B * (M + N + 2) + 64;
}

hipError_t sk_train_backward(const float* Cc, const float* U, const float* V, const float* gZ, const float* gext, int B,
                             int M, int N, int iters, float* gcost, float* galpha, float* ws, hipStream_t st) {
  const int M1 = M + 1, N1 = N + 1;
  const float norm = -logf((float)(M + N)), lmu_last = logf((float)N) + norm, lnu_last = logf((float)M) + norm;
  const long long tot = (long long)B * M1 * N1;
  float* gC = ws;
  float* base = gC + tot + sk_train_row_slack_floats();  // [B][M1]: d/d u_T from Z (after gC's read slack)
  float* gu = base + (size_t)B * M1;        // [B][M1]
  float* gv = gu + (size_t)B * M1;          // [B][N1]: d/d v_t
  float* gv2 = gv + (size_t)B * N1;         // [B][N1]: d/d v_{t-1}
  float* part = gv2 + (size_t)B * N1;       // [B]
  float* cpart = part + B + 64;              // column-pass partials
  const bool defer = sk_defer(N1, iters);
  float* GUall = cpart + std::max(sk_col_part_floats(B, M, N), skf_part_floats(B, M, N)) + 256;  // [T][B][M1]
  float* GVall = GUall + (size_t)iters * B * M1;                                                // [T][B][N1]
  if (defer) gv = GVall + (size_t)(iters - 1) * B * N1;  // d/d v_T
  hipError_t e = hipMemcpyAsync(gC, gZ, tot * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return e;
  // Z = C + u_T + v_T - norm: d/d u_T = row sums of gZ, d/d v_T = column sums
  hipLaunchKernelGGL(sk_row_kernel, dim3(cdiv((long long)B * M1, 4)), dim3(256), 0, st, gZ, B, M1, N1, nullptr, nullptr,
                     nullptr, nullptr, norm, lmu_last, lnu_last, 2, base);
  sk_col(gZ, B, M1, N1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, norm, lmu_last, lnu_last, 2, cpart, gv, st);
  for (int t = iters; t >= 1; --t) {
    const float* u = U + (size_t)(t - 1) * B * M1;
    const float* v = V + (size_t)t * B * N1;
    const float* vp = t > 1 ? V + (size_t)(t - 1) * B * N1 : nullptr;  // v_0 = 0
    if (defer) {  // the step reads C only; its gC term waits for sk_bwd_accum_kernel
      const unsigned nwg = cdiv(M1, SKF_R);
      float* gut = GUall + (size_t)(t - 1) * B * M1;
      float* gvp = t > 1 ? GVall + (size_t)(t - 2) * B * N1 : gv2;  // d/d v_{t-1} (v_0 = 0: unused)
      hipLaunchKernelGGL((sk_bwd_fused_kernel<true>), dim3(nwg, B), dim3(256), 0, st, Cc, M1, N1, u, v, vp, gv,
                         t == iters ? base : nullptr, gC, norm, lmu_last, lnu_last, gut, cpart);
      hipLaunchKernelGGL(sk_bwd_colsum_kernel, dim3(cdiv((long long)B * N1, 256)), dim3(256), 0, st, cpart, B, N1, (int)nwg,
                         gvp);
      gv = gvp;
      continue;
    }
    if (skf_ok(N1)) {  // both halves of the step in one pass over C
      const unsigned nwg = cdiv(M1, SKF_R);
      hipLaunchKernelGGL((sk_bwd_fused_kernel<false>), dim3(nwg, B), dim3(256), 0, st, Cc, M1, N1, u, v, vp, gv,
                         t == iters ? base : nullptr, gC, norm, lmu_last, lnu_last, gu, cpart);
      hipLaunchKernelGGL(sk_bwd_colsum_kernel, dim3(cdiv((long long)B * N1, 256)), dim3(256), 0, st, cpart, B, N1, (int)nwg,
                         gv2);
      std::swap(gv, gv2);
      continue;
    }
    // v_t = lnu - LSE_i(C + u_t): d/d u_t = base (t = T) - sum_j gv_j pc
    hipLaunchKernelGGL(sk_row_kernel, dim3(cdiv((long long)B * M1, 4)), dim3(256), 0, st, Cc, B, M1, N1, u, v, gv,
                       t == iters ? base : nullptr, norm, lmu_last, lnu_last, 1, gu);
    // u_t = lmu - LSE_j(C + v_{t-1}): d/d v_{t-1}, and both steps' d/d C
    sk_col(Cc, B, M1, N1, u, v, vp, gu, gv, gC, norm, lmu_last, lnu_last, 1, cpart, gv2, st);
    std::swap(gv, gv2);
  }
  if (defer) {
    hipLaunchKernelGGL(sk_bwd_accum_kernel, dim3(cdiv(N1, 256), cdiv(M1, SKA_R), B), dim3(256), 0, st, Cc, B, M1, N1, iters,
                       U, V, GUall, GVall, gC, norm, lmu_last, lnu_last);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const long long per = (long long)M * N;
  const unsigned gx = 1 + (unsigned)std::min<long long>(cdiv(per, 256), 4096);
  hipLaunchKernelGGL(sk_finish_kernel, dim3(gx, B), dim3(256), 0, st, gC, gext, M, N, gcost, part);
  if (galpha) hipLaunchKernelGGL(sk_alpha_kernel, dim3(1), dim3(64), 0, st, part, B, galpha);
  return hipGetLastError();
}

hipError_t sg_nll_grad(const uint8_t* gta, const int64_t* gt0, const int64_t* gt1, const float* stats, const float* g_nll,
                       const float* g_pos, const float* g_neg, int B, int M, int N, int mode, float bal, float* gla,
                       hipStream_t st) {
  const long long tot = (long long)B * (M + 1) * (N + 1);
  if (tot == 0) return hipSuccess;
  hipLaunchKernelGGL(sg_nll_grad_kernel, dim3(B * (M + 1)), dim3(256), 0, st, gta, gt0, gt1, stats, g_nll, g_pos, g_neg, B,
                     M, N, mode, bal, gla);
  return hipGetLastError();
}

}  // namespace lg
