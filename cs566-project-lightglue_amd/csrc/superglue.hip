#include <algorithm>
// SuperGlue pieces that are not shared with LightGlue (gluefactory_nonfree/superglue.py):
//   the keypoint encoder (normalize_keypoints + MLP with eval BatchNorm, :75-104) added to the
//   descriptors, load-time weight folds / permutations, and the NLL losses (:309-339 and
//   gluefactory/models/utils/losses.py).  The GNN runs on the LightGlue kernels (superglue_api.cpp).
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace lg {

namespace {
constexpr int kEncRows = 32;  // keypoints per workgroup
constexpr int kEncMaxC = 256;
}  // namespace

// One workgroup = 32 keypoints of one image set; activations in LDS, layer by layer.  Layer l:
// out[o] = b[o] + sum_c Wt[c][o] in[c] (sequential over c, fp32; a thread computes 4 consecutive
// outputs of one keypoint from float4 weight reads), then -- where the layer has a BatchNorm --
// eval BatchNorm in ATen's CPU form (alpha = w / sqrt(var + eps), out * alpha + (b - mean * alpha))
// and ReLU.  The last layer computed here writes global rows: out[r] = (desc[r] +) value.
__global__ __launch_bounds__(256) void sg_kenc_kernel(SgEncArgs a) {
  constexpr int AS = kEncMaxC + 4;  // LDS row stride (float4-aligned rows)
  __shared__ __attribute__((aligned(16))) float act[2][kEncRows][AS];
  __shared__ int live[kEncRows];  // a ragged batch: the keypoint is a real point of its pair
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * kEncRows;
  const int nrow = min(kEncRows, a.rows - row0);
  // inputs: normalised keypoint (x, y) and the score (superglue.py:82-86, 97-101)
  if (tid < kEncRows) {
    const int r = row0 + tid;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    const bool on = tid < nrow && (!a.cnt || r - (r / a.n) * a.n < a.cnt[r / a.n]);
    live[tid] = on;
    if (on) {
      const int b = r / a.n;
      const float w = a.size ? a.size[2 * b] : a.fw, h = a.size ? a.size[2 * b + 1] : a.fh;
      const float scale = fmaxf(w, h) * 0.7f;
      v0 = (a.kpts[2 * (size_t)r] - w / 2.f) / scale;
      v1 = (a.kpts[2 * (size_t)r + 1] - h / 2.f) / scale;
      // per-keypoint score; in endpoints mode the array holds one score per LINE (rows / 2
      // entries) and is read below
      if (a.scores && !a.endpoints) v2 = a.scores[r];
    }
    act[0][tid][0] = v0;
    act[0][tid][1] = v1;
    act[0][tid][2] = v2;
    if (a.endpoints) {
      // EndPtEncoder (gluestick.py:495-514): rows are line endpoints [B][2L][2], a.n = 2L; channels
      // x, y, the offset to the line's other endpoint (row r ^ 1), and the line score, which the
      // reference lays out as scores.repeat(1, 2): endpoint column c reads line c mod L
      float o0 = 0.f, o1 = 0.f;
      if (on) {
        const int b = r / a.n, c = r - b * a.n, nl = a.n / 2;
        const float w = a.size ? a.size[2 * b] : a.fw, h = a.size ? a.size[2 * b + 1] : a.fh;
        const float scale = fmaxf(w, h) * 0.7f;
        const size_t q = (size_t)(r ^ 1);
        o0 = (a.kpts[2 * q] - w / 2.f) / scale - v0;
        o1 = (a.kpts[2 * q + 1] - h / 2.f) / scale - v1;
        v2 = a.scores[(size_t)b * nl + (c % nl)];
      }
      act[0][tid][2] = o0;
      act[0][tid][3] = o1;
      act[0][tid][4] = v2;
    }
  }
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < a.nl; ++l) {
    const int cin = a.ch[l], cout = a.ch[l + 1], og = cout / 4;
    const SgEncLayer& L = a.layer[l];
    const bool last = l == a.nl - 1;
    for (int idx = tid; idx < kEncRows * og; idx += blockDim.x) {
      const int k = idx / og, o = (idx - k * og) * 4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < cin; ++c) {
        const float x = act[cur][k][c];
        const f32x4 w = *reinterpret_cast<const f32x4*>(L.Wt + (size_t)c * cout + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(w[e], x, acc[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] += L.b[o + e];
        if (L.bn_w) {
          const float alpha = L.bn_w[o + e] * (1.f / sqrtf(L.bn_var[o + e] + 1e-5f));
          const float beta = L.bn_b[o + e] - L.bn_mean[o + e] * alpha;
          acc[e] = fmaxf(acc[e] * alpha + beta, 0.f);
        }
      }
      if (!last) {
        *reinterpret_cast<f32x4*>(&act[cur ^ 1][k][o]) = acc;
      } else if (live[k]) {
        const size_t r = (size_t)(row0 + k);
        if (a.desc) {
          const f32x4 d = *reinterpret_cast<const f32x4*>(a.desc + r * kEncMaxC + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = d[e] + acc[e];
        }
        *reinterpret_cast<f32x4*>(a.out + r * a.ldo + o) = acc;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

hipError_t sg_keypoint_encoder(const SgEncArgs& a, hipStream_t st) {
  if (a.rows <= 0) return hipSuccess;
  if (a.nl < 1 || a.nl > kSgMaxEnc || a.n <= 0 || !a.out || a.ldo < a.ch[a.nl]) return hipErrorInvalidValue;
  if (a.desc && a.ch[a.nl] != kEncMaxC) return hipErrorInvalidValue;
  if (a.endpoints) {  // x, y, offset, line score; endpoints come in pairs
    if (a.ch[0] != 5 || !a.scores || a.n % 2 || a.rows % a.n) return hipErrorInvalidValue;
  } else if (a.ch[0] < 2 || a.ch[0] > 3) {  // x, y (, keypoint score)
    return hipErrorInvalidValue;
  }
  for (int l = 1; l <= a.nl; ++l)
    if (a.ch[l] <= 0 || a.ch[l] > kEncMaxC || a.ch[l] % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sg_kenc_kernel, dim3((a.rows + kEncRows - 1) / kEncRows), dim3(256), 0, st, a);
  return hipGetLastError();
}

// dst[c][o] = src[o][c] (the encoder's weights, read coalesced over o)
__global__ void sg_transpose_kernel(const float* src, int rows, int cols, float* dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const int o = i / cols, c = i - o * cols;
  dst[(size_t)c * rows + o] = src[i];
}
hipError_t sg_transpose(const float* src, int rows, int cols, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(sg_transpose_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, st, src, rows, cols, dst);
  return hipGetLastError();
}

// dst[r][c] = src[r][idx[c]]
__global__ void sg_gather_cols_kernel(float* dst, const float* src, const int* idx, int rows, int cols) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const int r = i / cols, c = i - r * cols;
  dst[i] = src[(size_t)r * cols + idx[c]];
}
hipError_t sg_gather_cols(float* dst, const float* src, const int* idx, int rows, int cols, hipStream_t st) {
  hipLaunchKernelGGL(sg_gather_cols_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, st, dst, src, idx, rows, cols);
  return hipGetLastError();
}

// eval BatchNorm folded into the preceding linear: W[o][:] *= alpha[o], b[o] = b[o] alpha[o] + beta[o]
__global__ void sg_bn_fold_kernel(float* W, float* b, const float* g, const float* be, const float* mean, const float* var,
                                  int rows, int cols) {
  const int o = blockIdx.x;
  const float alpha = g[o] * (1.f / sqrtf(var[o] + 1e-5f));
  const float beta = be[o] - mean[o] * alpha;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) W[(size_t)o * cols + c] *= alpha;
  if (threadIdx.x == 0) b[o] = b[o] * alpha + beta;
}
hipError_t sg_bn_fold(float* W, float* b, const float* g, const float* be, const float* mean, const float* var, int rows,
                      int cols, hipStream_t st) {
  hipLaunchKernelGGL(sg_bn_fold_kernel, dim3(rows), dim3(256), 0, st, W, b, g, be, mean, var, rows, cols);
  return hipGetLastError();
}

// NLL of a log assignment [B][M+1][N+1] against a ground truth (one workgroup per pair; sums in
// fp64, one rounding to fp32 at the end).  out[k * B + b]: 0 nll, 1 nll_pos, 2 nll_neg,
// 3 num_matchable, 4 num_unmatchable.
//   mode 0 (SuperGlue.loss, superglue.py:309-339): num_pos = max(#pos, 1), num_neg = max(#neg0 +
//          #neg1, 1), nll_neg = (neg0 + neg1) / num_neg
//   mode 1 (losses.py NLLLoss + weight_loss): the dustbin row weights are written at [:, -1, :M]
//          (the caller checks M == N), counts clamped separately, num_unmatchable = (n0 + n1) / 2
// Pass 1: the inner block's positive sums, one workgroup per (pair, chunk of kNllRows rows), fp64
// partials [B][chunks][2]; pass 2 (one workgroup per pair): the partials in chunk order, the two
// dustbin sums and the loss terms.  Fixed reduction order: deterministic.  (One workgroup per pair
// over the whole [M, N] block took 5.3 ms per head at B = 32, N = 2048 -- the training loss runs it
// on every layer's head.)
constexpr int kNllRows = 16;
__global__ __launch_bounds__(256) void sg_nll_part_kernel(const float* la, int M, int N, const uint8_t* gta, double* part) {
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int r0 = chunk * kNllRows, r1 = min(M, r0 + kNllRows);
  double pos = 0.0, npos = 0.0;
  for (int r = r0; r < r1; ++r) {
    const float* L = la + ((size_t)b * (M + 1) + r) * (N + 1);
    const uint8_t* g = gta + ((size_t)b * M + r) * N;
    for (int c = tid; c < N; c += 256)
      if (g[c]) {
        pos += L[c];
        npos += 1.0;
      }
  }
  __shared__ double red[2][256];
  red[0][tid] = pos;
  red[1][tid] = npos;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      red[0][tid] += red[0][tid + st];
      red[1][tid] += red[1][tid + st];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[((size_t)b * gridDim.x + chunk) * 2] = red[0][0];
    part[((size_t)b * gridDim.x + chunk) * 2 + 1] = red[1][0];
  }
}

__global__ __launch_bounds__(256) void sg_nll_kernel(const float* la, int M, int N, const double* part, int nchunk,
                                                     const int64_t* gt0, const int64_t* gt1, int mode, float bal, int B,
                                                     float* out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* L = la + (size_t)b * (M + 1) * (N + 1);
  double neg0 = 0.0, n0 = 0.0, neg1 = 0.0, n1 = 0.0;
  for (int i = tid; i < M; i += blockDim.x)
    if (gt0[(size_t)b * M + i] == -1) {
      neg0 += L[(size_t)i * (N + 1) + N];
      n0 += 1.0;
    }
  for (int j = tid; j < N; j += blockDim.x)
    if (gt1[(size_t)b * N + j] == -1) {
      neg1 += L[(size_t)M * (N + 1) + j];
      n1 += 1.0;
    }
  __shared__ double red[4][256];
  red[0][tid] = neg0; red[1][tid] = n0; red[2][tid] = neg1; red[3][tid] = n1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    double P = 0.0, NPd = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      P += part[((size_t)b * nchunk + c) * 2];
      NPd += part[((size_t)b * nchunk + c) * 2 + 1];
    }
    const float NP = (float)NPd, G0 = (float)red[0][0], C0 = (float)red[1][0];
    const float G1 = (float)red[2][0], C1 = (float)red[3][0];
    float num_pos = fmaxf(NP, 1.f), nll_pos = -(float)P / num_pos, nll_neg, num_neg;
    if (mode == 0) {
      num_neg = fmaxf(C0 + C1, 1.f);
      nll_neg = (-G0 + -G1) / num_neg;
    } else {
      const float a0 = fmaxf(C0, 1.f), a1 = fmaxf(C1, 1.f);
      nll_neg = (-G0 + -G1) / (a0 + a1);
      num_neg = (a0 + a1) / 2.f;
    }
    const float nll = bal * nll_pos + (1.f - bal) * nll_neg;
    out[0 * B + b] = nll;
    out[1 * B + b] = nll_pos;
    out[2 * B + b] = nll_neg;
    out[3 * B + b] = num_pos;
    out[4 * B + b] = num_neg;
  }
}
size_t sg_nll_part_doubles(int B, int M) { return 2 * (size_t)std::max(B, 0) * std::max(1, (M + kNllRows - 1) / kNllRows); }

hipError_t sg_nll_loss(const float* la, int B, int M, int N, const uint8_t* gta, const int64_t* gt0, const int64_t* gt1,
                       int mode, float balancing, float* out, double* part, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const int nchunk = std::max(1, (M + kNllRows - 1) / kNllRows);
  // the fp64 partials: the caller's workspace, or (the workspace-less C-ABI entry) a stream-ordered
  // allocation that every path below frees
  double* own = nullptr;
  hipError_t e = hipSuccess;
  if (!part) {
    if ((e = hipMallocAsync(reinterpret_cast<void**>(&own), sizeof(double) * sg_nll_part_doubles(B, M), st)) != hipSuccess)
      return e;
    part = own;
  }
  if (M > 0) {
    hipLaunchKernelGGL(sg_nll_part_kernel, dim3(nchunk, B), dim3(256), 0, st, la, M, N, gta, part);
    e = hipGetLastError();
  } else {
    e = hipMemsetAsync(part, 0, sizeof(double) * 2 * B * nchunk, st);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(sg_nll_kernel, dim3(B), dim3(256), 0, st, la, M, N, part, nchunk, gt0, gt1, mode, balancing, B, out);
    e = hipGetLastError();
  }
  if (own) {
    const hipError_t f = hipFreeAsync(own, st);
    if (e == hipSuccess) e = f;
  }
  return e;
}


}  // namespace lg
