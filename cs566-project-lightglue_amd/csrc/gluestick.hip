// GlueStick pieces that are not shared with SuperGlue (gluefactory/models/matchers/gluestick.py):
//   the line layer's gather and per-junction mean (LineLayer, :582-684), log_double_softmax
//   (:761-772) and the line head's orientation maximum (:351-357).  The endpoint encoder is the
//   keypoint encoder kernel in its `endpoints` mode (superglue.hip); the GEMMs are the shared fp16x3 /
//   bf16x6 ones (gluestick_api.cpp).
// Rows of the residual stream: image 0 of pair b at b*M, image 1 at B*M + b*N.  Endpoints likewise:
// image 0 of pair b at b*E0, image 1 at B*E0 + b*E1 (E = 2 L; endpoint e and e ^ 1 share a line).
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace lg {

namespace {

__device__ inline void gs_locate(const GsLayout& g, int e, int& row_base, int& n) {
  if (e < g.B * g.E0) {
    row_base = (e / g.E0) * g.M;
    n = g.M;
  } else {
    row_base = g.B * g.M + ((e - g.B * g.E0) / g.E1) * g.N;
    n = g.N;
  }
}

__global__ void gs_clamp_idx_kernel(const int64_t* idx64, size_t count, int n, int* idx32) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t v = idx64[e];
  idx32[e] = v < 0 ? 0 : (v >= n ? n - 1 : (int)v);
}

// One workgroup per image of a pair: degree count (integer atomics: the counts do not depend on
// their order), exclusive scan, then a stable fill -- chunks of 256 endpoints in order, each
// thread ranked among the earlier threads of its chunk with the same junction -- so list[] holds
// every junction's endpoints in endpoint order whatever the scheduling.
__global__ __launch_bounds__(256) void gs_csr_kernel(const int* idx32, GsLayout g, int* deg, int* start, int* cursor,
                                                     int* list) {
  __shared__ int part[256];
  __shared__ int keys[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const bool im1 = s >= g.B;
  const int n = im1 ? g.N : g.M, ne = im1 ? g.E1 : g.E0;
  const int rb = im1 ? g.B * g.M + (s - g.B) * g.N : s * g.M;
  const int eb = im1 ? g.B * g.E0 + (s - g.B) * g.E1 : s * g.E0;
  for (int r = tid; r < n; r += 256) deg[rb + r] = 0;
  __syncthreads();
  for (int e = tid; e < ne; e += 256) atomicAdd(&deg[rb + idx32[eb + e]], 1);
  __syncthreads();
  const int chunk = (n + 255) / 256;
  const int r0 = min(n, tid * chunk), r1 = min(n, r0 + chunk);
  int sum = 0;
  for (int r = r0; r < r1; ++r) sum += deg[rb + r];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = part[t];
      part[t] = run;
      run += v;
    }
  }
  __syncthreads();
  int run = eb + part[tid];
  for (int r = r0; r < r1; ++r) {
    start[rb + r] = run;
    cursor[rb + r] = run;
    run += deg[rb + r];
  }
  __syncthreads();
  for (int c0 = 0; c0 < ne; c0 += 256) {
    const int e = c0 + tid;
    const bool on = e < ne;
    const int key = on ? idx32[eb + e] : -1;
    keys[tid] = key;
    __syncthreads();
    int rank = 0;
    bool last = true;
    if (on) {
      for (int t = 0; t < tid; ++t) rank += keys[t] == key;
      for (int t = tid + 1; t < 256; ++t) last = last && keys[t] != key;
    }
    const int base = on ? cursor[rb + key] : 0;
    __syncthreads();
    if (on) {
      list[base + rank] = eb + e;
      if (last) cursor[rb + key] = base + rank + 1;
    }
    __syncthreads();
  }
}

// G[e] = [x[j(e)] | x[j(e ^ 1)] | enc[e]]: 192 threads, one float4 each
__global__ __launch_bounds__(192) void gs_gather_ep_kernel(const float* X, const float* enc, const int* idx32, GsLayout g,
                                                           float* G) {
  const int e = blockIdx.x, t = threadIdx.x;
  int rb, n;
  gs_locate(g, e, rb, n);
  const int seg = t >> 6, c = (t & 63) * 4;
  const float* src = seg == 2 ? enc + (size_t)e * 256 : X + (size_t)(rb + idx32[seg == 0 ? e : (e ^ 1)]) * 256;
  *reinterpret_cast<f32x4*>(G + (size_t)e * 768 + seg * 256 + c) = *reinterpret_cast<const f32x4*>(src + c);
}

// one wave per junction row: the mean of its endpoints' rows of U in list order, added to x
__global__ __launch_bounds__(256) void gs_scatter_mean_kernel(float* X, int R, const float* U, const int* deg,
                                                              const int* start, const int* list) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const int d = deg[r];
  if (d == 0) return;
  const int s0 = start[r];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < d; ++k) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(U + (size_t)list[s0 + k] * 256 + lane * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += u[i];
  }
  f32x4* xp = reinterpret_cast<f32x4*>(X + (size_t)r * 256 + lane * 4);
  f32x4 x = *xp;
  const float cnt = (float)d;
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] += acc[i] / cnt;
  *xp = x;
}

__global__ __launch_bounds__(64) void gs_gather_rows_kernel(const float* src, int ld, int n, const int64_t* idx, int ne,
                                                            float* dst) {
  const int e = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  int64_t j = idx[(size_t)b * ne + e];
  j = j < 0 ? 0 : (j >= n ? n - 1 : j);
  *reinterpret_cast<f32x4*>(dst + ((size_t)b * ne + e) * 256 + lane * 4) =
      *reinterpret_cast<const f32x4*>(src + ((size_t)b * n + j) * ld + lane * 4);
}

__device__ inline float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ inline float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// log-softmax statistics of [row, bin]: one wave per row; rmax / rlog [B*M]
__global__ __launch_bounds__(256) void gs_row_stats_kernel(const float* S, float bin, int rows, int N, float* rmax,
                                                           float* rlog) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* p = S + (size_t)r * N;
  float m = bin;
  for (int j = lane; j < N; j += 64) m = fmaxf(m, p[j]);
  m = wave_max(m);
  float s = 0.f;
  for (int j = lane; j < N; j += 64) s += expf(p[j] - m);
  s = wave_sum(s) + expf(bin - m);
  if (lane == 0) {
    rmax[r] = m;
    rlog[r] = logf(s);
  }
}

// the same down the columns: 64 columns x 4 row slices per workgroup; cmax / clog [B*N]
__global__ __launch_bounds__(256) void gs_col_stats_kernel(const float* S, float bin, int M, int N, float* cmax,
                                                           float* clog) {
  __shared__ float red[4][64];
  const int b = blockIdx.y, c = threadIdx.x & 63, gidx = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  const float* p = S + (size_t)b * M * N;
  float m = bin;
  if (j < N)
    for (int i = gidx; i < M; i += 4) m = fmaxf(m, p[(size_t)i * N + j]);
  red[gidx][c] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0][c], red[1][c]), fmaxf(red[2][c], red[3][c]));
  __syncthreads();
  float s = 0.f;
  if (j < N)
    for (int i = gidx; i < M; i += 4) s += expf(p[(size_t)i * N + j] - m);
  red[gidx][c] = s;
  __syncthreads();
  if (gidx == 0 && j < N) {
    s = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) + expf(bin - m);
    cmax[(size_t)b * N + j] = m;
    clog[(size_t)b * N + j] = logf(s);
  }
}

// out [B][M+1][N+1]: interior half the sum of the two log-softmaxes, last column the row's bin
// term, last row the column's, corner 0
__global__ __launch_bounds__(256) void gs_dsm_write_kernel(const float* S, float bin, int M, int N, const float* rmax,
                                                           const float* rlog, const float* cmax, const float* clog,
                                                           float* out) {
  const int i = blockIdx.x, b = blockIdx.y;
  float* o = out + ((size_t)b * (M + 1) + i) * (N + 1);
  if (i == M) {
    for (int j = threadIdx.x; j <= N; j += 256)
      o[j] = j == N ? 0.f : (bin - cmax[(size_t)b * N + j]) - clog[(size_t)b * N + j];
    return;
  }
  const float* p = S + ((size_t)b * M + i) * N;
  const float rm = rmax[(size_t)b * M + i], rl = rlog[(size_t)b * M + i];
  for (int j = threadIdx.x; j <= N; j += 256) {
    if (j == N) {
      o[j] = (bin - rm) - rl;
    } else {
      const float s = p[j];
      const float a0 = (s - rm) - rl;
      const float a1 = (s - cmax[(size_t)b * N + j]) - clog[(size_t)b * N + j];
      o[j] = (a0 + a1) / 2.f;
    }
  }
}

__global__ __launch_bounds__(256) void gs_line_combine_kernel(const float* S, int L0, int L1, float* raw) {
  const int i = blockIdx.x, b = blockIdx.y;
  const float* r0 = S + ((size_t)b * 2 * L0 + 2 * i) * (2 * L1);
  const float* r1 = r0 + 2 * L1;
  float* o = raw + ((size_t)b * L0 + i) * L1;
  for (int j = threadIdx.x; j < L1; j += 256) {
    const float s00 = r0[2 * j], s01 = r0[2 * j + 1], s10 = r1[2 * j], s11 = r1[2 * j + 1];
    o[j] = 0.5f * fmaxf(s00 + s11, s01 + s10);
  }
}

}  // namespace

hipError_t gs_clamp_idx(const int64_t* idx64, size_t count, int n, int* idx32, hipStream_t st) {
  if (count == 0) return hipSuccess;
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gs_clamp_idx_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, idx64, count, n, idx32);
  return hipGetLastError();
}

hipError_t gs_build_csr(const int* idx32, const GsLayout& g, int* deg, int* start, int* cursor, int* list,
                        hipStream_t st) {
  if (g.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(gs_csr_kernel, dim3(2 * g.B), dim3(256), 0, st, idx32, g, deg, start, cursor, list);
  return hipGetLastError();
}

hipError_t gs_gather_endpoints(const float* X, const float* enc, const int* idx32, const GsLayout& g, float* G,
                               hipStream_t st) {
  const int total = g.B * (g.E0 + g.E1);
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(gs_gather_ep_kernel, dim3(total), dim3(192), 0, st, X, enc, idx32, g, G);
  return hipGetLastError();
}

hipError_t gs_scatter_mean(float* X, int R, const float* U, const int* deg, const int* start, const int* list,
                           hipStream_t st) {
  if (R <= 0) return hipSuccess;
  hipLaunchKernelGGL(gs_scatter_mean_kernel, dim3((R + 3) / 4), dim3(256), 0, st, X, R, U, deg, start, list);
  return hipGetLastError();
}

hipError_t gs_gather_rows256(const float* src, int ld, int n, const int64_t* idx, int B, int ne, float* dst,
                             hipStream_t st) {
  if (B <= 0 || ne <= 0) return hipSuccess;
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gs_gather_rows_kernel, dim3(ne, B), dim3(64), 0, st, src, ld, n, idx, ne, dst);
  return hipGetLastError();
}

hipError_t gs_double_softmax(const float* scores, float bin, int B, int M, int N, float* out, float* ws, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (M <= 0 || N <= 0) return hipErrorInvalidValue;
  float *rmax = ws, *rlog = ws + (size_t)B * M, *cmax = ws + 2 * (size_t)B * M, *clog = cmax + (size_t)B * N;
  hipLaunchKernelGGL(gs_row_stats_kernel, dim3((B * M + 3) / 4), dim3(256), 0, st, scores, bin, B * M, N, rmax, rlog);
  hipLaunchKernelGGL(gs_col_stats_kernel, dim3((N + 63) / 64, B), dim3(256), 0, st, scores, bin, M, N, cmax, clog);
  hipLaunchKernelGGL(gs_dsm_write_kernel, dim3(M + 1, B), dim3(256), 0, st, scores, bin, M, N, rmax, rlog, cmax, clog, out);
  return hipGetLastError();
}

hipError_t gs_line_combine(const float* S, int B, int L0, int L1, float* raw, hipStream_t st) {
  if (B <= 0 || L0 <= 0 || L1 <= 0) return hipSuccess;
  hipLaunchKernelGGL(gs_line_combine_kernel, dim3(L0, B), dim3(256), 0, st, S, L0, L1, raw);
  return hipGetLastError();
}

}  // namespace lg
