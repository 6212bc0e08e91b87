// The wireframe step in front of GlueStick (gluefactory/models/lines/wireframe.py).
//
//   wf_cluster_kernel     one workgroup per image: DBSCAN(eps, min_samples = 1) of the 2 L line endpoints
//                         = connected components of "distance <= eps", numbered by lowest member;
//                         junction means and scores, the rewritten lines, lines_junc_idx, the fill slots
//   wf_merge_points_kernel one workgroup per image: keypoints on an endpoint are replaced in place
//                         (forced) or dropped by a stable compaction (free)
//   wf_descriptor_kernel  one wave per output row: bilinear sample of the NHWC dense map + L2 norm, or
//                         a copy of the point extractor's row
//   wf_eye_kernel / wf_pairs_kernel  the bool connectivity matrices
//
// Built with -ffp-contract=off: the two distance tests decide set membership, so every operation
// rounds on its own.  No float atomics: sums run in ascending endpoint order in one thread, the only
// atomics are integer atomicMin on labels whose fixpoint does not depend on the order of updates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace lg {
namespace {

constexpr int kWfThreads = 1024;
constexpr int kWfWaves = kWfThreads / 64;

// Exclusive count of `flag` over the threads before this one in the block; total: over the block.
// Every thread of the block calls it (it synchronises).
__device__ inline int block_count_before(bool flag, int* wave_tot, int& total) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();  // the previous call's readers are done with wave_tot
  if (lane == 0) wave_tot[w] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
  for (int i = 0; i < kWfWaves; ++i) {
    const int c = wave_tot[i];
    base += i < w ? c : 0;
    tot += c;
  }
  total = tot;
  return base + before;
}

struct ClusterArgs {
  const float2* ep;         // [B][E]
  const float* line_scores; // [B][L]
  const float2* fill;       // [B][J] or null
  int E, J, N, merge, forced;
  double eps2;
  float2* points;  // [B][N]
  float* scores;   // [B][N]
  float2* new_ep;  // [B][E]
  int64_t* idx;    // [B][E]
  int* counts;     // [B]
};

__global__ __launch_bounds__(kWfThreads) void wf_cluster_kernel(ClusterArgs a) {
  __shared__ float2 xy[kWfMaxEndpoints];
  __shared__ int par[kWfMaxEndpoints];
  __shared__ unsigned short rnk[kWfMaxEndpoints];
  __shared__ int wave_tot[kWfWaves];
  __shared__ int changed;
  const int b = blockIdx.x, t = threadIdx.x, E = a.E;
  const float2* ep = a.ep + (size_t)b * E;
  for (int i = t; i < E; i += kWfThreads) {
    xy[i] = ep[i];
    par[i] = i;
  }
  __syncthreads();
  if (a.merge) {
    // par[i] always names a member of i's component with par[i] <= i.  A sweep hooks i (and the
    // member it pointed at) under the smallest par of its neighbours, then every i jumps to its
    // root.  The loop ends only after a sweep that changed nothing: then par is constant on each
    // component and equal to its lowest index, whatever order the updates happened in.
    for (;;) {
      if (t == 0) changed = 0;
      __syncthreads();
      for (int i = t; i < E; i += kWfThreads) {
        const double xi = xy[i].x, yi = xy[i].y;
        const int mine = par[i];
        int m = mine;
        for (int j = 0; j < E; ++j) {
          const float2 q = xy[j];
          const double dx = xi - (double)q.x, dy = yi - (double)q.y;
          if (dx * dx + dy * dy <= a.eps2) m = min(m, par[j]);
        }
        if (m < mine) {
          atomicMin(&par[mine], m);
          atomicMin(&par[i], m);
          changed = 1;
        }
      }
      __syncthreads();
      const int again = changed;
      for (int i = t; i < E; i += kWfThreads) {
        int p = par[i];
        for (int q = par[p]; q != p; q = par[p]) p = q;  // strictly decreasing: ends at a root
        par[i] = p;
      }
      __syncthreads();
      if (!again) break;
    }
  }
  // rank of every root among the roots = sklearn's label of its component
  int n_true = 0;
  for (int i0 = 0; i0 < E; i0 += kWfThreads) {
    const int i = i0 + t;
    const bool root = i < E && par[i] == i;
    int tot;
    const int r = block_count_before(root, wave_tot, tot);
    if (root) rnk[i] = (unsigned short)(n_true + r);
    n_true += tot;
  }
  __syncthreads();
  // means: fp32 sums in ascending endpoint order, one division (scatter_reduce_ "mean" on the CPU)
  const float* ls = a.line_scores + (size_t)b * (E / 2);
  for (int i = t; i < E; i += kWfThreads) {
    if (par[i] != i) continue;
    float sx = 0.f, sy = 0.f, ss = 0.f;
    int c = 0;
    const int jend = a.merge ? E : i + 1;
    for (int j = i; j < jend; ++j) {
      if (par[j] != i) continue;
      const float2 q = xy[j];
      sx += q.x, sy += q.y, ss += ls[j >> 1];
      ++c;
    }
    const float n = (float)c;
    const float2 mean = make_float2(sx / n, sy / n);
    xy[i] = mean;  // only this root's own scan read xy[i]
    const size_t row = (size_t)b * a.N + rnk[i];
    a.points[row] = mean;
    a.scores[row] = ss / n;
  }
  __syncthreads();
  for (int i = t; i < E; i += kWfThreads) {
    const int r = par[i];
    a.new_ep[(size_t)b * E + i] = xy[r];
    a.idx[(size_t)b * E + i] = rnk[r];
  }
  if (a.forced && a.fill) {
    for (int j = n_true + t; j < a.J; j += kWfThreads) {
      const size_t row = (size_t)b * a.N + j;
      a.points[row] = a.fill[(size_t)b * a.J + (j - n_true)];
      a.scores[row] = 0.f;
    }
  }
  if (t == 0) a.counts[b] = n_true;
}

struct MergeArgs {
  const float2* ep;   // [B][E] endpoints of the original lines
  const float2* kp;   // [B][K]
  const float* kps;   // [B][K]
  const float2* fill; // [B][K] or null
  int E, K, J, N, merge, forced;
  float r;
  float2* points;
  float* scores;
  int* src;      // [B][K]: keypoint slot -> source row; -1 sample at the slot's position; -2 unused
  int* counts;   // [B] keypoints kept
  uint8_t* removed;  // [B][K] or null
};

__global__ __launch_bounds__(kWfThreads) void wf_merge_points_kernel(MergeArgs a) {
  __shared__ float2 xy[kWfMaxEndpoints];
  __shared__ int wave_tot[kWfWaves];
  const int b = blockIdx.x, t = threadIdx.x, E = a.merge ? a.E : 0, K = a.K;
  for (int i = t; i < E; i += kWfThreads) xy[i] = a.ep[(size_t)b * a.E + i];
  __syncthreads();
  int kept = 0;
  for (int k0 = 0; k0 < K; k0 += kWfThreads) {
    const int k = k0 + t;
    const bool in = k < K;
    bool rem = false;
    float2 p = make_float2(0.f, 0.f);
    float sc = 0.f;
    if (in) {
      p = a.kp[(size_t)b * K + k];
      sc = a.kps[(size_t)b * K + k];
      for (int j = 0; j < E; ++j) {  // torch.norm(kp - ep) < r, strict, fp32
        const float dx = p.x - xy[j].x, dy = p.y - xy[j].y;
        rem |= sqrtf(dx * dx + dy * dy) < a.r;
      }
      if (a.removed) a.removed[(size_t)b * K + k] = rem ? 1 : 0;
    }
    if (a.forced) {
      if (in) {
        const size_t row = (size_t)b * a.N + a.J + k;
        a.points[row] = rem ? a.fill[(size_t)b * K + k] : p;
        a.scores[row] = rem ? 0.f : sc;
        a.src[(size_t)b * K + k] = rem ? -1 : k;
      }
      kept += min(kWfThreads, K - k0);
    } else {
      int tot;
      const int pos = kept + block_count_before(in && !rem, wave_tot, tot);
      if (in && !rem) {  // pos <= k: stable, in place of nothing that is still to be read
        const size_t row = (size_t)b * a.N + a.J + pos;
        a.points[row] = p;
        a.scores[row] = sc;
        a.src[(size_t)b * K + pos] = k;
      }
      kept += tot;
    }
  }
  if (!a.forced)
    for (int k = kept + t; k < K; k += kWfThreads) a.src[(size_t)b * K + k] = -2;
  if (t == 0) a.counts[b] = kept;
}

// One wave: the dense map [Hc][Wc][D] of one image sampled at pixel p, L2-normalised, to out[D].
__device__ inline void sample_row(const float* __restrict__ dense, int Hc, int Wc, int D, float s, float2 p,
                                  float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const float fx = p.x / s - 0.5f, fy = p.y / s - 0.5f;
  float w[4] = {0.f, 0.f, 0.f, 0.f};
  long long off[4] = {-1, -1, -1, -1};
  if (fx > -1.f && fx < (float)Wc && fy > -1.f && fy < (float)Hc) {  // else (NaN too): all four corners outside
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float x1f = x0f + 1.f, y1f = y0f + 1.f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float wgt[4] = {(x1f - fx) * (y1f - fy), (fx - x0f) * (y1f - fy), (x1f - fx) * (fy - y0f), (fx - x0f) * (fy - y0f)};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = x0 + (q & 1), y = y0 + (q >> 1);
      if (x >= 0 && x < Wc && y >= 0 && y < Hc) {
        off[q] = ((long long)y * Wc + x) * D;
        w[q] = wgt[q];
      }
    }
  }
  float4 v[4];
  float ssq = 0.f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int c = it * 256 + lane * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < D) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (off[q] < 0) continue;
        const float4 g = *reinterpret_cast<const float4*>(dense + off[q] + c);
        acc.x += g.x * w[q], acc.y += g.y * w[q], acc.z += g.z * w[q], acc.w += g.w * w[q];
      }
      ssq += acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w;
    }
    v[it] = acc;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) ssq += __shfl_xor(ssq, m);
  const float den = fmaxf(sqrtf(ssq), 1e-12f);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int c = it * 256 + lane * 4;
    if (c < D)
      *reinterpret_cast<float4*>(out + c) = make_float4(v[it].x / den, v[it].y / den, v[it].z / den, v[it].w / den);
  }
}

struct DescArgs {
  const float* dense;    // [B][Hc][Wc][D]
  const float* kp_desc;  // [B][K][D]
  const float2* points;  // [B][N]
  const int* src;        // [B][K]
  const int* counts;     // [B] true junctions
  int B, J, K, N, D, Hc, Wc, all_junctions;
  float s;
  float* out;  // [B][N][D]
};

__global__ __launch_bounds__(256) void wf_descriptor_kernel(DescArgs a) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)a.B * a.N) return;
  const int b = (int)(row / a.N), r = (int)(row % a.N), lane = threadIdx.x & 63;
  float* out = a.out + (size_t)row * a.D;
  if (r < a.J) {
    if (r >= (a.all_junctions ? a.J : a.counts[b])) return;
  } else {
    const int sidx = a.src[(size_t)b * a.K + (r - a.J)];
    if (sidx == -2) return;
    if (sidx >= 0) {
      if (sidx >= a.K) return;
      const float* from = a.kp_desc + ((size_t)b * a.K + sidx) * a.D;
      for (int c = lane * 4; c < a.D; c += 256) *reinterpret_cast<float4*>(out + c) = *reinterpret_cast<const float4*>(from + c);
      return;
    }
  }
  sample_row(a.dense + (size_t)b * a.Hc * a.Wc * a.D, a.Hc, a.Wc, a.D, a.s, a.points[row], out);
}

__global__ __launch_bounds__(256) void wf_sample_kernel(const float2* points, const float* dense, long long rows, int P,
                                                        int Hc, int Wc, int D, float s, float* out) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  sample_row(dense + (size_t)(row / P) * Hc * Wc * D, Hc, Wc, D, s, points[row], out + (size_t)row * D);
}

// out [B][N][N] bytes = identity; 16 bytes per thread
__global__ __launch_bounds__(256) void wf_eye_kernel(uint8_t* out, long long total, long long NN, int N) {
  const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (g >= total) return;
  long long w = g % NN;
  int r = (int)(w % (N + 1));
  uint32_t word[4] = {0u, 0u, 0u, 0u};
  uint8_t byte[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    byte[t] = r == 0 ? 1 : 0;
    word[t >> 2] |= (uint32_t)byte[t] << (8 * (t & 3));
    ++w, ++r;
    if (r == N + 1) r = 0;
    if (w == NN) w = 0, r = 0;
  }
  if (g + 16 <= total) {
    *reinterpret_cast<uint4*>(out + g) = make_uint4(word[0], word[1], word[2], word[3]);
  } else {
    for (int t = 0; t < 16 && g + t < total; ++t) out[g + t] = byte[t];
  }
}

__global__ __launch_bounds__(256) void wf_pairs_kernel(const int64_t* idx, long long lines, int L, int N, uint8_t* out) {
  const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
  if (l >= lines) return;
  const int64_t i = idx[2 * l], j = idx[2 * l + 1];
  if (i < 0 || i >= N || j < 0 || j >= N) return;
  uint8_t* m = out + (size_t)(l / L) * N * N;
  m[(size_t)i * N + j] = 1;
  m[(size_t)j * N + i] = 1;
}

}  // namespace

size_t wireframe_workspace_bytes(int B, int L, int K) {
  (void)L;
  return (((size_t)B * K * sizeof(int) + 255) & ~(size_t)255) + 256;
}

hipError_t wireframe_connectivity(const int64_t* idx, int B, int L, int N, int identity_only, uint8_t* out,
                                  hipStream_t st) {
  const long long NN = (long long)N * N, total = NN * B;
  if (total == 0) return hipSuccess;
  const long long chunks = (total + 15) / 16;
  hipLaunchKernelGGL(wf_eye_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, out, total, NN, N);
  const long long lines = (long long)B * L;
  if (!identity_only && lines > 0)
    hipLaunchKernelGGL(wf_pairs_kernel, dim3((unsigned)((lines + 255) / 256)), dim3(256), 0, st, idx, lines, L, N, out);
  return hipGetLastError();
}

hipError_t sample_descriptors_corner(const float* points, const float* dense, int B, int P, int Hc, int Wc, int D, int s,
                                     float* out, hipStream_t st) {
  const long long rows = (long long)B * P;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(wf_sample_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const float2*)points, dense,
                     rows, P, Hc, Wc, D, (float)s, out);
  return hipGetLastError();
}

hipError_t wireframe_forward(const WfCall& c, void* workspace, hipStream_t st) {
  if (c.B == 0) return hipSuccess;
  const int E = 2 * c.L, N = c.J + c.K;
  int* src = (int*)workspace;
  ClusterArgs ca;
  ca.ep = (const float2*)c.lines, ca.line_scores = c.line_scores, ca.fill = (const float2*)c.fill_junc;
  ca.E = E, ca.J = c.J, ca.N = N, ca.merge = c.merge_endpoints, ca.forced = c.force_lines && c.merge_endpoints;
  ca.eps2 = c.eps * c.eps;
  ca.points = (float2*)c.points, ca.scores = c.scores, ca.new_ep = (float2*)c.new_lines, ca.idx = c.idx;
  ca.counts = c.counts;
  hipLaunchKernelGGL(wf_cluster_kernel, dim3(c.B), dim3(kWfThreads), 0, st, ca);
  MergeArgs ma;
  ma.ep = (const float2*)c.lines, ma.kp = (const float2*)c.kp, ma.kps = c.kp_scores, ma.fill = (const float2*)c.fill_kp;
  ma.E = E, ma.K = c.K, ma.J = c.J, ma.N = N, ma.merge = c.merge_points;
  ma.forced = c.force_kp || !c.merge_points;  // nothing removed: in place is the compaction
  ma.r = (float)c.eps;
  ma.points = (float2*)c.points, ma.scores = c.scores, ma.src = src, ma.counts = c.counts + c.B, ma.removed = c.removed;
  hipLaunchKernelGGL(wf_merge_points_kernel, dim3(c.B), dim3(kWfThreads), 0, st, ma);
  const long long rows = (long long)c.B * N;
  if (rows > 0) {
    DescArgs da;
    da.dense = c.dense, da.kp_desc = c.kp_desc, da.points = (const float2*)c.points, da.src = src, da.counts = c.counts;
    da.B = c.B, da.J = c.J, da.K = c.K, da.N = N, da.D = c.D, da.Hc = c.Hc, da.Wc = c.Wc;
    da.all_junctions = ca.forced;
    da.s = (float)c.s;
    da.out = c.out_desc;
    hipLaunchKernelGGL(wf_descriptor_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, da);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (c.conn) {
    e = wireframe_connectivity(c.idx, c.B, c.L, c.J, !c.merge_endpoints, c.conn, st);
    if (e != hipSuccess) return e;
  }
  if (c.pl) e = wireframe_connectivity(c.idx, c.B, c.L, N, !c.merge_endpoints, c.pl, st);
  return e;
}

}  // namespace lg
