// Homography ground truth on the device: gt_matches_from_homography (reference
// gluefactory/geometry/gt_generation.py:109-161 over warp_points_torch, geometry/homography.py:161-180)
// without any [B, M, N] intermediate.  Per pair: kp0 [M,2], kp1 [N,2], H [3,3], all fp32.
//
//   gt_project   kp0_1 = warp(kp0, H), kp1_0 = warp(kp1, H^-1); H^-1 is the adjugate over the
//                determinant of the fp32 H in fp64, rounded once to fp32 (a singular H is outside the
//                contract, include/lightglue_mi355x.h)
//   gt_stats     pass 1, both directions in one launch: per row (min_j dist, first argmin_j dist,
//                min_j dist0), per column (min_i dist, first argmin_i dist, min_i dist1).  64 owned
//                points per workgroup, one per lane; the other side is staged in LDS in chunks of
//                kChunk points (raw and projected coordinates, 16 B each) and every wave scans its
//                quarter of each chunk, so a single pair still uses four waves per 64 points.  All lanes
//                read the same LDS address (a broadcast, no bank conflicts).  No atomics: the four
//                partials merge in a fixed order, equal minima keep the lowest index.
//   gt_fill0     zeros of the uint8 assignment, 16-byte stores over the flat [B*M*N] buffer
//   gt_finalize  matches0/1, matching_scores0/1 and the (at most one per row) ones of the assignment
//   gt_reward    (dist < pos_th^2) - (dist > neg_th^2) with dist recomputed by the same expression,
//                16-byte stores over each pair's flat [M*N] block behind a scalar head up to the
//                first 16-byte boundary (odd N, unaligned pair bases)
//
// This TU is built with -ffp-contract=off (Makefile): every subtraction, product and sum of a distance
// is rounded on its own, as the reference's separate torch passes do, and pass 1 and the write pass
// get the same bits for the same (i, j).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace lg {
namespace {

constexpr int kOwn = 64;      // owned points per workgroup (one per lane)
constexpr int kWaves = 4;     // waves per workgroup, each scans a quarter of a staged chunk
constexpr int kChunk = 1024;  // staged points per chunk: 16 KiB of LDS

// |a - b|^2 as torch.sum((a - b) ** 2, -1): four roundings.  (a - b) and (b - a) differ by sign only,
// so the value does not depend on the operand order.
__device__ __forceinline__ float sqd(float ax, float ay, float bx, float by) {
  const float dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy;
}

// dist(i, j) and its two halves from point i of image 0 (raw a, projected pa = kp0_1[i]) and point j
// of image 1 (raw b, projected pb = kp1_0[j]): dist0 = |pa - b|^2, dist1 = |a - pb|^2 (:124-126)
struct Dist {
  float d0, d1, d;
};
__device__ __forceinline__ Dist pair_dist(float ax, float ay, float pax, float pay, float bx, float by, float pbx,
                                          float pby) {
  Dist r;
  r.d0 = sqd(pax, pay, bx, by);
  r.d1 = sqd(ax, ay, pbx, pby);
  r.d = fmaxf(r.d0, r.d1);
  return r;
}

// from_homogeneous(points @ H^T, eps=1e-5) (homography.py:176-179, utils.py:30)
__device__ __forceinline__ float2 warp(const float* h, float x, float y) {
  const float u = (h[0] * x + h[1] * y) + h[2];
  const float v = (h[3] * x + h[4] * y) + h[5];
  const float w = ((h[6] * x + h[7] * y) + h[8]) + 1e-5f;
  return make_float2(u / w, v / w);
}

__global__ __launch_bounds__(256) void gt_project(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                  const float* __restrict__ H, int M, int N, int bpp,
                                                  float* __restrict__ p01, float* __restrict__ p10) {
  const int b = blockIdx.x / bpp;
  const int t = (blockIdx.x - b * bpp) * 256 + threadIdx.x;
  float h[9], hi[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = H[(size_t)b * 9 + k];
  {
    const double a = h[0], bb = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7], i = h[8];
    const double A = e * i - f * hh, Bc = -(d * i - f * g), C = d * hh - e * g;
    const double inv = 1.0 / (a * A + bb * Bc + c * C);
    hi[0] = (float)(A * inv);
    hi[1] = (float)(-(bb * i - c * hh) * inv);
    hi[2] = (float)((bb * f - c * e) * inv);
    hi[3] = (float)(Bc * inv);
    hi[4] = (float)((a * i - c * g) * inv);
    hi[5] = (float)(-(a * f - c * d) * inv);
    hi[6] = (float)(C * inv);
    hi[7] = (float)(-(a * hh - bb * g) * inv);
    hi[8] = (float)((a * e - bb * d) * inv);
  }
  if (t < M) {
    const size_t o = ((size_t)b * M + t) * 2;
    const float2 r = warp(h, kp0[o], kp0[o + 1]);
    p01[o] = r.x;
    p01[o + 1] = r.y;
  }
  if (t < N) {
    const size_t o = ((size_t)b * N + t) * 2;
    const float2 r = warp(hi, kp1[o], kp1[o + 1]);
    p10[o] = r.x;
    p10[o + 1] = r.y;
  }
}

// Pass 1.  Blocks [0, B * bm) own rows (points of image 0, scanning image 1), the rest own columns.
// With u = |proj(own) - raw(other)|^2 and v = |raw(own) - proj(other)|^2: a row has dist0 = u,
// dist1 = v; a column has dist1 = u, dist0 = v (sqd is symmetric).  Either way dist = max(u, v) and the
// third statistic is min u, so one body serves both directions.
__global__ __launch_bounds__(kOwn* kWaves) void gt_stats(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                         const float* __restrict__ p01, const float* __restrict__ p10,
                                                         int B, int M, int N, int bm, int bn,
                                                         float* __restrict__ rmin, int* __restrict__ rarg,
                                                         float* __restrict__ rmin0, float* __restrict__ cmin,
                                                         int* __restrict__ carg, float* __restrict__ cmin1) {
  __shared__ float4 stage[kChunk];
  __shared__ float pmin[kWaves][kOwn];
  __shared__ float pthird[kWaves][kOwn];
  __shared__ int parg[kWaves][kOwn];

  int blk = blockIdx.x;
  const bool cols = blk >= B * bm;
  if (cols) blk -= B * bm;
  const int per = cols ? bn : bm;
  const int b = blk / per;
  const int P = cols ? N : M, Q = cols ? M : N;  // owned side, scanned side
  const float* own_raw = (cols ? kp1 : kp0) + (size_t)b * P * 2;
  const float* own_prj = (cols ? p10 : p01) + (size_t)b * P * 2;
  const float* oth_raw = (cols ? kp0 : kp1) + (size_t)b * Q * 2;
  const float* oth_prj = (cols ? p01 : p10) + (size_t)b * Q * 2;

  const int lane = threadIdx.x & (kOwn - 1), wave = threadIdx.x / kOwn;
  const int p = (blk - b * per) * kOwn + lane;
  const bool live = p < P;
  float ox = 0.f, oy = 0.f, opx = 0.f, opy = 0.f;
  if (live) {
    const float2 r = reinterpret_cast<const float2*>(own_raw)[p], q = reinterpret_cast<const float2*>(own_prj)[p];
    ox = r.x;
    oy = r.y;
    opx = q.x;
    opy = q.y;
  }
  float best = __builtin_inff(), third = __builtin_inff();
  int arg = 0;
  constexpr int kQuarter = kChunk / kWaves;
  for (int q0 = 0; q0 < Q; q0 += kChunk) {
    const int cnt = min(kChunk, Q - q0);
    __syncthreads();  // the previous chunk is fully read
    for (int t = threadIdx.x; t < cnt; t += kOwn * kWaves) {
      const int q = q0 + t;
      const float2 r = reinterpret_cast<const float2*>(oth_raw)[q], pr = reinterpret_cast<const float2*>(oth_prj)[q];
      stage[t] = make_float4(r.x, r.y, pr.x, pr.y);
    }
    __syncthreads();
    const int t1 = min(cnt, (wave + 1) * kQuarter);
#pragma unroll 4
    for (int t = wave * kQuarter; t < t1; ++t) {  // ascending, strict <: the first minimum stays
      const float4 s = stage[t];
      const float u = sqd(opx, opy, s.x, s.y);
      const float v = sqd(ox, oy, s.z, s.w);
      const float d = fmaxf(u, v);
      if (d < best) {
        best = d;
        arg = q0 + t;
      }
      third = fminf(third, u);
    }
  }
  pmin[wave][lane] = best;
  parg[wave][lane] = arg;
  pthird[wave][lane] = third;
  __syncthreads();
  if (wave == 0 && live) {
    // a wave's indices ascend within a chunk but interleave with the other waves' across chunks:
    // equal minima resolve to the lowest index explicitly
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      const float m = pmin[w][lane];
      const int a = parg[w][lane];
      if (m < best || (m == best && a < arg)) {
        best = m;
        arg = a;
      }
      third = fminf(third, pthird[w][lane]);
    }
    const size_t o = (size_t)b * P + p;
    (cols ? cmin : rmin)[o] = best;
    (cols ? carg : rarg)[o] = arg;
    (cols ? cmin1 : rmin0)[o] = third;
  }
}

// Zeros over n bytes: a scalar head up to the first 16-byte boundary, uint4 stores, a scalar tail.
__global__ __launch_bounds__(256) void gt_fill0(uint8_t* __restrict__ dst, size_t n) {
  const size_t head = min(n, (size_t)((16 - ((uintptr_t)dst & 15)) & 15));
  const size_t nvec = (n - head) / 16;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  uint4* v = reinterpret_cast<uint4*>(dst + head);
  for (size_t k = tid; k < nvec; k += stride) v[k] = make_uint4(0, 0, 0, 0);
  if (tid < head) dst[tid] = 0;
  const size_t tail0 = head + nvec * 16;
  if (tail0 + tid < n) dst[tail0 + tid] = 0;  // fewer than 16 bytes
}

// matches / scores of both sides (:139-158) and the ones of `positive` (:137).  positive[i, j] needs
// j = argmin_row[i], argmin_col[j] = i and dist(i, j) < pos2, and dist(i, argmin_row[i]) is rmin[i].
__global__ __launch_bounds__(256) void gt_finalize(const float* __restrict__ rmin, const int* __restrict__ rarg,
                                                   const float* __restrict__ rmin0, const float* __restrict__ cmin,
                                                   const int* __restrict__ carg, const float* __restrict__ cmin1, int B,
                                                   int M, int N, float pos2, float neg2, uint8_t* __restrict__ assignment,
                                                   int64_t* __restrict__ m0, int64_t* __restrict__ m1,
                                                   float* __restrict__ s0, float* __restrict__ s1) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t nr = (size_t)B * M, nc = (size_t)B * N;
  if (t < nr) {
    const size_t b = t / M;
    const int i = (int)(t - b * M), j = rarg[t];
    const bool pos = carg[b * N + j] == i && rmin[t] < pos2;
    int64_t m = pos ? (int64_t)j : -2;
    if (rmin0[t] > neg2) m = -1;
    m0[t] = m;
    s0[t] = m > -1 ? 1.f : 0.f;
    if (pos) assignment[(b * M + i) * N + j] = 1;
  } else if (t < nr + nc) {
    const size_t c = t - nr, b = c / N;
    const int j = (int)(c - b * N), i = carg[c];
    const bool pos = rarg[b * M + i] == j && cmin[c] < pos2;
    int64_t m = pos ? (int64_t)i : -2;
    if (cmin1[c] > neg2) m = -1;
    m1[c] = m;
    s1[c] = m > -1 ? 1.f : 0.f;
  }
}

// reward (:128).  Pair b's block is a flat run of MN floats; thread g owns the four entries from
// head + 4 g, where head is the distance to the first 16-byte boundary, and thread 0 also writes the head.
__global__ __launch_bounds__(256) void gt_reward(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                 const float* __restrict__ p01, const float* __restrict__ p10, int M, int N,
                                                 unsigned bpp, float pos2, float neg2, float* __restrict__ reward) {
  const unsigned b = blockIdx.x / bpp;
  const unsigned g = (blockIdx.x - b * bpp) * 256u + threadIdx.x;
  const unsigned MN = (unsigned)M * (unsigned)N;
  float* out = reward + (size_t)b * MN;
  const float* a = kp0 + (size_t)b * M * 2;
  const float* pa = p01 + (size_t)b * M * 2;
  const float* bq = kp1 + (size_t)b * N * 2;
  const float* pb = p10 + (size_t)b * N * 2;
  // keypoints as 8-byte loads (the API checks the alignment); the row's point is reloaded only
  // where the flat run wraps into the next row
  const float2* a2 = reinterpret_cast<const float2*>(a);
  const float2* pa2 = reinterpret_cast<const float2*>(pa);
  const float2* b2 = reinterpret_cast<const float2*>(bq);
  const float2* pb2 = reinterpret_cast<const float2*>(pb);
  auto value = [&](float2 ra, float2 rpa, unsigned j) {
    const float2 cb = b2[j], cpb = pb2[j];
    const float d = pair_dist(ra.x, ra.y, rpa.x, rpa.y, cb.x, cb.y, cpb.x, cpb.y).d;
    return (d < pos2 ? 1.f : 0.f) - (d > neg2 ? 1.f : 0.f);
  };
  const unsigned head = min(MN, (unsigned)(((16 - ((uintptr_t)out & 15)) & 15) >> 2));
  if (g == 0)
    for (unsigned r = 0; r < head; ++r) out[r] = value(a2[r / N], pa2[r / N], r % N);
  const unsigned long long r0 = head + 4ull * g;
  if (r0 >= MN) return;
  unsigned i = (unsigned)r0 / (unsigned)N, j = (unsigned)r0 - i * (unsigned)N;
  const unsigned left = MN - (unsigned)r0;
  float2 ra = a2[i], rpa = pa2[i];
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if ((unsigned)k < left) {
      v[k] = value(ra, rpa, j);
      if (++j == (unsigned)N) {
        j = 0;
        if (++i < (unsigned)M) {
          ra = a2[i];
          rpa = pa2[i];
        }
      }
    }
  }
  if (left >= 4) {
    *reinterpret_cast<float4*>(out + r0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (unsigned k = 0; k < left; ++k) out[r0 + k] = v[k];
  }
}

size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

size_t gt_homography_workspace_bytes(int B, int M, int N) {
  // per row: min dist, argmin, min dist0; per column: min dist, argmin, min dist1
  return 3 * up256((size_t)B * M * 4) + 3 * up256((size_t)B * N * 4);
}

hipError_t gt_matches_from_homography(const float* kp0, const float* kp1, const float* H, int B, int M, int N, float pos2,
                                      float neg2, uint8_t* assignment, float* reward, int64_t* m0, int64_t* m1, float* s0,
                                      float* s1, float* p01, float* p10, void* workspace, hipStream_t st) {
  char* w = static_cast<char*>(workspace);
  const size_t rb = up256((size_t)B * M * 4), cb = up256((size_t)B * N * 4);
  float* rmin = reinterpret_cast<float*>(w);
  int* rarg = reinterpret_cast<int*>(w + rb);
  float* rmin0 = reinterpret_cast<float*>(w + 2 * rb);
  float* cmin = reinterpret_cast<float*>(w + 3 * rb);
  int* carg = reinterpret_cast<int*>(w + 3 * rb + cb);
  float* cmin1 = reinterpret_cast<float*>(w + 3 * rb + 2 * cb);

  const int bpp = (max(M, N) + 255) / 256;
  gt_project<<<dim3((unsigned)B * bpp), dim3(256), 0, st>>>(kp0, kp1, H, M, N, bpp, p01, p10);
  const int bm = (M + kOwn - 1) / kOwn, bn = (N + kOwn - 1) / kOwn;
  gt_stats<<<dim3((unsigned)B * (bm + bn)), dim3(kOwn * kWaves), 0, st>>>(kp0, kp1, p01, p10, B, M, N, bm, bn, rmin, rarg,
                                                                         rmin0, cmin, carg, cmin1);
  const size_t nbytes = (size_t)B * M * N;
  const size_t fill_blocks = (nbytes / 16 + 255) / 256 + 1;
  gt_fill0<<<dim3((unsigned)(fill_blocks < 65536 ? fill_blocks : 65536)), dim3(256), 0, st>>>(assignment, nbytes);
  const size_t nfin = (size_t)B * M + (size_t)B * N;
  gt_finalize<<<dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, st>>>(rmin, rarg, rmin0, cmin, carg, cmin1, B, M, N, pos2,
                                                                        neg2, assignment, m0, m1, s0, s1);
  if (reward) {
    const unsigned rpp = (unsigned)(((size_t)M * N / 4 + 1 + 255) / 256);
    gt_reward<<<dim3((unsigned)B * rpp), dim3(256), 0, st>>>(kp0, kp1, p01, p10, M, N, rpp, pos2, neg2, reward);
  }
  return hipGetLastError();
}

}  // namespace lg
