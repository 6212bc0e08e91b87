// What the two ground-truth translation units share (gt_match.hip: homography pairs, gt_depth.hip:
// posed pairs with depth): the zero fill of the assignment, the 64-points-per-workgroup LDS-staged scan
// that keeps per-row and per-column statistics without an [M, N] intermediate, the finalize that turns
// those statistics into matches / scores / the ones of the assignment, and the flat [M*N] writer of
// the reward (16-byte stores behind a scalar head).  A path plugs in through a small `Op` type; the
// arithmetic of a path lives in its Op, so the homography path computes what it computed before this
// header existed, bit for bit.  Both TUs are built with -ffp-contract=off (Makefile).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lg {
namespace gt {

constexpr int kOwn = 64;      // owned points per workgroup (one per lane)
constexpr int kWaves = 4;     // waves per workgroup, each scans a quarter of a staged chunk
constexpr int kChunk = 1024;  // staged points per chunk: 16 KiB of LDS (+ 1 KiB of flags where an Op has them)

// |a - b|^2 as torch.sum((a - b) ** 2, -1): four roundings.  (a - b) and (b - a) differ by sign only,
// so the value does not depend on the operand order.
__device__ __forceinline__ float sqd(float ax, float ay, float bx, float by) {
  const float dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy;
}

// from_homogeneous(points @ H^T, eps=1e-5) (geometry/homography.py:176-179, utils.py:30)
__device__ __forceinline__ float2 warp(const float* h, float x, float y) {
  const float u = (h[0] * x + h[1] * y) + h[2];
  const float v = (h[3] * x + h[4] * y) + h[5];
  const float w = ((h[6] * x + h[7] * y) + h[8]) + 1e-5f;
  return make_float2(u / w, v / w);
}

// H^-1 as the adjugate over the determinant of the fp32 H in fp64, rounded once to fp32
__device__ __forceinline__ void invert_h(const float* h, float* hi) {
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

inline size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

// Zeros over n bytes: a scalar head up to the first 16-byte boundary, uint4 stores, a scalar tail.
static __global__ __launch_bounds__(256) void gt_fill0(uint8_t* __restrict__ dst, size_t n) {
  const size_t head = min(n, (size_t)((16 - ((uintptr_t)dst & 15)) & 15));
  const size_t nvec = (n - head) / 16;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  uint4* v = reinterpret_cast<uint4*>(dst + head);
  for (size_t k = tid; k < nvec; k += stride) v[k] = make_uint4(0, 0, 0, 0);
  if (tid < head) dst[tid] = 0;
  const size_t tail0 = head + nvec * 16;
  if (tail0 + tid < n) dst[tail0 + tid] = 0;  // fewer than 16 bytes
}

inline void launch_fill0(uint8_t* dst, size_t nbytes, hipStream_t st) {
  const size_t fill_blocks = (nbytes / 16 + 255) / 256 + 1;
  gt_fill0<<<dim3((unsigned)(fill_blocks < 65536 ? fill_blocks : 65536)), dim3(256), 0, st>>>(dst, nbytes);
}

// The scan.  A workgroup of kOwn * kWaves threads owns kOwn points (lane = threadIdx.x % kOwn holds
// `own`); the Q points of the other side are staged in LDS in chunks of kChunk (Op::stage: 16 bytes
// and, with Op::kFlag, one flag byte per point) and every wave scans its quarter of each chunk, so a
// single pair still uses four waves per 64 points.  All lanes read the same LDS address (a broadcast,
// no bank conflicts).  Op::eval gives d (minimised with its first index) and u (minimised alone).  No
// atomics: the four partials merge in a fixed order, equal minima keep the lowest index, an all-inf
// row keeps index 0.  The result is valid in wave 0 (returns true there).  Every thread of the
// workgroup must call it.
template <class Op>
__device__ __forceinline__ bool scan(const Op& op, const typename Op::Own& own, int Q, float& best, int& arg,
                                     float& third) {
  __shared__ float4 stage[kChunk];
  __shared__ uint8_t sflag[Op::kFlag ? kChunk : 1];
  __shared__ float pmin[kWaves][kOwn];
  __shared__ float pthird[kWaves][kOwn];
  __shared__ int parg[kWaves][kOwn];

  const int lane = threadIdx.x & (kOwn - 1), wave = threadIdx.x / kOwn;
  best = __builtin_inff();
  third = __builtin_inff();
  arg = 0;
  constexpr int kQuarter = kChunk / kWaves;
  for (int q0 = 0; q0 < Q; q0 += kChunk) {
    const int cnt = min(kChunk, Q - q0);
    __syncthreads();  // the previous chunk is fully read
    for (int t = threadIdx.x; t < cnt; t += kOwn * kWaves) {
      uint8_t f = 1;
      stage[t] = op.stage(q0 + t, f);
      if constexpr (Op::kFlag) sflag[t] = f;
    }
    __syncthreads();
    const int t1 = min(cnt, (wave + 1) * kQuarter);
#pragma unroll 4
    for (int t = wave * kQuarter; t < t1; ++t) {  // ascending, strict <: the first minimum stays
      const float4 s = stage[t];
      uint8_t f = 1;
      if constexpr (Op::kFlag) f = sflag[t];
      float d, u;
      op.eval(own, s, f, d, u);
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
  if (wave != 0) return false;
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
  return true;
}

// matches / scores of both sides and the ones of `positive` (gt_generation.py:55-75 == :130-150).
// positive[i, j] needs j = argmin_row[i], argmin_col[j] = i and dist(i, j) < pos2, and
// dist(i, argmin_row[i]) is rmin[i].  kValid: `negative` is and-ed with the point's depth validity
// (:64-65) and ign0 / ign1 (when not null) receive matches == -2 as bytes.
template <bool kValid>
__global__ __launch_bounds__(256) void gt_finalize(const float* __restrict__ rmin, const int* __restrict__ rarg,
                                                   const float* __restrict__ rmin0, const float* __restrict__ cmin,
                                                   const int* __restrict__ carg, const float* __restrict__ cmin1, int B,
                                                   int M, int N, float pos2, float neg2, uint8_t* __restrict__ assignment,
                                                   int64_t* __restrict__ m0, int64_t* __restrict__ m1,
                                                   float* __restrict__ s0, float* __restrict__ s1,
                                                   const uint8_t* __restrict__ valid0, const uint8_t* __restrict__ valid1,
                                                   uint8_t* __restrict__ ign0, uint8_t* __restrict__ ign1) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t nr = (size_t)B * M, nc = (size_t)B * N;
  if (t < nr) {
    const size_t b = t / M;
    const int i = (int)(t - b * M), j = rarg[t];
    const bool pos = carg[b * N + j] == i && rmin[t] < pos2;
    int64_t m = pos ? (int64_t)j : -2;
    bool neg = rmin0[t] > neg2;
    if constexpr (kValid) neg = neg && valid0[t];
    if (neg) m = -1;
    m0[t] = m;
    s0[t] = m > -1 ? 1.f : 0.f;
    if (pos) assignment[(b * M + i) * N + j] = 1;
    if constexpr (kValid)
      if (ign0) ign0[t] = m == -2;
  } else if (t < nr + nc) {
    const size_t c = t - nr, b = c / N;
    const int j = (int)(c - b * N), i = carg[c];
    const bool pos = rarg[b * M + i] == j && cmin[c] < pos2;
    int64_t m = pos ? (int64_t)i : -2;
    bool neg = cmin1[c] > neg2;
    if constexpr (kValid) neg = neg && valid1[c];
    if (neg) m = -1;
    m1[c] = m;
    s1[c] = m > -1 ? 1.f : 0.f;
    if constexpr (kValid)
      if (ign1) ign1[c] = m == -2;
  }
}

// The reward writer.  A pair's block is a flat run of MN floats; thread g owns the four entries from
// head + 4 g, where head is the distance to the first 16-byte boundary, and thread 0 also writes the
// head.  Op::row(i) loads what a row contributes (reloaded only where the flat run wraps into the next
// row), Op::value(row, j) is the entry.
template <class Op>
__device__ __forceinline__ void write_flat(const Op& op, float* __restrict__ out, unsigned M, unsigned N, unsigned g) {
  const unsigned MN = M * N;
  const unsigned head = min(MN, (unsigned)(((16 - ((uintptr_t)out & 15)) & 15) >> 2));
  if (g == 0)
    for (unsigned r = 0; r < head; ++r) out[r] = op.value(op.row(r / N), r % N);
  const unsigned long long r0 = head + 4ull * g;
  if (r0 >= MN) return;
  unsigned i = (unsigned)r0 / N, j = (unsigned)r0 - i * N;
  const unsigned left = MN - (unsigned)r0;
  typename Op::Row row = op.row(i);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if ((unsigned)k < left) {
      v[k] = op.value(row, j);
      if (++j == N) {
        j = 0;
        if (++i < M) row = op.row(i);
      }
    }
  }
  if (left >= 4) {
    *reinterpret_cast<float4*>(out + r0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (unsigned k = 0; k < left; ++k) out[r0 + k] = v[k];
  }
}

}  // namespace gt
}  // namespace lg
