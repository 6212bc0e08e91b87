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
// The scan of gt_stats, gt_fill0, gt_finalize and the flat writer of gt_reward are the templates of
// gt_common.h, shared with the pose-and-depth ground truth (gt_depth.hip); this file supplies the
// homography arithmetic they run.
//
// This TU is built with -ffp-contract=off (Makefile): every subtraction, product and sum of a distance
// is rounded on its own, as the reference's separate torch passes do, and pass 1 and the write pass
// get the same bits for the same (i, j).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gt_common.h"
#include "kernels.h"

namespace lg {
namespace {

using namespace gt;

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

// warp and invert_h (the reference's from_homogeneous(points @ H^T) and the fp64-adjugate inverse) are in
// gt_common.h, shared with the line ground truth (gt_lines.hip)
__global__ __launch_bounds__(256) void gt_project(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                  const float* __restrict__ H, int M, int N, int bpp,
                                                  float* __restrict__ p01, float* __restrict__ p10) {
  const int b = blockIdx.x / bpp;
  const int t = (blockIdx.x - b * bpp) * 256 + threadIdx.x;
  float h[9], hi[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = H[(size_t)b * 9 + k];
  invert_h(h, hi);
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
// third statistic is min u, so one body serves both directions (gt_common.h: scan).
struct HomographyScan {
  static constexpr bool kFlag = false;
  struct Own {
    float x, y, px, py;
  };
  const float2 *oth_raw, *oth_prj;
  __device__ __forceinline__ float4 stage(int q, uint8_t&) const {
    const float2 r = oth_raw[q], pr = oth_prj[q];
    return make_float4(r.x, r.y, pr.x, pr.y);
  }
  __device__ __forceinline__ void eval(const Own& o, float4 s, uint8_t, float& d, float& u) const {
    u = sqd(o.px, o.py, s.x, s.y);
    const float v = sqd(o.x, o.y, s.z, s.w);
    d = fmaxf(u, v);
  }
};

__global__ __launch_bounds__(kOwn* kWaves) void gt_stats(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                         const float* __restrict__ p01, const float* __restrict__ p10,
                                                         int B, int M, int N, int bm, int bn,
                                                         float* __restrict__ rmin, int* __restrict__ rarg,
                                                         float* __restrict__ rmin0, float* __restrict__ cmin,
                                                         int* __restrict__ carg, float* __restrict__ cmin1) {
  int blk = blockIdx.x;
  const bool cols = blk >= B * bm;
  if (cols) blk -= B * bm;
  const int per = cols ? bn : bm;
  const int b = blk / per;
  const int P = cols ? N : M, Q = cols ? M : N;  // owned side, scanned side
  const float* own_raw = (cols ? kp1 : kp0) + (size_t)b * P * 2;
  const float* own_prj = (cols ? p10 : p01) + (size_t)b * P * 2;
  HomographyScan op;
  op.oth_raw = reinterpret_cast<const float2*>((cols ? kp0 : kp1) + (size_t)b * Q * 2);
  op.oth_prj = reinterpret_cast<const float2*>((cols ? p01 : p10) + (size_t)b * Q * 2);

  const int lane = threadIdx.x & (kOwn - 1);
  const int p = (blk - b * per) * kOwn + lane;
  const bool live = p < P;
  HomographyScan::Own own = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float2 r = reinterpret_cast<const float2*>(own_raw)[p], q = reinterpret_cast<const float2*>(own_prj)[p];
    own = {r.x, r.y, q.x, q.y};
  }
  float best, third;
  int arg;
  if (scan(op, own, Q, best, arg, third) && live) {
    const size_t o = (size_t)b * P + p;
    (cols ? cmin : rmin)[o] = best;
    (cols ? carg : rarg)[o] = arg;
    (cols ? cmin1 : rmin0)[o] = third;
  }
}

// reward (:128): (dist < pos_th^2) - (dist > neg_th^2) with dist recomputed by the same expression
// (gt_common.h: write_flat).  Keypoints as 8-byte loads (the API checks the alignment).
struct HomographyReward {
  struct Row {
    float2 a, pa;
  };
  const float2 *a2, *pa2, *b2, *pb2;
  float pos2, neg2;
  __device__ __forceinline__ Row row(unsigned i) const { return {a2[i], pa2[i]}; }
  __device__ __forceinline__ float value(const Row& r, unsigned j) const {
    const float2 cb = b2[j], cpb = pb2[j];
    const float d = pair_dist(r.a.x, r.a.y, r.pa.x, r.pa.y, cb.x, cb.y, cpb.x, cpb.y).d;
    return (d < pos2 ? 1.f : 0.f) - (d > neg2 ? 1.f : 0.f);
  }
};

__global__ __launch_bounds__(256) void gt_reward(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                 const float* __restrict__ p01, const float* __restrict__ p10, int M, int N,
                                                 unsigned bpp, float pos2, float neg2, float* __restrict__ reward) {
  const unsigned b = blockIdx.x / bpp;
  const unsigned g = (blockIdx.x - b * bpp) * 256u + threadIdx.x;
  HomographyReward op;
  op.a2 = reinterpret_cast<const float2*>(kp0 + (size_t)b * M * 2);
  op.pa2 = reinterpret_cast<const float2*>(p01 + (size_t)b * M * 2);
  op.b2 = reinterpret_cast<const float2*>(kp1 + (size_t)b * N * 2);
  op.pb2 = reinterpret_cast<const float2*>(p10 + (size_t)b * N * 2);
  op.pos2 = pos2;
  op.neg2 = neg2;
  write_flat(op, reward + (size_t)b * (unsigned)M * (unsigned)N, (unsigned)M, (unsigned)N, g);
}

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
  launch_fill0(assignment, (size_t)B * M * N, st);
  const size_t nfin = (size_t)B * M + (size_t)B * N;
  gt_finalize<false><<<dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, st>>>(
      rmin, rarg, rmin0, cmin, carg, cmin1, B, M, N, pos2, neg2, assignment, m0, m1, s0, s1, nullptr, nullptr, nullptr, nullptr);
  if (reward) {
    const unsigned rpp = (unsigned)(((size_t)M * N / 4 + 1 + 255) / 256);
    gt_reward<<<dim3((unsigned)B * rpp), dim3(256), 0, st>>>(kp0, kp1, p01, p10, M, N, rpp, pos2, neg2, reward);
  }
  return hipGetLastError();
}

}  // namespace lg
