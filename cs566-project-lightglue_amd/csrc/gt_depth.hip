// Pose-and-depth ground truth on the device: gt_matches_from_pose_depth (reference
// gluefactory/geometry/gt_generation.py:13-106 over sample_depth / project, geometry/depth.py:8-68, the
// Camera / Pose wrappers, geometry/wrappers.py, distort_points, geometry/utils.py:90-127, and
// sym_epipolar_distance_all, geometry/epipolar.py:59-72) without any [B, M, N] intermediate.
// Per pair: kp0 [M,2], kp1 [N,2], depth0 [H0,W0], depth1 [H1,W1], camera rows
// (w, h, fx, fy, cx, cy [, k1, k2 [, p1, p2]]), pose rows (R row-major, t), all fp32.
//
//   gtd_points     one launch over both images, one thread per keypoint: the depth at the keypoint
//                  (grid_sample bilinear with the nearest sample where that is NaN, over the map with
//                  every value <= 0 turned into NaN) or the caller's; the projection into the other
//                  camera with its validity; with th_consistency the way back through the other depth
//                  map; `visible`; and, where the epipolar distance is needed, per point the line
//                  F p0 (image 0) or the point and |(F^T p1)_xy| (image 1).  F = K1^-T [t]x R K0^-1 in
//                  fp64 from the fp32 rows, rounded once to fp32.
//   gtd_stats      the scan of gt_common.h with dist masked by visible0[i] && visible1[j]; the third
//                  statistic (min dist0 per row, min dist1 per column) stays unmasked (:64-65)
//   gt_fill0, gt_finalize<true>   as the homography path, `negative` and-ed with the depth validity
//   gtd_epi_stats  th_epi only: per point without valid depth, the minimum epipolar distance over the
//                  ignored (-2) points of the other image (:86-89)
//   gtd_reward     (dist < pos_th^2) - (epi > neg_th), epi masked to ignored x ignored with th_epi (:87,95)
//   gtd_epi_apply  th_epi only: matches = -1 where the depth is not valid and that minimum > neg_th (:90-91);
//                  after the reward, which reads the labels from before this step as the reference does
//
// Built with -ffp-contract=off (Makefile), like gt_match.hip: the scan and the reward pass get the
// same bits for the same (i, j).  No atomics; identical results run to run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gt_common.h"
#include "gt_depth_common.h"
#include "kernels.h"

namespace lg {
namespace {

using namespace gt;

// sym_epipolar_distance_all (epipolar.py:59-72) from the per-point halves: e0 = (F p0, sqrt(|F p0|_xy^2 + eps))
// of the image-0 point, e1 = (p1, sqrt(|F^T p1|_xy^2 + eps)) of the image-1 point
__device__ __forceinline__ float epi_dist(float4 e0, float4 e1) {
  const float n = fabsf((e1.x * e0.x + e1.y * e0.y) + e0.z);
  return (n / e0.w + n / e1.z) / 2.f;
}

struct PointArgs {
  const float *kp0, *kp1, *depth0, *depth1, *cam0, *cam1, *T01, *T10;
  int H0, W0, H1, W1, nd, M, N;
  int pre, cc, epi;
  float ccth;
  float *dk0, *dk1;
  const uint8_t *vin0, *vin1;
  uint8_t *valid0, *valid1, *vis0, *vis1;
  float *p01, *p10;
  float4 *E0, *E1;
};

__global__ __launch_bounds__(256) void gtd_points(PointArgs a, int bpp) {
  const int side = blockIdx.y;
  const int b = blockIdx.x / bpp;
  const int t = (blockIdx.x - b * bpp) * 256 + threadIdx.x;
  const int P = side ? a.N : a.M;
  if (t >= P) return;
  const int cw = 6 + a.nd;
  const Cam c0 = load_cam(a.cam0 + (size_t)b * cw, a.nd), c1 = load_cam(a.cam1 + (size_t)b * cw, a.nd);
  const Cam& ci = side ? c1 : c0;
  const Cam& cj = side ? c0 : c1;
  const PoseRt T = load_pose((side ? a.T10 : a.T01) + (size_t)b * 12);
  const float *R = T.R, *tr = T.t;
  const float* mi = side ? a.depth1 : a.depth0;
  const float* mj = side ? a.depth0 : a.depth1;
  const int Hi = side ? a.H1 : a.H0, Wi = side ? a.W1 : a.W0, Hj = side ? a.H0 : a.H1, Wj = side ? a.W0 : a.W1;
  const size_t o = (size_t)b * P + t;
  const float2 kp = reinterpret_cast<const float2*>(side ? a.kp1 : a.kp0)[o];

  float d;
  bool valid;
  if (a.pre) {  // gt_generation.py:31-33
    d = (side ? a.dk1 : a.dk0)[o];
    valid = (side ? a.vin1 : a.vin0)[o] != 0;
  } else {
    d = sample_depth(mi + (size_t)b * Hi * Wi, Hi, Wi, kp.x, kp.y);
    valid = depth_valid(d);
    (side ? a.dk1 : a.dk0)[o] = d;
  }
  (side ? a.valid1 : a.valid0)[o] = valid;

  // depth.py:52-59: image2cam (no undistortion), times the depth, T.transform, cam2image
  const P2 pj = project_to(ci, cj, a.nd, T, kp.x, kp.y, d);
  bool vis = valid && pj.ok;
  if (a.cc) {  // depth.py:61-68, T_itoj.inv() as Pose.inv computes it (wrappers.py:173-177)
    const float dj = sample_depth(mj + (size_t)b * Hj * Wj, Hj, Wj, pj.x, pj.y);
    const bool vdj = depth_valid(dj);
    const float lx = ((pj.x - cj.cx) / cj.fx) * dj, ly = ((pj.y - cj.cy) / cj.fy) * dj, lz = 1.f * dj;
    const float ti0 = -((R[0] * tr[0] + R[3] * tr[1]) + R[6] * tr[2]);
    const float ti1 = -((R[1] * tr[0] + R[4] * tr[1]) + R[7] * tr[2]);
    const float ti2 = -((R[2] * tr[0] + R[5] * tr[1]) + R[8] * tr[2]);
    const float bx = ((lx * R[0] + ly * R[3]) + lz * R[6]) + ti0;
    const float by = ((lx * R[1] + ly * R[4]) + lz * R[7]) + ti1;
    const float bz = ((lx * R[2] + ly * R[5]) + lz * R[8]) + ti2;
    const P2 back = cam2image(ci, a.nd, bx, by, bz);
    // the squared distance against the unsquared threshold, as the reference compares them
    const bool consistent = sqd(kp.x, kp.y, back.x, back.y) < a.ccth;
    vis = vis && consistent && back.ok && vdj;
  }
  float* prj = (side ? a.p10 : a.p01) + o * 2;
  prj[0] = pj.x;
  prj[1] = pj.y;
  (side ? a.vis1 : a.vis0)[o] = vis;

  if (a.epi) {
    // F = K1^-T [t]x R K0^-1 (gt_generation.py:77-81) of T_0to1, in fp64, rounded once
    const float* T0 = a.T01 + (size_t)b * 12;
    double Rm[9], tt[3], E[9], A[9], F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm[k] = T0[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tt[k] = T0[9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      E[k] = -tt[2] * Rm[3 + k] + tt[1] * Rm[6 + k];
      E[3 + k] = tt[2] * Rm[k] - tt[0] * Rm[6 + k];
      E[6 + k] = -tt[1] * Rm[k] + tt[0] * Rm[3 + k];
    }
    const double fx0 = c0.fx, fy0 = c0.fy, cx0 = c0.cx, cy0 = c0.cy, fx1 = c1.fx, fy1 = c1.fy, cx1 = c1.cx, cy1 = c1.cy;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      A[3 * r] = E[3 * r] / fx0;
      A[3 * r + 1] = E[3 * r + 1] / fy0;
      A[3 * r + 2] = E[3 * r + 2] - E[3 * r] * cx0 / fx0 - E[3 * r + 1] * cy0 / fy0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      F[k] = A[k] / fx1;
      F[3 + k] = A[3 + k] / fy1;
      F[6 + k] = A[6 + k] - A[k] * cx1 / fx1 - A[3 + k] * cy1 / fy1;
    }
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = (float)F[k];
    if (side == 0) {
      const float l0 = (f[0] * kp.x + f[1] * kp.y) + f[2];
      const float l1 = (f[3] * kp.x + f[4] * kp.y) + f[5];
      const float l2 = (f[6] * kp.x + f[7] * kp.y) + f[8];
      a.E0[o] = make_float4(l0, l1, l2, sqrtf((l0 * l0 + l1 * l1) + 1e-15f));
    } else {
      const float m0 = (f[0] * kp.x + f[3] * kp.y) + f[6];
      const float m1 = (f[1] * kp.x + f[4] * kp.y) + f[7];
      a.E1[o] = make_float4(kp.x, kp.y, sqrtf((m0 * m0 + m1 * m1) + 1e-15f), 0.f);
    }
  }
}

// dist(i, j) = visible0[i] && visible1[j] ? max(dist0, dist1) : +inf (:46-53); u as in gt_match.hip.
// A NaN projection belongs to a point that is not visible, so it never reaches the masked minimum.
struct DepthScan {
  static constexpr bool kFlag = true;
  struct Own {
    float x, y, px, py;
    bool vis;
  };
  const float2 *oth_raw, *oth_prj;
  const uint8_t* oth_vis;
  __device__ __forceinline__ float4 stage(int q, uint8_t& f) const {
    const float2 r = oth_raw[q], pr = oth_prj[q];
    f = oth_vis[q];
    return make_float4(r.x, r.y, pr.x, pr.y);
  }
  __device__ __forceinline__ void eval(const Own& o, float4 s, uint8_t f, float& d, float& u) const {
    u = sqd(o.px, o.py, s.x, s.y);
    d = __builtin_inff();
    if (o.vis && f) d = fmaxf(u, sqd(o.x, o.y, s.z, s.w));
  }
};

struct StatsArgs {
  const float *kp0, *kp1, *p01, *p10;
  const uint8_t *vis0, *vis1;
  float *rmin, *rmin0, *cmin, *cmin1;
  int *rarg, *carg;
};

__global__ __launch_bounds__(kOwn* kWaves) void gtd_stats(StatsArgs a, int B, int M, int N, int bm, int bn) {
  int blk = blockIdx.x;
  const bool cols = blk >= B * bm;
  if (cols) blk -= B * bm;
  const int per = cols ? bn : bm;
  const int b = blk / per;
  const int P = cols ? N : M, Q = cols ? M : N;  // owned side, scanned side
  const float2* own_raw = reinterpret_cast<const float2*>((cols ? a.kp1 : a.kp0) + (size_t)b * P * 2);
  const float2* own_prj = reinterpret_cast<const float2*>((cols ? a.p10 : a.p01) + (size_t)b * P * 2);
  const uint8_t* own_vis = (cols ? a.vis1 : a.vis0) + (size_t)b * P;
  DepthScan op;
  op.oth_raw = reinterpret_cast<const float2*>((cols ? a.kp0 : a.kp1) + (size_t)b * Q * 2);
  op.oth_prj = reinterpret_cast<const float2*>((cols ? a.p01 : a.p10) + (size_t)b * Q * 2);
  op.oth_vis = (cols ? a.vis0 : a.vis1) + (size_t)b * Q;

  const int lane = threadIdx.x & (kOwn - 1);
  const int p = (blk - b * per) * kOwn + lane;
  const bool live = p < P;
  DepthScan::Own own = {0.f, 0.f, 0.f, 0.f, false};
  if (live) {
    const float2 r = own_raw[p], q = own_prj[p];
    own = {r.x, r.y, q.x, q.y, own_vis[p] != 0};
  }
  float best, third;
  int arg;
  if (scan(op, own, Q, best, arg, third) && live) {
    // torch.min over a row of NaN (the projection of a point without depth) is NaN, and NaN > neg_th^2
    // is false: said here, not left to fminf
    if (own.px != own.px || own.py != own.py) third = __builtin_nanf("");
    const size_t o = (size_t)b * P + p;
    (cols ? a.cmin : a.rmin)[o] = best;
    (cols ? a.carg : a.rarg)[o] = arg;
    (cols ? a.cmin1 : a.rmin0)[o] = third;
  }
}

// th_epi (:85-89): min over the ignored points of the other image of the epipolar distance, for the
// owned points that are ignored and have no valid depth (the only ones :90-91 can change)
struct EpiScan {
  static constexpr bool kFlag = true;
  struct Own {
    float4 e;
  };
  const float4* oth;
  const uint8_t* oth_ign;
  bool cols;
  __device__ __forceinline__ float4 stage(int q, uint8_t& f) const {
    f = oth_ign[q];
    return oth[q];
  }
  __device__ __forceinline__ void eval(const Own& o, float4 s, uint8_t f, float& d, float& u) const {
    u = 0.f;
    d = __builtin_inff();
    if (f) d = cols ? epi_dist(s, o.e) : epi_dist(o.e, s);
  }
};

__global__ __launch_bounds__(kOwn* kWaves) void gtd_epi_stats(const float4* __restrict__ E0, const float4* __restrict__ E1,
                                                              const uint8_t* __restrict__ ign0,
                                                              const uint8_t* __restrict__ ign1,
                                                              const uint8_t* __restrict__ valid0,
                                                              const uint8_t* __restrict__ valid1, int B, int M, int N,
                                                              int bm, int bn, float* __restrict__ emin0,
                                                              float* __restrict__ emin1) {
  int blk = blockIdx.x;
  const bool cols = blk >= B * bm;
  if (cols) blk -= B * bm;
  const int per = cols ? bn : bm;
  const int b = blk / per;
  const int P = cols ? N : M, Q = cols ? M : N;
  const int lane = threadIdx.x & (kOwn - 1);
  const int p = (blk - b * per) * kOwn + lane;
  const bool live = p < P;
  const size_t o = (size_t)b * P + (live ? p : 0);
  const bool need = live && !(cols ? valid1 : valid0)[o] && (cols ? ign1 : ign0)[o];
  if (!__syncthreads_or(need)) return;  // every point of this block has depth: nothing reads its minimum
  EpiScan op;
  op.oth = (cols ? E0 : E1) + (size_t)b * Q;
  op.oth_ign = (cols ? ign0 : ign1) + (size_t)b * Q;
  op.cols = cols;
  EpiScan::Own own = {make_float4(0.f, 0.f, 0.f, 1.f)};
  if (live) own.e = (cols ? E1 : E0)[o];
  float best, third;
  int arg;
  if (scan(op, own, Q, best, arg, third) && live) (cols ? emin1 : emin0)[o] = need ? best : __builtin_inff();
}

__global__ __launch_bounds__(256) void gtd_epi_apply(const float* __restrict__ emin0, const float* __restrict__ emin1,
                                                     const uint8_t* __restrict__ valid0, const uint8_t* __restrict__ valid1,
                                                     size_t nr, size_t nc, float negf, int64_t* __restrict__ m0,
                                                     int64_t* __restrict__ m1) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nr) {
    if (!valid0[t] && emin0[t] > negf) m0[t] = -1;
  } else if (t < nr + nc) {
    const size_t c = t - nr;
    if (!valid1[c] && emin1[c] > negf) m1[c] = -1;
  }
}

// reward (:95) through write_flat: dist masked as in gtd_stats and recomputed by the same expression
struct DepthReward {
  struct Row {
    float2 a, pa;
    float4 e;
    bool vis, ign;
  };
  const float2 *a2, *pa2, *b2, *pb2;
  const float4 *E0, *E1;
  const uint8_t *vis0, *vis1, *ign0, *ign1;
  float pos2, negf;
  bool mask_epi;
  __device__ __forceinline__ Row row(unsigned i) const { return {a2[i], pa2[i], E0[i], vis0[i] != 0, ign0[i] != 0}; }
  __device__ __forceinline__ float value(const Row& r, unsigned j) const {
    float d = __builtin_inff();
    if (r.vis && vis1[j]) {
      const float2 cb = b2[j], cpb = pb2[j];
      d = fmaxf(sqd(r.pa.x, r.pa.y, cb.x, cb.y), sqd(r.a.x, r.a.y, cpb.x, cpb.y));
    }
    float e = __builtin_inff();
    if (!mask_epi || (r.ign && ign1[j])) e = epi_dist(r.e, E1[j]);
    return (d < pos2 ? 1.f : 0.f) - (e > negf ? 1.f : 0.f);
  }
};

__global__ __launch_bounds__(256) void gtd_reward(DepthReward op, int M, int N, unsigned bpp, float* __restrict__ reward) {
  const unsigned b = blockIdx.x / bpp;
  const unsigned g = (blockIdx.x - b * bpp) * 256u + threadIdx.x;
  op.a2 += (size_t)b * M;
  op.pa2 += (size_t)b * M;
  op.E0 += (size_t)b * M;
  op.vis0 += (size_t)b * M;
  op.ign0 += (size_t)b * M;
  op.b2 += (size_t)b * N;
  op.pb2 += (size_t)b * N;
  op.E1 += (size_t)b * N;
  op.vis1 += (size_t)b * N;
  op.ign1 += (size_t)b * N;
  write_flat(op, reward + (size_t)b * (unsigned)M * (unsigned)N, (unsigned)M, (unsigned)N, g);
}

}  // namespace

size_t gt_depth_workspace_bytes(int B, int M, int N) {
  // per point: four 4-byte statistics (min dist, argmin, min dist0 / dist1, min epi), the 16-byte
  // epipolar half, the depth validity and the ignore flag
  const size_t r = (size_t)B * M, c = (size_t)B * N;
  return 4 * up256(r * 4) + up256(r * 16) + 2 * up256(r) + 4 * up256(c * 4) + up256(c * 16) + 2 * up256(c);
}

hipError_t gt_matches_from_pose_depth(const GtDepthCall& c, void* workspace, hipStream_t st) {
  const int B = c.B, M = c.M, N = c.N;
  char* w = static_cast<char*>(workspace);
  auto take = [&](size_t bytes) {
    char* p = w;
    w += up256(bytes);
    return p;
  };
  const size_t nr = (size_t)B * M, nc = (size_t)B * N;
  float4* E0 = reinterpret_cast<float4*>(take(nr * 16));
  float4* E1 = reinterpret_cast<float4*>(take(nc * 16));
  float* rmin = reinterpret_cast<float*>(take(nr * 4));
  int* rarg = reinterpret_cast<int*>(take(nr * 4));
  float* rmin0 = reinterpret_cast<float*>(take(nr * 4));
  float* emin0 = reinterpret_cast<float*>(take(nr * 4));
  float* cmin = reinterpret_cast<float*>(take(nc * 4));
  int* carg = reinterpret_cast<int*>(take(nc * 4));
  float* cmin1 = reinterpret_cast<float*>(take(nc * 4));
  float* emin1 = reinterpret_cast<float*>(take(nc * 4));
  uint8_t* valid0 = reinterpret_cast<uint8_t*>(take(nr));
  uint8_t* ign0 = reinterpret_cast<uint8_t*>(take(nr));
  uint8_t* valid1 = reinterpret_cast<uint8_t*>(take(nc));
  uint8_t* ign1 = reinterpret_cast<uint8_t*>(take(nc));

  const bool need_epi = c.reward != nullptr || c.use_epi;
  PointArgs pa;
  pa.kp0 = c.kp0, pa.kp1 = c.kp1, pa.depth0 = c.depth0, pa.depth1 = c.depth1, pa.cam0 = c.cam0, pa.cam1 = c.cam1;
  pa.T01 = c.T_0to1, pa.T10 = c.T_1to0;
  pa.H0 = c.H0, pa.W0 = c.W0, pa.H1 = c.H1, pa.W1 = c.W1, pa.nd = c.n_dist, pa.M = M, pa.N = N;
  pa.pre = c.valid_in0 != nullptr, pa.cc = c.use_cc, pa.epi = need_epi, pa.ccth = c.ccth;
  pa.dk0 = c.dk0, pa.dk1 = c.dk1, pa.vin0 = c.valid_in0, pa.vin1 = c.valid_in1;
  pa.valid0 = valid0, pa.valid1 = valid1, pa.vis0 = c.vis0, pa.vis1 = c.vis1, pa.p01 = c.p01, pa.p10 = c.p10;
  pa.E0 = E0, pa.E1 = E1;
  const int bpp = (max(M, N) + 255) / 256;
  gtd_points<<<dim3((unsigned)B * bpp, 2), dim3(256), 0, st>>>(pa, bpp);

  const int bm = (M + kOwn - 1) / kOwn, bn = (N + kOwn - 1) / kOwn;
  StatsArgs sa = {c.kp0, c.kp1, c.p01, c.p10, c.vis0, c.vis1, rmin, rmin0, cmin, cmin1, rarg, carg};
  gtd_stats<<<dim3((unsigned)B * (bm + bn)), dim3(kOwn * kWaves), 0, st>>>(sa, B, M, N, bm, bn);
  launch_fill0(c.assignment, (size_t)B * M * N, st);
  const unsigned fin_blocks = (unsigned)((nr + nc + 255) / 256);
  gt_finalize<true><<<dim3(fin_blocks), dim3(256), 0, st>>>(rmin, rarg, rmin0, cmin, carg, cmin1, B, M, N, c.pos2, c.neg2,
                                                           c.assignment, c.m0, c.m1, c.s0, c.s1, valid0, valid1, ign0, ign1);
  if (c.use_epi)
    gtd_epi_stats<<<dim3((unsigned)B * (bm + bn)), dim3(kOwn * kWaves), 0, st>>>(E0, E1, ign0, ign1, valid0, valid1, B, M, N,
                                                                                bm, bn, emin0, emin1);
  if (c.reward) {
    DepthReward op;
    op.a2 = reinterpret_cast<const float2*>(c.kp0), op.pa2 = reinterpret_cast<const float2*>(c.p01);
    op.b2 = reinterpret_cast<const float2*>(c.kp1), op.pb2 = reinterpret_cast<const float2*>(c.p10);
    op.E0 = E0, op.E1 = E1, op.vis0 = c.vis0, op.vis1 = c.vis1, op.ign0 = ign0, op.ign1 = ign1;
    op.pos2 = c.pos2, op.negf = c.negf, op.mask_epi = c.use_epi;
    const unsigned rpp = (unsigned)(((size_t)M * N / 4 + 1 + 255) / 256);
    gtd_reward<<<dim3((unsigned)B * rpp), dim3(256), 0, st>>>(op, M, N, rpp, c.reward);
  }
  if (c.use_epi)
    gtd_epi_apply<<<dim3(fin_blocks), dim3(256), 0, st>>>(emin0, emin1, valid0, valid1, nr, nc, c.negf, c.m0, c.m1);
  return hipGetLastError();
}

}  // namespace lg
