// Batched match evaluation (include/lightglue_mi355x.h: lg_eval_matches): what
// gluefactory/eval/utils.py:40-91,176-196 computes from matches0 / matching_scores0, one workgroup
// per pair and one launch per batch.
//
//   homography precision  geometry/homography.py:314-323 (sym_homography_error), counts below 1 and 3 px
//   epipolar precision    geometry/epipolar.py:32-56,75-85 (essential = True, squared = False), counts
//                         below 1e-4, 5e-4, 1e-3
//   weighted DLT          hpatches_metrics.find_homography_dlt + homography_corner_error
//
// Every metric is a masked reduction over the pair's M query keypoints: thread t adds matches t,
// t + 256, ... in that order, a wave64 shuffle tree adds the lanes, the four waves' partials meet in
// LDS and are added in wave order.  No atomics, so the same input gives the same bits.  Inputs are
// fp32, all arithmetic is fp64 (a few hundred flops per match).  The counts ride in the same fp64
// reduction as the sums (exact below 2^53).
#include <hip/hip_runtime.h>

#include <cmath>

#include "dlt_common.h"
#include "kernels.h"

namespace lg {
namespace {

__global__ __launch_bounds__(EV_THREADS) void match_eval_kernel(const EvalCall c) {
  __shared__ double red[EV_WAVES * 24];
  __shared__ double jA[81], jV[81];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = c.M, N = c.N;
  int n0 = M, n1 = N;
  if (c.num0) {  // a ragged batch: slots past the counts are padding, whatever they hold
    n0 = min(max(c.num0[b], 0), M);
    n1 = min(max(c.num1[b], 0), N);
  }
  const float* kp0 = c.kp0 + (int64_t)b * M * 2;
  const float* kp1 = c.kp1 + (int64_t)b * N * 2;
  const int64_t* m0 = c.m0 + (int64_t)b * M;
  const bool hom = c.flags & 1, epi = c.flags & 2, dlt = c.flags & 4;

  double H[9] = {}, Hi[9] = {};
  if (hom || dlt) {
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = c.H[(int64_t)b * 9 + k];
    if (hom) inverse3(H, Hi);
  }
  double E[9] = {}, f0x = 1, f0y = 1, c0x = 0, c0y = 0, f1x = 1, f1y = 1, c1x = 0, c1y = 0;
  if (epi) {
    const float *a0 = c.cam0 + (int64_t)b * 6, *a1 = c.cam1 + (int64_t)b * 6, *T = c.T + (int64_t)b * 12;
    f0x = a0[2], f0y = a0[3], c0x = a0[4], c0y = a0[5];
    f1x = a1[2], f1y = a1[3], c1x = a1[4], c1y = a1[5];
    const double tx = T[9], ty = T[10], tz = T[11];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // E = [t]x R, column k
      const double r0 = T[k], r1 = T[3 + k], r2 = T[6 + k];
      E[k] = -tz * r1 + ty * r2;
      E[3 + k] = tz * r0 - tx * r2;
      E[6 + k] = -ty * r0 + tx * r1;
    }
  }

  // ---- pass 1: n, the five threshold counts and the coordinate sums of the two Hartley means
  double acc[10] = {};
  for (int64_t i = tid; i < n0; i += EV_THREADS) {
    const int64_t j = m0[i];
    if (j < 0 || j >= n1) continue;
    const double x0 = kp0[2 * i], y0 = kp0[2 * i + 1], x1 = kp1[2 * j], y1 = kp1[2 * j + 1];
    acc[0] += 1.0;
    if (hom) {
      const double err = (warp_dist(H, x0, y0, x1, y1) + warp_dist(Hi, x1, y1, x0, y0)) / 2.0;
      acc[1] += err < 1.0 ? 1.0 : 0.0;
      acc[2] += err < 3.0 ? 1.0 : 0.0;
    }
    if (epi) {
      const double px = (x0 - c0x) / f0x, py = (y0 - c0y) / f0y, qx = (x1 - c1x) / f1x, qy = (y1 - c1y) / f1y;
      const double e0 = E[0] * px + E[1] * py + E[2], e1 = E[3] * px + E[4] * py + E[5], e2 = E[6] * px + E[7] * py + E[8];
      const double g0 = E[0] * qx + E[3] * qy + E[6], g1 = E[1] * qx + E[4] * qy + E[7];
      const double d0 = fmax(e0 * e0 + e1 * e1, 1e-6), d1 = fmax(g0 * g0 + g1 * g1, 1e-6);
      const double d = fabs(qx * e0 + qy * e1 + e2) * (1.0 / sqrt(d0) + 1.0 / sqrt(d1)) / 2.0;
      acc[3] += d < 1e-4 ? 1.0 : 0.0;
      acc[4] += d < 5e-4 ? 1.0 : 0.0;
      acc[5] += d < 1e-3 ? 1.0 : 0.0;
    }
    if (dlt) acc[6] += x0, acc[7] += y0, acc[8] += x1, acc[9] += y1;
  }
  block_sum(acc, red);
  if (tid == 0) {
    if (hom) {
      int* o = c.hom_counts + (int64_t)b * 3;
      o[0] = (int)acc[0], o[1] = (int)acc[1], o[2] = (int)acc[2];
    }
    if (epi) {
      int* o = c.epi_counts + (int64_t)b * 4;
      o[0] = (int)acc[0], o[1] = (int)acc[3], o[2] = (int)acc[4], o[3] = (int)acc[5];
    }
  }
  if (!dlt) return;

  float* Hout = c.H_dlt + (int64_t)b * 9;
  const double n = acc[0];
  if (n < 4.0) {  // hpatches_metrics.eval_homography_dlt: an all-inf homography, its corner error 0 * inf
    if (tid < 9) Hout[tid] = INFINITY;
    if (tid == 0) c.H_err[b] = NAN;
    return;
  }
  const float* sc = c.s0 + (int64_t)b * M;
  const double m0x = acc[6] / n, m0y = acc[7] / n, m1x = acc[8] / n, m1y = acc[9] / n;

  // ---- pass 2: mean distance to each mean -> the two Hartley scales
  double dist[2] = {};
  for (int64_t i = tid; i < n0; i += EV_THREADS) {
    const int64_t j = m0[i];
    if (j < 0 || j >= n1) continue;
    const double ax = kp0[2 * i] - m0x, ay = kp0[2 * i + 1] - m0y, bx = kp1[2 * j] - m1x, by = kp1[2 * j + 1] - m1y;
    dist[0] += sqrt(ax * ax + ay * ay);
    dist[1] += sqrt(bx * bx + by * by);
  }
  block_sum(dist, red);
  const double s0 = 1.4142135623730951 / (dist[0] / n + 1e-8), s1 = 1.4142135623730951 / (dist[1] / n + 1e-8);

  // ---- pass 3: A^T W A.  With u = (x, y, 1) of image 0 and (X, Y) of image 1 (both normalised) a
  // match's two rows are (0, -u, Y u) and (u, 0, -X u), so the 9x9 matrix is 3x3 blocks of
  // U = w u u^T: [[U, 0, -X U], [0, U, -Y U], [-X U, -Y U, (X^2 + Y^2) U]].  Its 45 unique entries
  // are these 24 sums (6 unique entries of U, times 1, X, Y, X^2 + Y^2).
  double S[24] = {};
  for (int64_t i = tid; i < n0; i += EV_THREADS) {
    const int64_t j = m0[i];
    if (j < 0 || j >= n1) continue;
    const double x = s0 * (kp0[2 * i] - m0x), y = s0 * (kp0[2 * i + 1] - m0y);
    const double X = s1 * (kp1[2 * j] - m1x), Y = s1 * (kp1[2 * j + 1] - m1y);
    const double w = sc[i];
    dlt_accumulate(S, x, y, X, Y, w);
  }
  block_sum(S, red);
  dlt_build_system(S, red, jA, jV);
  if (tid >= 64) return;

  jacobi9(jA, jV, tid);
  wave_sync();
  double G[9];
  dlt_solution(jA, jV, s0, m0x, m0y, s1, m1x, m1y, G);
  const double g22 = G[8] + 1e-8;
#pragma unroll
  for (int k = 0; k < 9; ++k) G[k] /= g22;
  // homography_corner_error against H_gt on the corners of image 0
  const double W = c.size0[(int64_t)b * 2], Hh = c.size0[(int64_t)b * 2 + 1];
  const double err = corner_error(H, G, W, Hh);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Hout[k] = (float)G[k];
    c.H_err[b] = (float)err;
  }
}

}  // namespace

hipError_t eval_matches(const EvalCall& c, hipStream_t st) {
  hipLaunchKernelGGL(match_eval_kernel, dim3(c.B), dim3(EV_THREADS), 0, st, c);
  return hipGetLastError();
}

}  // namespace lg
