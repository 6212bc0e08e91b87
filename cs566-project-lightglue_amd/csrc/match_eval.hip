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

#include "kernels.h"

namespace lg {
namespace {

constexpr int EV_THREADS = 256, EV_WAVES = EV_THREADS / 64;
// cyclic Jacobi on 9x9 in fp64 ends in 5-7 sweeps; the cap bounds a matrix with a zero eigenvalue, whose
// rotations never become negligible against it
constexpr int EV_SWEEPS = 12;

// sum of v[k] over the workgroup, returned to every thread; red: EV_WAVES * K doubles of LDS
template <int K>
__device__ inline void block_sum(double (&v)[K], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  __syncthreads();  // the previous reduction's readers are done with red
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = red[k];
#pragma unroll
    for (int w = 1; w < EV_WAVES; ++w) s += red[w * K + k];
    v[k] = s;
  }
}

// lanes of one wave meet here between LDS phases of the Jacobi solve (they run in lockstep; this
// keeps the compiler from moving LDS accesses across the point)
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 3x3 inverse by the adjugate (row-major)
__device__ inline void inverse3(const double (&h)[9], double (&o)[9]) {
  const double c0 = h[4] * h[8] - h[5] * h[7], c1 = h[5] * h[6] - h[3] * h[8], c2 = h[3] * h[7] - h[4] * h[6];
  const double r = 1.0 / (h[0] * c0 + h[1] * c1 + h[2] * c2);
  o[0] = c0 * r, o[1] = (h[2] * h[7] - h[1] * h[8]) * r, o[2] = (h[1] * h[5] - h[2] * h[4]) * r;
  o[3] = c1 * r, o[4] = (h[0] * h[8] - h[2] * h[6]) * r, o[5] = (h[2] * h[3] - h[0] * h[5]) * r;
  o[6] = c2 * r, o[7] = (h[1] * h[6] - h[0] * h[7]) * r, o[8] = (h[0] * h[4] - h[1] * h[3]) * r;
}

// from_homogeneous(h (x, y, 1)) - (u, v), its norm
__device__ inline double warp_dist(const double (&h)[9], double x, double y, double u, double v) {
  const double w = h[6] * x + h[7] * y + h[8];
  const double dx = (h[0] * x + h[1] * y + h[2]) / w - u, dy = (h[3] * x + h[4] * y + h[5]) / w - v;
  return sqrt(dx * dx + dy * dy);
}

// Symmetric 9x9 eigenproblem by cyclic Jacobi, run by one wave on a [9][9] LDS image: A (overwritten;
// its diagonal ends as the eigenvalues) and V (starts as the identity, ends with the eigenvectors in
// its columns).  Lane k < 9 owns row k of V and, through the symmetry, the entries (k, p), (p, k),
// (k, q), (q, k) of a rotation in the plane (p, q); lane p also writes the 2x2 pivot block.  All lanes
// read the pivot block and compute the same c and s, so the loop stays uniform.
__device__ inline void jacobi9(volatile double* A, volatile double* V, int lane) {
  for (int sweep = 0; sweep < EV_SWEEPS; ++sweep) {
    double off = 0.0;
    for (int e = 0; e < 81; ++e)  // the same 81 broadcast reads on every lane: a uniform test
      if (e / 9 != e % 9) off += fabs(A[e]);
    if (off == 0.0) break;  // converged to the last bit: the rule below zeroes what no longer counts
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const double apq = A[p * 9 + q];
        if (apq == 0.0) continue;  // uniform
        const double app = A[p * 9 + p], aqq = A[q * 9 + q];
        const double g = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
          // negligible against both diagonal entries: drop it instead of rotating (uniform)
          if (lane == 0) A[p * 9 + q] = 0.0, A[q * 9 + p] = 0.0;
          wave_sync();
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        const int k = lane < 9 ? lane : 0;
        const double akp = A[k * 9 + p], akq = A[k * 9 + q], vkp = V[k * 9 + p], vkq = V[k * 9 + q];
        wave_sync();  // every lane has its old values
        if (lane < 9) {
          V[k * 9 + p] = cs * vkp - sn * vkq;
          V[k * 9 + q] = sn * vkp + cs * vkq;
          if (k == p) {
            A[p * 9 + p] = app - t * apq;
            A[q * 9 + q] = aqq + t * apq;
            A[p * 9 + q] = 0.0;
            A[q * 9 + p] = 0.0;
          } else if (k != q) {
            const double np = cs * akp - sn * akq, nq = sn * akp + cs * akq;
            A[k * 9 + p] = np, A[p * 9 + k] = np;
            A[k * 9 + q] = nq, A[q * 9 + k] = nq;
          }
        }
        wave_sync();
      }
  }
}

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
    const double U[6] = {w * x * x, w * x * y, w * x, w * y * y, w * y, w};
    const double r2 = X * X + Y * Y;
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] += U[k], S[6 + k] += X * U[k], S[12 + k] += Y * U[k], S[18 + k] += r2 * U[k];
  }
  block_sum(S, red);
  __syncthreads();  // every thread has read the partials
  if (tid == 0)
#pragma unroll
    for (int k = 0; k < 24; ++k) red[k] = S[k];
  __syncthreads();
  if (tid < 81) {
    const int r = tid / 9, q = tid % 9;
    const int br = min(r / 3, q / 3), bc = max(r / 3, q / 3);
    const int ur = min(r % 3, q % 3), uc = max(r % 3, q % 3);
    const int ui = (ur == 0 ? 0 : ur == 1 ? 2 : 3) + uc;  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -> 0..5
    double a = 0.0;
    if (br == bc) a = red[(br == 2 ? 18 : 0) + ui];
    else if (bc == 2) a = -red[(br == 0 ? 6 : 12) + ui];
    jA[tid] = a;
    jV[tid] = r == q ? 1.0 : 0.0;
  }
  __syncthreads();
  if (tid >= 64) return;

  jacobi9(jA, jV, tid);
  wave_sync();
  int best = 0;
  double ev = jA[0];
  for (int k = 1; k < 9; ++k) {
    const double e = jA[k * 9 + k];
    if (e < ev) ev = e, best = k;
  }
  double h[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = jV[k * 9 + best];
  // T2^-1 h T1, T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]]
  double X[9], G[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    X[3 * r] = h[3 * r] * s0, X[3 * r + 1] = h[3 * r + 1] * s0;
    X[3 * r + 2] = h[3 * r + 2] - s0 * (m0x * h[3 * r] + m0y * h[3 * r + 1]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    G[k] = X[k] / s1 + m1x * X[6 + k];
    G[3 + k] = X[3 + k] / s1 + m1y * X[6 + k];
    G[6 + k] = X[6 + k];
  }
  const double g22 = G[8] + 1e-8;
#pragma unroll
  for (int k = 0; k < 9; ++k) G[k] /= g22;
  // homography_corner_error against H_gt on the corners of image 0
  const double W = c.size0[(int64_t)b * 2], Hh = c.size0[(int64_t)b * 2 + 1];
  const double cx[4] = {0.0, W, W, 0.0}, cy[4] = {0.0, 0.0, Hh, Hh};
  double err = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double wg = H[6] * cx[k] + H[7] * cy[k] + H[8];
    const double ug = (H[0] * cx[k] + H[1] * cy[k] + H[2]) / wg, vg = (H[3] * cx[k] + H[4] * cy[k] + H[5]) / wg;
    err += warp_dist(G, cx[k], cy[k], ug, vg);
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Hout[k] = (float)G[k];
    c.H_err[b] = (float)(err / 4.0);
  }
}

}  // namespace

hipError_t eval_matches(const EvalCall& c, hipStream_t st) {
  hipLaunchKernelGGL(match_eval_kernel, dim3(c.B), dim3(EV_THREADS), 0, st, c);
  return hipGetLastError();
}

}  // namespace lg
