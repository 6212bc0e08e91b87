// What the homography kernels share (match_eval.hip, ransac_homography.hip): the workgroup sum, the
// Hartley-normalised DLT's building blocks in fp64 (the 24 sums of A^T W A, its 9x9 image, the cyclic
// Jacobi eigen-solve on one wave, the denormalisation) and the corner error.  Device code only; every
// function runs in a workgroup of EV_THREADS threads.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

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

// One match's share of A^T W A.  With u = (x, y, 1) of image 0 and (X, Y) of image 1 (both normalised)
// a match's two rows are (0, -u, Y u) and (u, 0, -X u), so the 9x9 matrix is 3x3 blocks of
// U = w u u^T: [[U, 0, -X U], [0, U, -Y U], [-X U, -Y U, (X^2 + Y^2) U]].  Its 45 unique entries
// are these 24 sums (6 unique entries of U, times 1, X, Y, X^2 + Y^2).
__device__ inline void dlt_accumulate(double (&S)[24], double x, double y, double X, double Y, double w) {
  const double U[6] = {w * x * x, w * x * y, w * x, w * y * y, w * y, w};
  const double r2 = X * X + Y * Y;
#pragma unroll
  for (int k = 0; k < 6; ++k) S[k] += U[k], S[6 + k] += X * U[k], S[12 + k] += Y * U[k], S[18 + k] += r2 * U[k];
}

// The workgroup's 24 sums (in every thread after block_sum) -> the 9x9 image jA and the identity jV
// in LDS; red is block_sum's buffer.  Ends on a barrier.
__device__ inline void dlt_build_system(const double (&S)[24], double* red, double* jA, double* jV) {
  const int tid = threadIdx.x;
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
}

// After jacobi9 on one wave: the eigenvector of the smallest eigenvalue, taken out of the Hartley
// frames: G = T2^-1 h T1, T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]].  Not yet scaled.
__device__ inline void dlt_solution(const double* jA, const double* jV, double s0, double m0x, double m0y, double s1,
                                    double m1x, double m1y, double (&G)[9]) {
  int best = 0;
  double ev = jA[0];
  for (int k = 1; k < 9; ++k) {
    const double e = jA[k * 9 + k];
    if (e < ev) ev = e, best = k;
  }
  double h[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = jV[k * 9 + best];
  double X[9];
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
}

// homography_corner_error of G against H on the corners of a W x Hh image
__device__ inline double corner_error(const double (&H)[9], const double (&G)[9], double W, double Hh) {
  const double cx[4] = {0.0, W, W, 0.0}, cy[4] = {0.0, 0.0, Hh, Hh};
  double err = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double wg = H[6] * cx[k] + H[7] * cy[k] + H[8];
    const double ug = (H[0] * cx[k] + H[1] * cy[k] + H[2]) / wg, vg = (H[3] * cx[k] + H[4] * cy[k] + H[5]) / wg;
    err += warp_dist(G, cx[k], cy[k], ug, vg);
  }
  return err / 4.0;
}

}  // namespace
}  // namespace lg
