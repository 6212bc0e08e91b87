// Batched LO-RANSAC for homographies (include/lightglue_mi355x.h: lg_ransac_homography; DESIGN.md
// §10k): what the reference's robust homography estimator does for gluefactory/eval/utils.py:132-173,
// one workgroup of 256 threads per pair and one launch per batch.
//
//   phase 0   the pair's live matches are compacted in slot order into m_kpts (a ballot prefix scan,
//             no atomics) and, when they fit, staged in LDS as (x0, y0, x1, y1) rows
//   rounds    256 hypotheses at a time, one per thread: a counter-based sample of four matches, the
//             projective-basis closed form, and the inlier count against every match (all lanes read
//             the same LDS row, a broadcast); the round's best is a workgroup argmax
//   LO        after a round that raised the best minimal count: 8 unweighted DLT refits with shrinking
//             thresholds, by the whole workgroup, on the helpers match_eval.hip uses (dlt_common.h)
//   result    the kept model over h33 in fp32, and the mask that matrix gives in fp64
//
// All arithmetic is fp64 on the fp32 inputs.  Every branch that reaches a barrier is taken on values
// every thread read from LDS or from the call, so it is workgroup-uniform.  No atomics: the same input
// gives the same bits, alone or inside any batch.  The translation unit is built with
// -ffp-contract=off, so a residual is the same number in every pass that classifies with it.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dlt_common.h"
#include "kernels.h"

namespace lg {
namespace {

constexpr int RH_DRAWS = 64;     // a hypothesis whose four indices need more draws is invalid
constexpr int RH_LO_STEPS = 8;

struct RhShared {
  alignas(16) float m[RH_LDS_MATCHES * 4];
  double red[EV_WAVES * 24];
  double jA[81], jV[81];
  double Hkept[9], Hfit[9], Hbest[9];
  unsigned long long key[EV_WAVES];
  int cnt[EV_WAVES];
};

__device__ inline uint64_t mix64(uint64_t z) {  // splitmix64's finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// squared forward transfer error; w == 0 gives inf or NaN, which no threshold accepts
__device__ inline double resid2(const double (&h)[9], double x, double y, double u, double v) {
  const double w = h[6] * x + h[7] * y + h[8];
  const double dx = (h[0] * x + h[1] * y + h[2]) / w - u, dy = (h[3] * x + h[4] * y + h[5]) / w - v;
  return dx * dx + dy * dy;
}

// twice the signed area of the triangle (a, b, c): det [a 1; b 1; c 1]
__device__ inline double det3(double ax, double ay, double bx, double by, double cx, double cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

__device__ inline float4 rh_match(const RhShared& sh, const float4* gm, bool lds, int i) {
  return lds ? reinterpret_cast<const float4*>(sh.m)[i] : gm[i];
}

// Hypothesis t: its four matches, the closed-form model.  False when it is invalid.
__device__ inline bool rh_hypothesis(const RhShared& sh, const float4* gm, bool lds, int K, uint64_t seed_mix, int t,
                                     double min_area, double (&h)[9]) {
  int i0 = -1, i1 = -1, i2 = -1, i3 = -1, n = 0;
  const uint64_t base = seed_mix + ((uint64_t)(uint32_t)t << 16);
  for (int d = 0; d < RH_DRAWS && n < 4; ++d) {
    const int idx = (int)(((mix64(base + (uint64_t)d) >> 32) * (uint64_t)K) >> 32);
    if (idx == i0 || idx == i1 || idx == i2) continue;  // unset ones are -1
    if (n == 0) i0 = idx;
    else if (n == 1) i1 = idx;
    else if (n == 2) i2 = idx;
    else i3 = idx;
    ++n;
  }
  if (n < 4) return false;
  const float4 a = rh_match(sh, gm, lds, i0), b = rh_match(sh, gm, lds, i1), c = rh_match(sh, gm, lds, i2),
               e = rh_match(sh, gm, lds, i3);
  const double px[4] = {a.x, b.x, c.x, e.x}, py[4] = {a.y, b.y, c.y, e.y};
  const double qx[4] = {a.z, b.z, c.z, e.z}, qy[4] = {a.w, b.w, c.w, e.w};
  // p3 = (d0 p0 + d1 p1 + d2 p2) / d3 (Cramer), likewise in image 1
  const double d[4] = {det3(px[3], py[3], px[1], py[1], px[2], py[2]), det3(px[0], py[0], px[3], py[3], px[2], py[2]),
                       det3(px[0], py[0], px[1], py[1], px[3], py[3]), det3(px[0], py[0], px[1], py[1], px[2], py[2])};
  const double g[4] = {det3(qx[3], qy[3], qx[1], qy[1], qx[2], qy[2]), det3(qx[0], qy[0], qx[3], qy[3], qx[2], qy[2]),
                       det3(qx[0], qy[0], qx[1], qy[1], qx[3], qy[3]), det3(qx[0], qy[0], qx[1], qy[1], qx[2], qy[2])};
  int same = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (fabs(d[k]) < min_area || fabs(g[k]) < min_area) return false;
    same += ((d[k] > 0.0) == (g[k] > 0.0)) ? 1 : 0;
  }
  if (same != 0 && same != 4) return false;
  // A = [d0 p0, d1 p1, d2 p2] (columns), B likewise; H = B adj(A), adj(A)'s rows are a1 x a2, a2 x a0, a0 x a1
  double A[3][3], Bm[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    A[k][0] = d[k] * px[k], A[k][1] = d[k] * py[k], A[k][2] = d[k];
    Bm[k][0] = g[k] * qx[k], Bm[k][1] = g[k] * qy[k], Bm[k][2] = g[k];
  }
  double R[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int u = (k + 1) % 3, v = (k + 2) % 3;
    R[k][0] = A[u][1] * A[v][2] - A[u][2] * A[v][1];
    R[k][1] = A[u][2] * A[v][0] - A[u][0] * A[v][2];
    R[k][2] = A[u][0] * A[v][1] - A[u][1] * A[v][0];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) h[3 * i + j] = Bm[0][i] * R[0][j] + Bm[1][i] * R[1][j] + Bm[2][i] * R[2][j];
  return true;
}

// matches within th of the model in every thread's h (the same model), to every thread
__device__ inline int rh_count(RhShared& sh, const float4* gm, bool lds, int K, const double (&h)[9], double t2) {
  double n[1] = {0.0};
  for (int i = threadIdx.x; i < K; i += EV_THREADS) {
    const float4 m = rh_match(sh, gm, lds, i);
    n[0] += resid2(h, m.x, m.y, m.z, m.w) < t2 ? 1.0 : 0.0;
  }
  block_sum(n, sh.red);
  return (int)n[0];
}

// Local optimisation from the model in sh.Hkept with `kept` inliers; returns the kept count, the kept
// model is left in sh.Hkept.  Called by the whole workgroup.
__device__ inline int rh_local_optimisation(RhShared& sh, const float4* gm, bool lds, int K, double th, int kept) {
  const int tid = threadIdx.x;
  const double t2 = th * th;
#pragma nounroll
  for (int s = 0; s < RH_LO_STEPS; ++s) {
    const double mult = s == 0 ? 3.0 : s == 1 ? 2.5 : s == 2 ? 2.0 : s == 3 ? 1.5 : 1.0;
    const double tm = mult * th, tm2 = tm * tm;
    double hk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) hk[k] = sh.Hkept[k];
    // the selected matches' number and the coordinate sums of the two Hartley means
    double acc[5] = {};
    for (int i = tid; i < K; i += EV_THREADS) {
      const float4 m = rh_match(sh, gm, lds, i);
      if (!(resid2(hk, m.x, m.y, m.z, m.w) < tm2)) continue;
      acc[0] += 1.0, acc[1] += m.x, acc[2] += m.y, acc[3] += m.z, acc[4] += m.w;
    }
    block_sum(acc, sh.red);
    const double n = acc[0];
    if (n < 4.0) break;  // too few to fit: the optimisation ends with what it kept
    const double m0x = acc[1] / n, m0y = acc[2] / n, m1x = acc[3] / n, m1y = acc[4] / n;
    double dist[2] = {};
    for (int i = tid; i < K; i += EV_THREADS) {
      const float4 m = rh_match(sh, gm, lds, i);
      if (!(resid2(hk, m.x, m.y, m.z, m.w) < tm2)) continue;
      const double ax = m.x - m0x, ay = m.y - m0y, bx = m.z - m1x, by = m.w - m1y;
      dist[0] += sqrt(ax * ax + ay * ay);
      dist[1] += sqrt(bx * bx + by * by);
    }
    block_sum(dist, sh.red);
    const double s0 = 1.4142135623730951 / (dist[0] / n + 1e-8), s1 = 1.4142135623730951 / (dist[1] / n + 1e-8);
    double S[24] = {};
    for (int i = tid; i < K; i += EV_THREADS) {
      const float4 m = rh_match(sh, gm, lds, i);
      if (!(resid2(hk, m.x, m.y, m.z, m.w) < tm2)) continue;
      dlt_accumulate(S, s0 * (m.x - m0x), s0 * (m.y - m0y), s1 * (m.z - m1x), s1 * (m.w - m1y), 1.0);
    }
    block_sum(S, sh.red);
    dlt_build_system(S, sh.red, sh.jA, sh.jV);
    if (tid < 64) {
      jacobi9(sh.jA, sh.jV, tid);
      wave_sync();
      double G[9];
      dlt_solution(sh.jA, sh.jV, s0, m0x, m0y, s1, m1x, m1y, G);
      if (tid == 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) sh.Hfit[k] = G[k];
    }
    __syncthreads();
    double hf[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) hf[k] = sh.Hfit[k];
    const int cf = rh_count(sh, gm, lds, K, hf, t2);
    if (cf >= kept) {
      kept = cf;
      __syncthreads();  // every thread has read Hkept
      if (tid < 9) sh.Hkept[tid] = sh.Hfit[tid];
      __syncthreads();
    }
  }
  return kept;
}

struct RhState {
  int best_min, best_t, best_lo, rounds, valid;
};

__device__ inline void rh_rounds(RhShared& sh, const float4* gm, bool lds, int K, double th, int max_iters, double min_area,
                                 double log_fail, uint64_t seed, RhState& st) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double t2 = th * th;
  const uint64_t seed_mix = mix64(seed);
  for (int r = 0;; ++r) {
    const int t = r * EV_THREADS + tid;
    double h[9] = {};
    int count = -1;
    if (t < max_iters && rh_hypothesis(sh, gm, lds, K, seed_mix, t, min_area, h)) {
      count = 0;
      for (int i = 0; i < K; ++i) {  // division-free form of resid2 < t2
        const float4 m = rh_match(sh, gm, lds, i);
        const double x = m.x, y = m.y, u = m.z, v = m.w;
        const double w = h[6] * x + h[7] * y + h[8];
        const double ex = (h[0] * x + h[1] * y + h[2]) - u * w, ey = (h[3] * x + h[4] * y + h[5]) - v * w;
        count += ex * ex + ey * ey < t2 * (w * w) ? 1 : 0;
      }
    }
    // the round's best: highest count, then lowest t
    unsigned long long key = count >= 0 ? ((unsigned long long)(count + 1) << 32) | (0xFFFFFFFFu - (unsigned)t) : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(key, off, 64);
      key = o > key ? o : key;
    }
    const int nvalid = __popcll(__ballot(count >= 0));
    if (lane == 0) sh.key[wave] = key, sh.cnt[wave] = nvalid;
    __syncthreads();
    unsigned long long kmax = sh.key[0];
    int vsum = sh.cnt[0];
#pragma unroll
    for (int w = 1; w < EV_WAVES; ++w) {
      kmax = sh.key[w] > kmax ? sh.key[w] : kmax;
      vsum += sh.cnt[w];
    }
    st.valid += vsum;
    st.rounds = r + 1;
    const int done = min((r + 1) * EV_THREADS, max_iters);
    const int rc = (int)(kmax >> 32) - 1, rt = (int)(0xFFFFFFFFu - (unsigned)(kmax & 0xFFFFFFFFull));
    if (kmax != 0ull && rc > st.best_min) {
      st.best_min = rc, st.best_t = rt;
      if (t == rt)
#pragma unroll
        for (int k = 0; k < 9; ++k) sh.Hkept[k] = h[k];
      __syncthreads();
      const int kept = rh_local_optimisation(sh, gm, lds, K, th, rc);
      if (kept > st.best_lo) {
        st.best_lo = kept;
        if (tid < 9) sh.Hbest[tid] = sh.Hkept[tid];
      }
    }
    __syncthreads();  // key, cnt and Hkept are free again; Hbest is visible
    if (done >= max_iters) break;
    if (st.best_lo >= 4) {
      const double q = (double)st.best_lo / (double)K;
      if ((double)done * log1p(-(q * q * q * q)) <= log_fail) break;
    }
  }
}

// Phase 0 and the rounds of pair b: its live matches, in slot order, into m_kpts[b][0 .. K), then the
// search.  Returns K.  Nothing of this outlives the call but K and st, so that the per-pair pointers
// are not held in scalar registers through the rounds for the result phase.
__device__ inline int rh_search(const RansacCall& c, RhShared& sh, int b, RhState& st) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int K = 0;
  const int M = c.M, N = c.N;
  int n0 = M, n1 = N;
  if (c.num0) {  // a ragged batch: slots past the counts are padding, whatever they hold
    n0 = min(max(c.num0[b], 0), M);
    n1 = min(max(c.num1[b], 0), N);
  }
  const float* kp0 = c.kp0 + (int64_t)b * M * 2;
  const float* kp1 = c.kp1 + (int64_t)b * N * 2;
  const int64_t* m0 = c.m0 ? c.m0 + (int64_t)b * M : nullptr;
  float4* gm = reinterpret_cast<float4*>(c.m_kpts) + (int64_t)b * M;
  const double th = c.th[b];

  for (int64_t base = 0; base < n0; base += EV_THREADS) {
    const int64_t i = base + tid;
    int64_t j = -1;
    if (i < n0) j = m0 ? m0[i] : i;
    const bool live = j >= 0 && j < n1;
    const unsigned long long bal = __ballot(live);
    if (lane == 0) sh.cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = K + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) {
      const int cw = sh.cnt[w];
      off += w < wave ? cw : 0;
      K += cw;
    }
    if (live) gm[off] = make_float4(kp0[2 * i], kp0[2 * i + 1], kp1[2 * j], kp1[2 * j + 1]);
    __syncthreads();  // cnt is free again; the rows are visible to the workgroup
  }
  const bool lds = K <= RH_LDS_MATCHES;
  if (lds)
    for (int i = tid; i < K; i += EV_THREADS) reinterpret_cast<float4*>(sh.m)[i] = gm[i];
  __syncthreads();

  if (K >= 4) rh_rounds(sh, gm, lds, K, th, c.max_iters, c.min_area, c.log_fail, c.seed, st);
  return K;
}

__global__ __launch_bounds__(EV_THREADS) void ransac_homography_kernel(const RansacCall c) {
  __shared__ RhShared sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  RhState st = {-1, -1, -1, 0, 0};
  const int K = rh_search(c, sh, b, st);

  // ---- result: the kept model over h33, rounded to fp32; the mask is that matrix's own.  The call's
  // arguments are read again from the kernel-argument segment behind a compiler barrier: loaded at
  // entry they would sit in scalar registers through the rounds and be parked in vector lanes
  const __attribute__((address_space(4))) RansacCall* late =
      (const __attribute__((address_space(4))) RansacCall*)__builtin_amdgcn_kernarg_segment_ptr();  // c lies at offset 0
  asm volatile("" : "+s"(late));
  const int M = late->M, N = late->N;
  int n0 = M, n1 = N;
  if (late->num0) {
    n0 = min(max(late->num0[b], 0), M);
    n1 = min(max(late->num1[b], 0), N);
  }
  const float* kp0 = late->kp0 + (int64_t)b * M * 2;
  const float* kp1 = late->kp1 + (int64_t)b * N * 2;
  const int64_t* m0 = late->m0 ? late->m0 + (int64_t)b * M : nullptr;
  const double th = late->th[b];
  bool success = st.best_lo >= 0;
  float hf[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (success) {
    double hb[9], big = 0.0;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) hb[k] = sh.Hbest[k], big = fmax(big, fabs(hb[k])), finite = finite && isfinite(hb[k]);
    if (!finite || !(fabs(hb[8]) > 1e-12 * big)) success = false;
    else
#pragma unroll
      for (int k = 0; k < 9; ++k) hf[k] = (float)(hb[k] / hb[8]);
  }
  double hd[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) hd[k] = hf[k];
  const double t2 = th * th;
  int ninl = 0;
  if (success) {  // uniform
    double cnt[1] = {0.0};
    for (int64_t i = tid; i < n0; i += EV_THREADS) {
      const int64_t j = m0 ? m0[i] : i;
      if (j < 0 || j >= n1) continue;
      cnt[0] += resid2(hd, kp0[2 * i], kp0[2 * i + 1], kp1[2 * j], kp1[2 * j + 1]) < t2 ? 1.0 : 0.0;
    }
    block_sum(cnt, sh.red);
    ninl = (int)cnt[0];
    if (ninl < 4) success = false;
  }
  uint8_t* inl = late->inliers + (int64_t)b * M;
  for (int64_t i = tid; i < M; i += EV_THREADS) {
    bool in = false;
    if (success && i < n0) {
      const int64_t j = m0 ? m0[i] : i;
      if (j >= 0 && j < n1) in = resid2(hd, kp0[2 * i], kp0[2 * i + 1], kp1[2 * j], kp1[2 * j + 1]) < t2;
    }
    inl[i] = in ? 1 : 0;
  }
  if (tid == 0) {
    float* Ho = late->H + (int64_t)b * 9;
    const float eye[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
#pragma unroll
    for (int k = 0; k < 9; ++k) Ho[k] = success ? hf[k] : eye[k];
    int* o = late->info + (int64_t)b * 8;
    o[0] = success ? 1 : 0, o[1] = K, o[2] = success ? ninl : 0, o[3] = st.best_t, o[4] = max(st.best_min, 0);
    o[5] = st.rounds, o[6] = st.valid, o[7] = 0;
    if (late->H_err) {
      float e = INFINITY;
      if (success) {
        double Hg[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Hg[k] = late->H_gt[(int64_t)b * 9 + k];
        e = (float)corner_error(Hg, hd, (double)late->size0[(int64_t)b * 2], (double)late->size0[(int64_t)b * 2 + 1]);
      }
      late->H_err[b] = e;
    }
  }
}

}  // namespace

hipError_t ransac_homography(const RansacCall& c, hipStream_t st) {
  hipLaunchKernelGGL(ransac_homography_kernel, dim3(c.B), dim3(EV_THREADS), 0, st, c);
  return hipGetLastError();
}

}  // namespace lg
