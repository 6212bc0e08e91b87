// Batched hybrid LO-RANSAC for homographies from point and line matches (include/lightglue_mi355x.h:
// lg_ransac_homography_lines): what the reference's PointLineHomographyEstimator does
// for gluefactory/eval/utils.py:132-173 with lines, one workgroup of 256 threads per pair and one
// launch per batch.
//
//   phase 0   the pair's live point matches and live line matches are compacted in slot order into
//             m_kpts and m_lines (a ballot prefix scan each, no atomics); one similarity per image is
//             fixed from all of them (points and both endpoints of every line); what fits is staged in
//             LDS already normalised, a point as (x, y, u, v), a line as its image-0 endpoints and the
//             (a, b, c) of its image-1 segment, so that no hypothesis takes a square root
//   rounds    256 hypotheses at a time, one per thread: a counter-based sample of four features (two
//             points with two lines is rejected), the 8x9 system in a per-thread private array, its
//             null vector by Gauss-Jordan with complete pivoting, and the inlier count against every
//             feature (all lanes read the same LDS row, a broadcast); the round's best is a workgroup
//             argmax
//   LO        after a round that raised the best minimal count: 8 unweighted DLT refits in the fixed
//             frame with shrinking thresholds, by the whole workgroup (45 sums, jacobi9 of dlt_common.h)
//   result    the kept model taken out of the frame, over h33 in fp32, and the two masks that matrix
//             gives in fp64 on the pixel coordinates
//
// All arithmetic is fp64 on the fp32 inputs.  Every branch that reaches a barrier is taken on values
// every thread read from LDS or from the call, so it is workgroup-uniform.  No atomics: the same input
// gives the same bits, alone or inside any batch.  A feature read from global memory is normalised by
// the same expressions that staged it, and the translation unit is built with -ffp-contract=off, so
// the LDS and the global-memory routes give the same numbers.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dlt_common.h"
#include "kernels.h"

namespace lg {
namespace {

constexpr int RL_DRAWS = 64;  // a hypothesis whose four indices need more draws is invalid
constexpr int RL_LO_STEPS = 8;
constexpr double RL_FLOOR = 1e-12;  // relative: a smaller pivot rejects the sample

struct RlShared {
  double pt[RL_LDS_POINTS * 4];  // x, y, u, v
  double ln[RL_LDS_LINES * 7];   // ax, ay, bx, by (image 0), a, b, c (image 1)
  double red[EV_WAVES * 46];
  double jA[81], jV[81];
  double Hkept[9], Hfit[9], Hbest[9];
  unsigned long long key[EV_WAVES];
  int cnt[EV_WAVES];
};
static_assert(sizeof(RlShared) <= 64 * 1024, "the static LDS of a workgroup");

struct RlFrame {  // T x = s (x - m), per image
  double m0x, m0y, s0, m1x, m1y, s1;
};
struct RlPt {
  double x, y, u, v;
};
struct RlLn {
  double ax, ay, bx, by, a, b, c;
};
// where a pair's features are read from: LDS when the set fits, else its compacted rows
struct RlSrc {
  const float4* gp;  // m_kpts rows
  const float4* gl;  // m_lines rows, two float4 each
  bool pt_lds, ln_lds;
  int Kp, Kl;
};

__device__ inline uint64_t rl_mix64(uint64_t z) {  // splitmix64's finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The line through a segment: unit normal (a, b) and c.  The endpoints are taken in lexicographic
// order, so that their order in the input cannot move a bit.  A zero-length segment gives NaN.
__device__ inline void rl_segment_line(double xa, double ya, double xb, double yb, double& a, double& b, double& c) {
  if (xa > xb || (xa == xb && ya > yb)) {
    const double tx = xa, ty = ya;
    xa = xb, ya = yb, xb = tx, yb = ty;
  }
  const double nx = ya - yb, ny = xb - xa;
  const double n = sqrt(nx * nx + ny * ny);
  a = nx / n, b = ny / n;
  c = -(a * xa + b * ya);
}

__device__ inline RlPt rl_normalise_point(const float4 m, const RlFrame& f) {
  return {f.s0 * (m.x - f.m0x), f.s0 * (m.y - f.m0y), f.s1 * (m.z - f.m1x), f.s1 * (m.w - f.m1y)};
}

__device__ inline RlLn rl_normalise_line(const float4 e0, const float4 e1, const RlFrame& f) {
  RlLn l;
  l.ax = f.s0 * (e0.x - f.m0x), l.ay = f.s0 * (e0.y - f.m0y), l.bx = f.s0 * (e0.z - f.m0x), l.by = f.s0 * (e0.w - f.m0y);
  rl_segment_line(f.s1 * (e1.x - f.m1x), f.s1 * (e1.y - f.m1y), f.s1 * (e1.z - f.m1x), f.s1 * (e1.w - f.m1y), l.a, l.b, l.c);
  return l;
}

__device__ inline RlPt rl_point(const RlShared& sh, const RlSrc& s, const RlFrame& f, int i) {
  if (s.pt_lds) return {sh.pt[4 * i], sh.pt[4 * i + 1], sh.pt[4 * i + 2], sh.pt[4 * i + 3]};
  return rl_normalise_point(s.gp[i], f);
}

__device__ inline RlLn rl_line(const RlShared& sh, const RlSrc& s, const RlFrame& f, int i) {
  if (s.ln_lds) {
    const double* r = sh.ln + 7 * i;
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
  }
  return rl_normalise_line(s.gl[2 * i], s.gl[2 * i + 1], f);
}

// forward transfer error below t, division-free; w == 0 or a non-finite value is an outlier
__device__ inline bool rl_point_in(const double (&h)[9], const RlPt& p, double t2) {
  const double w = h[6] * p.x + h[7] * p.y + h[8];
  const double ex = (h[0] * p.x + h[1] * p.y + h[2]) - p.u * w, ey = (h[3] * p.x + h[4] * p.y + h[5]) - p.v * w;
  return ex * ex + ey * ey < t2 * (w * w);
}

// both mapped image-0 endpoints within t of the image-1 line
__device__ inline bool rl_line_in(const double (&h)[9], const RlLn& l, double t2) {
  const double wa = h[6] * l.ax + h[7] * l.ay + h[8], wb = h[6] * l.bx + h[7] * l.by + h[8];
  const double ea = l.a * (h[0] * l.ax + h[1] * l.ay + h[2]) + l.b * (h[3] * l.ax + h[4] * l.ay + h[5]) + l.c * wa;
  const double eb = l.a * (h[0] * l.bx + h[1] * l.by + h[2]) + l.b * (h[3] * l.bx + h[4] * l.by + h[5]) + l.c * wb;
  return (ea * ea < t2 * (wa * wa)) && (eb * eb < t2 * (wb * wb));
}

__device__ inline void rl_point_rows(const RlPt& p, double (&r0)[9], double (&r1)[9]) {
  r0[0] = 0.0, r0[1] = 0.0, r0[2] = 0.0, r0[3] = -p.x, r0[4] = -p.y, r0[5] = -1.0;
  r0[6] = p.v * p.x, r0[7] = p.v * p.y, r0[8] = p.v;
  r1[0] = p.x, r1[1] = p.y, r1[2] = 1.0, r1[3] = 0.0, r1[4] = 0.0, r1[5] = 0.0;
  r1[6] = -p.u * p.x, r1[7] = -p.u * p.y, r1[8] = -p.u;
}

// H p lies on the image-1 line, for the endpoints a0 and b0
__device__ inline void rl_line_rows(const RlLn& l, double (&r0)[9], double (&r1)[9]) {
  r0[0] = l.a * l.ax, r0[1] = l.a * l.ay, r0[2] = l.a, r0[3] = l.b * l.ax, r0[4] = l.b * l.ay, r0[5] = l.b;
  r0[6] = l.c * l.ax, r0[7] = l.c * l.ay, r0[8] = l.c;
  r1[0] = l.a * l.bx, r1[1] = l.a * l.by, r1[2] = l.a, r1[3] = l.b * l.bx, r1[4] = l.b * l.by, r1[5] = l.b;
  r1[6] = l.c * l.bx, r1[7] = l.c * l.by, r1[8] = l.c;
}

// The null vector of the 8x9 system by Gauss-Jordan with complete pivoting: 1 on the free column,
// minus the reduced entries elsewhere.  False when a pivot is not above the floor.
__device__ inline bool rl_null_vector(double (&A)[8][9], double (&h)[9]) {
  double scale = 0.0;
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 9; ++k) scale = fmax(scale, fabs(A[i][k]));
  unsigned long long rows = 0;  // nibble c: the row whose pivot stands in column c
  unsigned used = 0;
  for (int s = 0; s < 8; ++s) {
    int br = s, bc = 0;
    double bm = -1.0;
    for (int r = s; r < 8; ++r)
      for (int c = 0; c < 9; ++c) {
        const double a = (used >> c & 1u) ? -1.0 : fabs(A[r][c]);
        if (a > bm) bm = a, br = r, bc = c;  // the first maximum in row-major order
      }
    const double piv = A[br][bc];
    if (!(fabs(piv) > RL_FLOOR * scale)) return false;
    for (int k = 0; k < 9; ++k) {
      const double a = A[s][k];
      A[s][k] = A[br][k], A[br][k] = a;
    }
    for (int k = 0; k < 9; ++k) A[s][k] = A[s][k] / piv;
    for (int i = 0; i < 8; ++i) {
      if (i == s) continue;
      const double f = A[i][bc];
      for (int k = 0; k < 9; ++k) A[i][k] = A[i][k] - f * A[s][k];
    }
    used |= 1u << bc;
    rows |= (unsigned long long)s << (4 * bc);
  }
  const int free = __builtin_ctz(~used & 0x1FFu);
#pragma unroll
  for (int c = 0; c < 9; ++c) h[c] = c == free ? 1.0 : -A[(int)(rows >> (4 * c)) & 15][free];
  return true;
}

// Hypothesis t: its four features, the system in sample order, the model.  False when it is invalid.
__device__ inline bool rl_hypothesis(const RlShared& sh, const RlSrc& src, const RlFrame& f, uint64_t seed_mix, int t,
                                     double (&h)[9]) {
  const int K = src.Kp + src.Kl;
  int ix[4] = {-1, -1, -1, -1}, n = 0;  // statically indexed throughout: registers
  const uint64_t base = seed_mix + ((uint64_t)(uint32_t)t << 16);
  for (int d = 0; d < RL_DRAWS && n < 4; ++d) {
    const int idx = (int)(((rl_mix64(base + (uint64_t)d) >> 32) * (uint64_t)K) >> 32);
    if (idx == ix[0] || idx == ix[1] || idx == ix[2]) continue;  // unset ones are -1
    if (n == 0) ix[0] = idx;
    else if (n == 1) ix[1] = idx;
    else if (n == 2) ix[2] = idx;
    else ix[3] = idx;
    ++n;
  }
  if (n < 4) return false;
  int npts = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) npts += ix[k] < src.Kp ? 1 : 0;
  if (npts == 2) return false;  // two points and two lines do not fix a homography
  double A[8][9];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double r0[9], r1[9];
    if (ix[k] < src.Kp) rl_point_rows(rl_point(sh, src, f, ix[k]), r0, r1);
    else rl_line_rows(rl_line(sh, src, f, ix[k] - src.Kp), r0, r1);
#pragma unroll
    for (int e = 0; e < 9; ++e) A[2 * k][e] = r0[e], A[2 * k + 1][e] = r1[e];
  }
  return rl_null_vector(A, h);
}

// features within t of the model in every thread's h (the same model), to every thread
__device__ inline int rl_count(RlShared& sh, const RlSrc& src, const RlFrame& f, const double (&h)[9], double t2) {
  double n[1] = {0.0};
  for (int i = threadIdx.x; i < src.Kp; i += EV_THREADS) n[0] += rl_point_in(h, rl_point(sh, src, f, i), t2) ? 1.0 : 0.0;
  for (int i = threadIdx.x; i < src.Kl; i += EV_THREADS) n[0] += rl_line_in(h, rl_line(sh, src, f, i), t2) ? 1.0 : 0.0;
  block_sum(n, sh.red);
  return (int)n[0];
}

// a DLT row's share of the upper triangle of A^T A
__device__ inline void rl_accumulate(double (&S)[46], const double (&r)[9]) {
  int o = 0;
#pragma unroll
  for (int a = 0; a < 9; ++a)
#pragma unroll
    for (int b = a; b < 9; ++b) S[o++] += r[a] * r[b];
}

// Local optimisation from the model in sh.Hkept with `kept` inliers; returns the kept count, the kept
// model is left in sh.Hkept.  Called by the whole workgroup.
__device__ inline int rl_local_optimisation(RlShared& sh, const RlSrc& src, const RlFrame& f, double th, int kept) {
  const int tid = threadIdx.x;
  const double t2 = th * th;
#pragma nounroll
  for (int s = 0; s < RL_LO_STEPS; ++s) {
    const double mult = s == 0 ? 3.0 : s == 1 ? 2.5 : s == 2 ? 2.0 : s == 3 ? 1.5 : 1.0;
    const double tm = mult * th, tm2 = tm * tm;
    double hk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) hk[k] = sh.Hkept[k];
    // the upper triangle of A^T A over the selected features' rows; S[45] is their number
    double S[46] = {};
    for (int i = tid; i < src.Kp; i += EV_THREADS) {
      const RlPt p = rl_point(sh, src, f, i);
      if (!rl_point_in(hk, p, tm2)) continue;
      double r0[9], r1[9];
      rl_point_rows(p, r0, r1);
      rl_accumulate(S, r0), rl_accumulate(S, r1);
      S[45] += 1.0;
    }
    for (int i = tid; i < src.Kl; i += EV_THREADS) {
      const RlLn l = rl_line(sh, src, f, i);
      if (!rl_line_in(hk, l, tm2)) continue;
      double r0[9], r1[9];
      rl_line_rows(l, r0, r1);
      rl_accumulate(S, r0), rl_accumulate(S, r1);
      S[45] += 1.0;
    }
    block_sum(S, sh.red);
    if (S[45] < 4.0) break;  // too few to fit: the optimisation ends with what it kept
    __syncthreads();         // every thread has read the partials
    if (tid == 0)
#pragma unroll
      for (int k = 0; k < 45; ++k) sh.red[k] = S[k];
    __syncthreads();
    if (tid < 81) {
      const int a = min(tid / 9, tid % 9), b = max(tid / 9, tid % 9);
      sh.jA[tid] = sh.red[a * 9 - a * (a - 1) / 2 + (b - a)];
      sh.jV[tid] = tid / 9 == tid % 9 ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
      jacobi9(sh.jA, sh.jV, tid);
      wave_sync();
      if (tid == 0) {
        int best = 0;
        double ev = sh.jA[0];
        for (int k = 1; k < 9; ++k)
          if (sh.jA[k * 9 + k] < ev) ev = sh.jA[k * 9 + k], best = k;
        for (int k = 0; k < 9; ++k) sh.Hfit[k] = sh.jV[k * 9 + best];
      }
    }
    __syncthreads();
    double hf[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) hf[k] = sh.Hfit[k];
    const int cf = rl_count(sh, src, f, hf, t2);
    if (cf >= kept) {
      kept = cf;
      __syncthreads();  // every thread has read Hkept
      if (tid < 9) sh.Hkept[tid] = sh.Hfit[tid];
      __syncthreads();
    }
  }
  return kept;
}

struct RlState {
  int best_min, best_t, best_lo, rounds, valid;
};

__device__ inline void rl_rounds(RlShared& sh, const RlSrc& src, const RlFrame& f, double th, int max_iters, double log_fail,
                                 uint64_t seed, RlState& st) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = src.Kp + src.Kl;
  const double t2 = th * th;
  const uint64_t seed_mix = rl_mix64(seed);
  for (int r = 0;; ++r) {
    const int t = r * EV_THREADS + tid;
    double h[9] = {};
    int count = -1;
    if (t < max_iters && rl_hypothesis(sh, src, f, seed_mix, t, h)) {
      count = 0;
      for (int i = 0; i < src.Kp; ++i) count += rl_point_in(h, rl_point(sh, src, f, i), t2) ? 1 : 0;
      for (int i = 0; i < src.Kl; ++i) count += rl_line_in(h, rl_line(sh, src, f, i), t2) ? 1 : 0;
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
      const int kept = rl_local_optimisation(sh, src, f, th, rc);
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

// slot i's matched point of pair-local arrays, when it is live
__device__ inline bool rl_live_point(const int64_t* m0, int64_t i, int n0, int n1, int64_t& j) {
  j = -1;
  if (i < n0) j = m0 ? m0[i] : i;
  return j >= 0 && j < n1;
}

// slot i's matched line, when it is live: a match inside the counts and both segments long enough
__device__ inline bool rl_live_line(const float4* ln0, const float4* ln1, const int64_t* lm0, int64_t i, int n0, int n1,
                                    double min_len2, float4& e0, float4& e1) {
  int64_t j = -1;
  if (i < n0) j = lm0 ? lm0[i] : i;
  if (!(j >= 0 && j < n1)) return false;
  e0 = ln0[i], e1 = ln1[j];
  const double dx0 = (double)e0.x - (double)e0.z, dy0 = (double)e0.y - (double)e0.w;
  const double dx1 = (double)e1.x - (double)e1.z, dy1 = (double)e1.y - (double)e1.w;
  return dx0 * dx0 + dy0 * dy0 >= min_len2 && dx1 * dx1 + dy1 * dy1 >= min_len2;
}

// `live` of every thread's slot -> its place in the compacted order; K moves on by the block's count
__device__ inline int rl_compact_offset(RlShared& sh, bool live, int& K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
  return off;
}

// Pair b's view of the call: its arrays, counts and threshold.  P points to the call, in whichever
// address space the caller read it from.
struct RlPair {
  int M, L0, n0, n1, nl0, nl1;
  const float *kp0, *kp1;
  const int64_t* m0;
  const float4 *ln0, *ln1;
  const int64_t* lm0;
  float4 *gp, *gl;  // m_kpts rows; m_lines rows, two float4 each
  double th;
};

template <class P>
__device__ inline RlPair rl_pair(P c, int b) {
  RlPair p;
  const int M = c->M, N = c->N, L0 = c->L0, L1 = c->L1;
  p.M = M, p.L0 = L0, p.n0 = M, p.n1 = N, p.nl0 = L0, p.nl1 = L1;
  if (c->num0) {  // a ragged batch: slots past the counts are padding, whatever they hold
    p.n0 = min(max(c->num0[b], 0), M);
    p.n1 = min(max(c->num1[b], 0), N);
  }
  if (c->nl0) {
    p.nl0 = min(max(c->nl0[b], 0), L0);
    p.nl1 = min(max(c->nl1[b], 0), L1);
  }
  p.kp0 = c->kp0 + (int64_t)b * M * 2;
  p.kp1 = c->kp1 + (int64_t)b * N * 2;
  p.m0 = c->m0 ? c->m0 + (int64_t)b * M : nullptr;
  p.ln0 = reinterpret_cast<const float4*>(c->ln0) + (int64_t)b * L0;
  p.ln1 = reinterpret_cast<const float4*>(c->ln1) + (int64_t)b * L1;
  p.lm0 = c->lm0 ? c->lm0 + (int64_t)b * L0 : nullptr;
  p.gp = reinterpret_cast<float4*>(c->m_kpts) + (int64_t)b * M;
  p.gl = reinterpret_cast<float4*>(c->m_lines) + (int64_t)b * L0 * 2;
  p.th = c->th[b];
  return p;
}

// Phase 0, the frames and the rounds of pair b.  Nothing of this outlives the call but the counts, the
// frames and st, so that the per-pair pointers are not held in scalar registers through the rounds for
// the result phase.
__device__ inline void rl_search(const RansacLinesCall& c, RlShared& sh, int b, RlState& st, RlFrame& f, int& Kp, int& Kl) {
  const int tid = threadIdx.x;
  const RlPair q = rl_pair(&c, b);
  float4 *gp = q.gp, *gl = q.gl;

  // ---- phase 0: the live points, then the live lines, in slot order
  for (int64_t base = 0; base < q.n0; base += EV_THREADS) {
    const int64_t i = base + tid;
    int64_t j;
    const bool live = rl_live_point(q.m0, i, q.n0, q.n1, j);
    const int off = rl_compact_offset(sh, live, Kp);
    if (live) gp[off] = make_float4(q.kp0[2 * i], q.kp0[2 * i + 1], q.kp1[2 * j], q.kp1[2 * j + 1]);
    __syncthreads();  // cnt is free again; the rows are visible to the workgroup
  }
  for (int64_t base = 0; base < q.nl0; base += EV_THREADS) {
    const int64_t i = base + tid;
    float4 e0, e1;
    const bool live = rl_live_line(q.ln0, q.ln1, q.lm0, i, q.nl0, q.nl1, c.min_len2, e0, e1);
    const int off = rl_compact_offset(sh, live, Kl);
    if (live) gl[2 * off] = e0, gl[2 * off + 1] = e1;
    __syncthreads();
  }
  if (Kp + Kl < 4) return;  // uniform
  const RlSrc src = {gp, gl, Kp <= RL_LDS_POINTS, Kl <= RL_LDS_LINES, Kp, Kl};
  // the frames: mean and mean distance over the points and both endpoints of every line; a line's
  // two endpoints enter as one sum, so that their order cannot move a bit
  double acc[4] = {};
  for (int i = tid; i < Kp; i += EV_THREADS) {
    const float4 m = gp[i];
    acc[0] += m.x, acc[1] += m.y, acc[2] += m.z, acc[3] += m.w;
  }
  for (int i = tid; i < Kl; i += EV_THREADS) {
    const float4 e0 = gl[2 * i], e1 = gl[2 * i + 1];
    acc[0] += (double)e0.x + (double)e0.z, acc[1] += (double)e0.y + (double)e0.w;
    acc[2] += (double)e1.x + (double)e1.z, acc[3] += (double)e1.y + (double)e1.w;
  }
  block_sum(acc, sh.red);
  const double n = (double)Kp + 2.0 * (double)Kl;
  f.m0x = acc[0] / n, f.m0y = acc[1] / n, f.m1x = acc[2] / n, f.m1y = acc[3] / n;
  double dist[2] = {};
  for (int i = tid; i < Kp; i += EV_THREADS) {
    const float4 m = gp[i];
    const double ax = m.x - f.m0x, ay = m.y - f.m0y, bx = m.z - f.m1x, by = m.w - f.m1y;
    dist[0] += sqrt(ax * ax + ay * ay);
    dist[1] += sqrt(bx * bx + by * by);
  }
  for (int i = tid; i < Kl; i += EV_THREADS) {
    const float4 e0 = gl[2 * i], e1 = gl[2 * i + 1];
    const double ax = e0.x - f.m0x, ay = e0.y - f.m0y, bx = e0.z - f.m0x, by = e0.w - f.m0y;
    const double cx = e1.x - f.m1x, cy = e1.y - f.m1y, dx = e1.z - f.m1x, dy = e1.w - f.m1y;
    dist[0] += sqrt(ax * ax + ay * ay) + sqrt(bx * bx + by * by);
    dist[1] += sqrt(cx * cx + cy * cy) + sqrt(dx * dx + dy * dy);
  }
  block_sum(dist, sh.red);
  f.s0 = 1.4142135623730951 / (dist[0] / n + 1e-8), f.s1 = 1.4142135623730951 / (dist[1] / n + 1e-8);
  if (src.pt_lds)
    for (int i = tid; i < Kp; i += EV_THREADS) {
      const RlPt p = rl_normalise_point(gp[i], f);
      sh.pt[4 * i] = p.x, sh.pt[4 * i + 1] = p.y, sh.pt[4 * i + 2] = p.u, sh.pt[4 * i + 3] = p.v;
    }
  if (src.ln_lds)
    for (int i = tid; i < Kl; i += EV_THREADS) {
      const RlLn l = rl_normalise_line(gl[2 * i], gl[2 * i + 1], f);
      double* r = sh.ln + 7 * i;
      r[0] = l.ax, r[1] = l.ay, r[2] = l.bx, r[3] = l.by, r[4] = l.a, r[5] = l.b, r[6] = l.c;
    }
  __syncthreads();
  rl_rounds(sh, src, f, f.s1 * q.th, c.max_iters, c.log_fail, c.seed, st);
}

__global__ __launch_bounds__(EV_THREADS) void ransac_homography_lines_kernel(const RansacLinesCall c) {
  __shared__ RlShared sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  RlState st = {-1, -1, -1, 0, 0};
  RlFrame f = {0.0, 0.0, 1.0, 0.0, 0.0, 1.0};
  int Kp = 0, Kl = 0;
  rl_search(c, sh, b, st, f, Kp, Kl);

  // ---- result.  The call's arguments are read again from the kernel-argument segment behind a
  // compiler barrier: loaded at entry they would sit in scalar registers through the rounds
  const __attribute__((address_space(4))) RansacLinesCall* late =
      (const __attribute__((address_space(4))) RansacLinesCall*)__builtin_amdgcn_kernarg_segment_ptr();  // c lies at offset 0
  asm volatile("" : "+s"(late));
  const RlPair q = rl_pair(late, b);
  const int M = q.M, L0 = q.L0, n0 = q.n0, n1 = q.n1, nl0 = q.nl0, nl1 = q.nl1;
  const float *kp0 = q.kp0, *kp1 = q.kp1;
  const int64_t *m0 = q.m0, *lm0 = q.lm0;
  const float4 *ln0 = q.ln0, *ln1 = q.ln1, *gp = q.gp, *gl = q.gl;
  const double th = q.th, min_len2 = late->min_len2;
  // the kept model out of the frame, over h33, rounded to fp32; the masks are that matrix's
  bool success = st.best_lo >= 0;
  float hf[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (success) {
    double h[9], X[9], hb[9], big = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = sh.Hbest[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {  // h T0, then T1^-1 (h T0)
      X[3 * r] = h[3 * r] * f.s0, X[3 * r + 1] = h[3 * r + 1] * f.s0;
      X[3 * r + 2] = h[3 * r + 2] - f.s0 * (f.m0x * h[3 * r] + f.m0y * h[3 * r + 1]);
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      hb[k] = X[k] / f.s1 + f.m1x * X[6 + k];
      hb[3 + k] = X[3 + k] / f.s1 + f.m1y * X[6 + k];
      hb[6 + k] = X[6 + k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) big = fmax(big, fabs(hb[k])), finite = finite && isfinite(hb[k]);
    if (!finite || !(fabs(hb[8]) > 1e-12 * big)) success = false;
    else
#pragma unroll
      for (int k = 0; k < 9; ++k) hf[k] = (float)(hb[k] / hb[8]);
  }
  double hd[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) hd[k] = hf[k];
  const double t2 = th * th;
  int npi = 0, nli = 0;
  if (success) {  // uniform
    double cnt[2] = {};
    for (int i = tid; i < Kp; i += EV_THREADS) {
      const float4 m = gp[i];
      cnt[0] += rl_point_in(hd, RlPt{m.x, m.y, m.z, m.w}, t2) ? 1.0 : 0.0;
    }
    for (int i = tid; i < Kl; i += EV_THREADS) {
      const float4 e0 = gl[2 * i], e1 = gl[2 * i + 1];
      RlLn l = {e0.x, e0.y, e0.z, e0.w, 0.0, 0.0, 0.0};
      rl_segment_line(e1.x, e1.y, e1.z, e1.w, l.a, l.b, l.c);
      cnt[1] += rl_line_in(hd, l, t2) ? 1.0 : 0.0;
    }
    block_sum(cnt, sh.red);
    npi = (int)cnt[0], nli = (int)cnt[1];
    if (npi + nli < 4) success = false;
  }
  uint8_t* inl = late->inliers + (int64_t)b * M;
  for (int64_t i = tid; i < M; i += EV_THREADS) {
    bool in = false;
    int64_t j;
    if (success && rl_live_point(m0, i, n0, n1, j))
      in = rl_point_in(hd, RlPt{kp0[2 * i], kp0[2 * i + 1], kp1[2 * j], kp1[2 * j + 1]}, t2);
    inl[i] = in ? 1 : 0;
  }
  uint8_t* linl = late->line_inliers + (int64_t)b * L0;
  for (int64_t i = tid; i < L0; i += EV_THREADS) {
    bool in = false;
    float4 e0, e1;
    if (success && rl_live_line(ln0, ln1, lm0, i, nl0, nl1, min_len2, e0, e1)) {
      RlLn l = {e0.x, e0.y, e0.z, e0.w, 0.0, 0.0, 0.0};
      rl_segment_line(e1.x, e1.y, e1.z, e1.w, l.a, l.b, l.c);
      in = rl_line_in(hd, l, t2);
    }
    linl[i] = in ? 1 : 0;
  }
  if (tid == 0) {
    float* Ho = late->H + (int64_t)b * 9;
    const float eye[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
#pragma unroll
    for (int k = 0; k < 9; ++k) Ho[k] = success ? hf[k] : eye[k];
    int* o = late->info + (int64_t)b * 12;
    o[0] = success ? 1 : 0, o[1] = Kp, o[2] = Kl, o[3] = success ? npi : 0, o[4] = success ? nli : 0;
    o[5] = st.best_t, o[6] = max(st.best_min, 0), o[7] = st.rounds, o[8] = st.valid;
    o[9] = 0, o[10] = 0, o[11] = 0;
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

hipError_t ransac_homography_lines(const RansacLinesCall& c, hipStream_t st) {
  hipLaunchKernelGGL(ransac_homography_lines_kernel, dim3(c.B), dim3(EV_THREADS), 0, st, c);
  return hipGetLastError();
}

}  // namespace lg
