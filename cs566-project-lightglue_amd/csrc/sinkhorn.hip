// Log-domain Sinkhorn with a dustbin (gfx950) — superglue.py:173-201 log_optimal_transport.
//
//   Zc = [[scores, alpha], [alpha, alpha]]            [B, M+1, N+1]
//   log_mu = [-log(M+N)] * M ++ [log N - log(M+N)],  log_nu likewise with M
//   iters x { u = log_mu - LSE_j(Zc + v);  v = log_nu - LSE_i(Zc + u) }
//   out = Zc + u + v + log(M+N)
//
// Fused path (N <= 4096, the configs[4] shape): ONE read of the scores per iteration.  A wave
// holds a whole row in registers (lane: columns 256k + 4 lane + e), so the u-step's LSE_j is the
// two-pass max-then-sum of torch.logsumexp without a second read; with u_i known, the same
// registers feed the v-step's column statistics Z_ij + u_i as running (max, sum) pairs per
// column.  The 8 waves of a workgroup (consecutive row runs of one pair) merge their column
// pairs through LDS, one partial per workgroup goes to HBM, and sinkhorn_colmerge_kernel turns
// the partials into v (LSE_i = M + log sum_p s_p e^(m_p - M)).  Order per iteration as in the
// reference: u from the previous v, then v from the new u.
// HBM bound: B*M*N*4 bytes read per iteration (+ partials, ~3%).
// General path (N > 4096): the u-step walks rows of `scores`, the v-step walks rows of a
// transposed copy made once (tiled LDS transpose); one wave per row, two-pass max-then-sum.
// Ragged batches (per-pair row / column counts): separate RAGGED instantiations of every kernel,
// see SkPair below; the uniform instantiations are the code they were without it.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>

#include "common.h"
#include "kernels.h"

#ifndef LG_SK_LOG2
#define LG_SK_LOG2 1  // sinkhorn_scaled_kernel's row pass in log2 units with packed adds / FMAs (VERDICT r3 item 4;
                      // 5.186 -> 5.105 ms at configs[4], two alternating same-box rounds, profiles/r04/sk_log2_ab.log)
#endif
#ifndef LG_SK_NT
#define LG_SK_NT 1  // streaming (non-temporal) score loads in sinkhorn_scaled_kernel: 5.94 -> 5.21 ms at B = 8, N = 4096
#endif

namespace lg {

// A ragged batch (per-pair counts): pair b has m <= M real rows and n <= N real
// columns, stored first; the rest of its [M][N] slot is arbitrary (NaN allowed) and is never used.
// sk_pairs_kernel clamps the caller's counts on the device and derives the pair's own marginals
// (superglue.py:194-197 at the pair's sizes); every kernel below has a RAGGED instantiation that
// reads its pair's entry once, bounds its row / column loops by the counts, and addresses the
// dustbin row / column at the capacity index (u[M], v[N], Z[M][.], Z[.][N]).  The uniform
// instantiations (RAGGED = false) never touch the table.
struct SkPair {
  int m, n;                   // clamped counts; both 0 for a pair with an empty image
  float norm, mu_bin, nu_bin; // -log(m+n), log n + norm (dustbin row), log m + norm (dustbin column)
  int pad[3];
};

// A pair whose counts equal the capacities takes the host's constants (the uniform launch's own
// bits); an empty pair (either count 0: superglue.py:257-264) gets zeros -- nothing of it is used.
__global__ void sk_pairs_kernel(const int* n0, const int* n1, SkPair* pairs, int B, int M, int N, float norm, float mu_bin,
                                float nu_bin) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B) return;
  int a = min(max(n0[t], 0), M), c = min(max(n1[t], 0), N);
  SkPair p{};
  if (a == 0 || c == 0) {
    a = c = 0;
  } else if (a == M && c == N) {
    p.norm = norm; p.mu_bin = mu_bin; p.nu_bin = nu_bin;
  } else {
    const float ms = (float)a, ns = (float)c;
    p.norm = -logf(ms + ns);
    p.mu_bin = logf(ns) + p.norm;
    p.nu_bin = logf(ms) + p.norm;
  }
  p.m = a; p.n = c;
  pairs[t] = p;
}

template <bool RAGGED = false>
__global__ __launch_bounds__(256) void transpose_kernel(const float* src, float* dst, int M, int N,
                                                        const SkPair* pairs = nullptr) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  if constexpr (RAGGED) {  // a tile wholly in the padding: never read back
    if (i0 >= pairs[b].m || j0 >= pairs[b].n) return;
  }
  const float* s = src + (size_t)b * M * N;
  float* d = dst + (size_t)b * M * N;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int i = i0 + r, j = j0 + tx;
    if (i < M && j < N) tile[r][tx] = s[(size_t)i * N + j];
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int j = j0 + r, i = i0 + tx;
    if (i < M && j < N) d[(size_t)j * M + i] = tile[tx][r];
  }
}

// One Sinkhorn half-step over `rows`+1 rows of length `cols`+1 (last row / column = dustbin).
// src: [B][rows][cols] real scores; other: the opposite potential [B][cols+1]; out: [B][rows+1].
// RAGGED: the pair's own row / column counts bound the walk (swapped: src is the transposed copy,
// rows are the pair's columns); position nc of the walk is the dustbin, read at index cols.
template <bool RAGGED = false>
__global__ __launch_bounds__(256) void lse_step_kernel(const float* src, const float* other, float* out, int B, int rows,
                                                       int cols, float alpha, float lm_in, float lm_bin,
                                                       const SkPair* pairs = nullptr, int swapped = 0) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= B * (rows + 1)) return;
  const int b = r / (rows + 1), i = r - b * (rows + 1);
  const float* o = other + (size_t)b * (cols + 1);
  const float* x = src + ((size_t)b * rows + i) * cols;
  const bool bin_row = i == rows;
  int nc = cols;
  if constexpr (RAGGED) {
    const SkPair pr = pairs[b];
    const int nr = swapped ? pr.n : pr.m;
    nc = swapped ? pr.m : pr.n;
    if (i >= nr && !bin_row) return;  // a padded row: no potential
    lm_in = pr.norm;
    lm_bin = swapped ? pr.nu_bin : pr.mu_bin;
  }
  float m = -INFINITY;
  for (int j = lane; j <= nc; j += 64) {
    const float z = (bin_row || j == nc) ? alpha : x[j];
    m = fmaxf(m, z + o[j == nc ? cols : j]);
  }
  m = wave_max(m);
  float s = 0.f;
  for (int j = lane; j <= nc; j += 64) {
    const float z = (bin_row || j == nc) ? alpha : x[j];
    s += expf((z + o[j == nc ? cols : j]) - m);
  }
  s = wave_sum(s);
  if (lane == 0) {
    const float lse = (m == -INFINITY) ? m : m + logf(s);
    out[r] = (bin_row ? lm_bin : lm_in) - lse;
  }
}

// out = Zc + u_i + v_j - norm (superglue.py:199-201): one row per blockIdx.x, 1024 columns per
// blockIdx.y; each load / store instruction covers 256 consecutive columns (coalesced whatever
// the alignment of the N+1-long output rows)
// RAGGED: also the frame of the fixed-shape Z -- real block at i < m, j < n, dustbin column at N
// (i < m), dustbin row at M (j < n), the corner [M][N]; every other entry -inf.  An empty pair:
// -inf except [M][N] = 0.
template <bool RAGGED = false>
__global__ __launch_bounds__(256) void sinkhorn_out_kernel(const float* scores, const float* u, const float* v,
                                                           float* Z, int M, int N, float alpha, float norm,
                                                           const SkPair* pairs = nullptr) {
  const int r = blockIdx.x;  // b * (M + 1) + i
  const int b = r / (M + 1), i = r - b * (M + 1);
  int mr = M, nr = N;
  if constexpr (RAGGED) {
    const SkPair pr = pairs[b];
    mr = pr.m; nr = pr.n; norm = pr.norm;
  }
  const float ui = u[r];
  const float* vb = v + (size_t)b * (N + 1);
  const float* sr = scores + ((size_t)b * M + min(i, M - 1)) * N;
  float* zr = Z + (size_t)r * (N + 1);
  float x[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = blockIdx.y * 1024 + e * 256 + threadIdx.x;
    x[e] = (i < mr && j < nr) ? sr[j] : alpha;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = blockIdx.y * 1024 + e * 256 + threadIdx.x;
    if constexpr (RAGGED) {
      if (j <= N) {
        const bool in = (i < mr || i == M) && (j < nr || j == N);  // empty pair (mr = nr = 0): only [M][N]
        const float z = mr == 0 ? 0.f : ((x[e] + ui) + vb[j]) - norm;
        zr[j] = in ? z : -INFINITY;
      }
    } else {
      if (j <= N) zr[j] = ((x[e] + ui) + vb[j]) - norm;
    }
  }
}


// ---------------------------------------------------------------- fused path (N <= 4096)
namespace {
constexpr int kSkMaxN = 4096;               // real columns held in registers (16 float4 per lane)
constexpr int kSkTargetWG = 256;            // ~one workgroup per CU
#ifndef LG_SINKHORN_SCALED
#define LG_SINKHORN_SCALED 1
#endif
constexpr bool kSkScaled = LG_SINKHORN_SCALED != 0;  // sinkhorn_scaled_kernel first (exact rerun if flagged)

// waves per workgroup: 8, except the exact kernel at 16 chunks per lane, whose row (64) and
// running column pairs (128) do not fit the 256 registers of two waves per SIMD
__host__ __device__ constexpr int sk_waves(int k4, bool exact) { return exact && k4 >= 16 ? 4 : 8; }

struct SkPlan {
  int rw;  // rows per wave
  int p;   // workgroups (partials) per pair
};

SkPlan sk_plan(int B, int M, int N, bool exact) {
  const int w = sk_waves((N + 255) / 256, exact);
  const int rows = M + 1;
  int p = (kSkTargetWG + B - 1) / B;
  p = std::max(1, std::min(p, (rows + w - 1) / w));
  const int rb = (rows + p - 1) / p;
  const int rw = (rb + w - 1) / w;
  return {rw, (rows + w * rw - 1) / (w * rw)};
}

bool sk_fused_ok(int M, int N) { return M > 0 && N > 0 && N <= kSkMaxN; }

// merge running (max, sum) pair b into a: sum of e^(x - max) over the union
__device__ __forceinline__ void lse_merge(float& am, float& as, float bm, float bs) {
  const float m = fmaxf(am, bm);
  const float ea = am == m ? 1.f : __expf(am - m);
  const float eb = bm == m ? 1.f : __expf(bm - m);
  as = as * ea + bs * eb;
  am = m;
}
}  // namespace

// One iteration: u <- log_mu - LSE_j(Zc + v) for the workgroup's rows, then this workgroup's
// column partials of Zc + u.  K4 = float4 column chunks per lane (columns 256k + 4 lane + e);
// VEC: rows are 16-byte aligned (N % 4 == 0).
// RAGGED (PF = false only): Mr / Nr are the pair's counts -- columns >= Nr are masked like the
// columns >= N of the uniform kernel, rows in [Mr, M) are skipped, the dustbin row stays row M.  A
// workgroup whose rows are all padding writes neutral partials (-inf, 0) and leaves.
template <int K4, bool VEC, int W, bool PF = false, bool RAGGED = false>
__global__ __launch_bounds__(W * 64) void sinkhorn_fused_kernel(const float* __restrict__ scores,
                                                                       const float* __restrict__ v, float* u,
                                                                       float2* part, int M, int N, int rw, int P,
                                                                       float alpha, float lm_in, float lm_bin,
                                                                       const SkPair* pairs = nullptr) {
  static_assert(!(PF && RAGGED), "the ragged walk loads each row at the top of its iteration");
  __shared__ float2 mbuf[W / 2][kSkMaxN + 1]; // wave-pair merge buffers
  __shared__ float4 vs[kSkMaxN / 4 + 1];      // v of the real columns
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / P, p = blockIdx.x - b * P;
  int Mr = M, Nr = N;
  if constexpr (RAGGED) {
    const SkPair pr = pairs[b];
    Mr = pr.m; Nr = pr.n; lm_in = pr.norm; lm_bin = pr.mu_bin;
    const int rb0 = p * W * rw;  // the workgroup's row run [rb0, rb0 + W rw)
    if (rb0 >= Mr && !(rb0 <= M && M < rb0 + W * rw)) {
      float2* dst = part + ((size_t)b * P + p) * (N + 1);
      for (int c = tid; c <= N; c += W * 64) dst[c] = make_float2(-INFINITY, 0.f);
      return;
    }
  }
  const float* vb = v + (size_t)b * (N + 1);
  for (int j = tid; j < 4 * (kSkMaxN / 4 + 1); j += W * 64)  // finite past N: masked columns stay -inf
    reinterpret_cast<float*>(vs)[j] = j < Nr ? vb[j] : 0.f;
  const float vbin = vb[N];
  __syncthreads();

  float cm[K4][4], cs[K4][4];
#pragma unroll
  for (int k = 0; k < K4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) cm[k][e] = -INFINITY, cs[k][e] = 0.f;
  float bm = -INFINITY, bs = 0.f;  // bin column (same in every lane)

  const int r0 = (p * W + wave) * rw;
  const int r1 = min(r0 + rw, M + 1);
  // row i -> registers (masked columns -inf; the dustbin row is alpha)
  auto load_row = [&](int i, float (&x)[K4][4]) {
    const bool bin_row = i == M;
    const float* row = scores + ((size_t)b * M + i) * N;
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const int c = 256 * k + 4 * lane;
      if (bin_row) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = c + e < Nr ? alpha : -INFINITY;
      } else if (VEC) {
        const f32x4 t = c < Nr ? *reinterpret_cast<const f32x4*>(row + c) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = RAGGED && c + e >= Nr ? -INFINITY : t[e];  // Nr need not be a multiple of 4
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[k][e] = c + e < Nr ? row[c + e] : -INFINITY;
      }
    }
  };
  float x[K4][4];
  if (!RAGGED && r0 < r1) load_row(r0, x);
#pragma unroll 1
  for (int i = r0; i < r1; ++i) {
    if constexpr (RAGGED) {
      if (i >= Mr && i != M) continue;  // padding
      load_row(i, x);
    }
    // PF: next row in flight while this one is reduced (measured slower: 10.9 vs 9.3 ms at
    // configs[4] -- the kernel is VALU-bound and the row copy costs 64 moves)
    float xn[K4][4];
    if (PF && i + 1 < r1) load_row(i + 1, xn);
    const bool bin_row = i == M;
    // u_i = log_mu_i - LSE_j(Zc_ij + v_j)   (superglue.py:178)
    // (Zc + v recomputed in the sum pass from LDS rather than held: registers go to x and the
    // column statistics)
    auto yv = [&](int k) {
      const float4 vv = vs[min(64 * k + lane, kSkMaxN / 4)];
      return f32x4{x[k][0] + vv.x, x[k][1] + vv.y, x[k][2] + vv.z, x[k][3] + vv.w};
    };
    float m = alpha + vbin;
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const f32x4 y = yv(k);
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, y[e]);
    }
    m = wave_max(m);
    asm volatile("" ::: "memory");  // re-read v from LDS below instead of holding Zc + v live
    float s = lane == 0 ? __expf((alpha + vbin) - m) : 0.f;
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const f32x4 y = yv(k);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += __expf(y[e] - m);
    }
    s = wave_sum(s);
    const float lse = m == -INFINITY ? m : m + __logf(s);
    const float ui = (bin_row ? lm_bin : lm_in) - lse;
    if (lane == 0) u[(size_t)b * (M + 1) + i] = ui;
    // column statistics of Zc_ij + u_i (superglue.py:179), one running (max, sum) per column
#pragma unroll
    for (int k = 0; k < K4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = x[k][e] + ui;
        const float d = z - cm[k][e];
        const float t = __expf(-fabsf(d));
        if (d > 0.f) {
          cs[k][e] = fmaf(cs[k][e], t, 1.f);
          cm[k][e] = z;
        } else {
          cs[k][e] += t;
        }
      }
    const float zb = alpha + ui;
    const float db = zb - bm, tb = __expf(-fabsf(db));
    if (db > 0.f) {
      bs = fmaf(bs, tb, 1.f);
      bm = zb;
    } else {
      bs += tb;
    }
    if (!RAGGED && i + 1 < r1) {
      if constexpr (PF) {
#pragma unroll
        for (int k = 0; k < K4; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) x[k][e] = xn[k][e];
      } else {
        load_row(i + 1, x);
      }
    }
  }

  // merge the W waves pairwise (W/2 -> 0.., ..., 1 -> 0) through LDS
#pragma unroll
  for (int half = W / 2; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) {
      float2* dst = mbuf[wave - half];
#pragma unroll
      for (int k = 0; k < K4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 256 * k + 4 * lane + e;
          if (c < N) dst[c] = make_float2(cm[k][e], cs[k][e]);
        }
      if (lane == 0) dst[N] = make_float2(bm, bs);
    }
    __syncthreads();
    if (wave < half) {
      const float2* src = mbuf[wave];
#pragma unroll
      for (int k = 0; k < K4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 256 * k + 4 * lane + e;
          if (c < N) {
            const float2 o = src[c];
            lse_merge(cm[k][e], cs[k][e], o.x, o.y);
          }
        }
      const float2 o = src[N];
      lse_merge(bm, bs, o.x, o.y);
    }
    __syncthreads();
  }
  if (wave == 0) {
    float2* dst = part + ((size_t)b * P + p) * (N + 1);
#pragma unroll
    for (int k = 0; k < K4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 256 * k + 4 * lane + e;
        if (c < N) dst[c] = make_float2(cm[k][e], cs[k][e]);
      }
    if (lane == 0) dst[N] = make_float2(bm, bs);
  }
}

// v_j = log_nu_j - LSE_i(Zc_ij + u_i) from the P workgroup partials of column j
// RAGGED: a padded column (j in [n, N)) has no potential and is left alone
template <bool RAGGED = false>
__global__ void sinkhorn_colmerge_kernel(const float2* part, float* v, int B, int N, int P, float lm_in, float lm_bin,
                                         const SkPair* pairs = nullptr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * (N + 1)) return;
  const int b = t / (N + 1), j = t - b * (N + 1);
  if constexpr (RAGGED) {
    const SkPair pr = pairs[b];
    if (j >= pr.n && j != N) return;
    lm_in = pr.norm; lm_bin = pr.nu_bin;
  }
  const float2* q = part + (size_t)b * P * (N + 1) + j;
  float m = -INFINITY, s = 0.f;
  for (int p = 0; p < P; ++p) {
    const float2 o = q[(size_t)p * (N + 1)];
    lse_merge(m, s, o.x, o.y);
  }
  const float lse = m == -INFINITY ? m : m + logf(s);
  v[t] = (j == N ? lm_bin : lm_in) - lse;
}


// Scaled variant (default): the column statistics reuse the row pass's exponentials.  With
// e_ij = exp(Zc_ij + v_j - m_i) (m_i the row max, so e_ij <= 1) and a_i = exp(u_i + m_i)
// = exp(log_mu_i) / s_i <= 1, e_ij * a_i = exp(Zc_ij + u_i + v_j): every row adds into the same
// per-column frame e^(v_j), so the column statistic is a plain sum S_j = sum_i e_ij a_i (one FMA
// per element, no second exponential, partials merge by addition) and
// LSE_i(Zc_ij + u_i) = log S_j - v_j.  Terms below fp32's range are lost where the exact kernel
// keeps them; the merge flags any column whose S_j falls under 2^-100 and
// log_optimal_transport then reruns with sinkhorn_fused_kernel (running max per column).
// RAGGED: as in sinkhorn_fused_kernel -- columns >= Nr masked (their sums stay 0), real rows end at
// Mr, the dustbin row stays row M; a workgroup of padding rows writes zero partials and leaves.
template <int K4, bool VEC, int W, bool NT, bool RAGGED = false>
__global__ __launch_bounds__(W * 64) void sinkhorn_scaled_kernel(const float* __restrict__ scores,
                                                                 const float* __restrict__ v, float* u, float* part,
                                                                 int M, int N, int rw, int P, float alpha, float lm_in,
                                                                 float lm_bin, const SkPair* pairs = nullptr) {
  __shared__ float sbuf[W / 2][kSkMaxN + 1];  // wave-pair merge buffers
  __shared__ float4 vs[kSkMaxN / 4 + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / P, p = blockIdx.x - b * P;
  int Mr = M, Nr = N;
  if constexpr (RAGGED) {
    const SkPair pr = pairs[b];
    Mr = pr.m; Nr = pr.n; lm_in = pr.norm; lm_bin = pr.mu_bin;
    const int rb0 = p * W * rw;  // the workgroup's row run [rb0, rb0 + W rw)
    if (rb0 >= Mr && !(rb0 <= M && M < rb0 + W * rw)) {
      float* dst = part + ((size_t)b * P + p) * (N + 1);
      for (int c = tid; c <= N; c += W * 64) dst[c] = 0.f;
      return;
    }
  }
  const float* vb = v + (size_t)b * (N + 1);
  // LG_SK_LOG2: the row pass works in log2 units (v staged as v log2 e, scores scaled by the same
  // FMA that adds v), so the exponentials are bare v_exp_f32 with no per-score multiply, and the
  // adds / FMAs run two columns per packed instruction
  constexpr float vsc = LG_SK_LOG2 ? 1.4426950408889634f : 1.f;
  for (int j = tid; j < 4 * (kSkMaxN / 4 + 1); j += W * 64) reinterpret_cast<float*>(vs)[j] = j < Nr ? vb[j] * vsc : 0.f;
  const float vbin = vb[N];
  const float ybin = LG_SK_LOG2 ? (alpha + vbin) * vsc : alpha + vbin;
  __syncthreads();

  float acc[K4][4];
#pragma unroll
  for (int k = 0; k < K4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[k][e] = 0.f;
  float accb = 0.f;

  const int r0 = (p * W + wave) * rw;
  const int r1 = min(r0 + rw, M + 1);
  // y: Zc_i row (masked columns -inf) -> Zc + v -> e; accumulates e * a into the column sums
  auto process = [&](float (&y)[K4][4], int i, bool bin_row) {
    asm volatile("" ::: "memory");  // re-read v from LDS per row rather than pinning 4*K4 registers
    float m = ybin;
#if LG_SK_LOG2
    const f32x2_ L2 = {vsc, vsc};
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const float4 vv = vs[min(64 * k + lane, kSkMaxN / 4)];
      const f32x2_ t0 = __builtin_elementwise_fma(f32x2_{y[k][0], y[k][1]}, L2, f32x2_{vv.x, vv.y});
      const f32x2_ t1 = __builtin_elementwise_fma(f32x2_{y[k][2], y[k][3]}, L2, f32x2_{vv.z, vv.w});
      y[k][0] = t0.x;
      y[k][1] = t0.y;
      y[k][2] = t1.x;
      y[k][3] = t1.y;
      m = fmaxf(m, fmaxf(t0.x, t0.y));
      m = fmaxf(m, fmaxf(t1.x, t1.y));
    }
    m = wave_max_dpp(m);
    const float eb = __builtin_amdgcn_exp2f(ybin - m);
    f32x2_ s2 = {lane == 0 ? eb : 0.f, 0.f};
    const f32x2_ nm = {-m, -m};
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const f32x2_ d0 = f32x2_{y[k][0], y[k][1]} + nm, d1 = f32x2_{y[k][2], y[k][3]} + nm;
      y[k][0] = __builtin_amdgcn_exp2f(d0.x);
      y[k][1] = __builtin_amdgcn_exp2f(d0.y);
      y[k][2] = __builtin_amdgcn_exp2f(d1.x);
      y[k][3] = __builtin_amdgcn_exp2f(d1.y);
      s2 += f32x2_{y[k][0], y[k][1]} + f32x2_{y[k][2], y[k][3]};
    }
    const float s = wave_sum_dpp(s2.x + s2.y);
    const float lm = bin_row ? lm_bin : lm_in;
    const float l2s = __log2f(s);
    const float ui = lm - (m + l2s) * 0.6931471805599453f;  // superglue.py:178, natural units
    if (lane == 0) u[(size_t)b * (M + 1) + i] = ui;
    const float a = __builtin_amdgcn_exp2f(lm * vsc - l2s);
    const f32x2_ a2 = {a, a};
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const f32x2_ r0 = __builtin_elementwise_fma(f32x2_{y[k][0], y[k][1]}, a2, f32x2_{acc[k][0], acc[k][1]});
      const f32x2_ r1 = __builtin_elementwise_fma(f32x2_{y[k][2], y[k][3]}, a2, f32x2_{acc[k][2], acc[k][3]});
      acc[k][0] = r0.x;
      acc[k][1] = r0.y;
      acc[k][2] = r1.x;
      acc[k][3] = r1.y;
    }
    accb = fmaf(eb, a, accb);
#else
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const float4 vv = vs[min(64 * k + lane, kSkMaxN / 4)];
      y[k][0] += vv.x;
      y[k][1] += vv.y;
      y[k][2] += vv.z;
      y[k][3] += vv.w;
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, y[k][e]);
    }
    m = wave_max_dpp(m);
    const float eb = __expf(ybin - m);
    float s = lane == 0 ? eb : 0.f;
#pragma unroll
    for (int k = 0; k < K4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y[k][e] = __expf(y[k][e] - m);
        s += y[k][e];
      }
    s = wave_sum_dpp(s);
    const float lm = bin_row ? lm_bin : lm_in;
    const float ls = __logf(s);
    const float ui = lm - (m + ls);  // superglue.py:178
    if (lane == 0) u[(size_t)b * (M + 1) + i] = ui;
    const float a = __expf(lm - ls);
#pragma unroll
    for (int k = 0; k < K4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[k][e] = fmaf(y[k][e], a, acc[k][e]);
    accb = fmaf(eb, a, accb);
#endif
  };
  const int rl = min(r1, Mr);  // real rows; the dustbin row M (all alpha) is handled after
  auto load = [&](float (&y)[K4][4], int i) {
    const char* row = reinterpret_cast<const char*>(scores + ((size_t)b * M + i) * N);
#pragma unroll
    for (int k = 0; k < K4; ++k) {
      const int c = 256 * k + 4 * lane;
      if (VEC) {
        f32x4 t = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (NT) {
          if (c < Nr) t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + 1024 * k + (uint32_t)(16 * lane)));
        } else {
          if (c < Nr) t = *reinterpret_cast<const f32x4*>(row + 1024 * k + (uint32_t)(16 * lane));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) y[k][e] = RAGGED && c + e >= Nr ? -INFINITY : t[e];  // Nr need not be a multiple of 4
      } else {
        const float* rf = reinterpret_cast<const float*>(row);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[k][e] = c + e < Nr ? rf[c + e] : -INFINITY;
      }
    }
  };
  // two row buffers in ping-pong: the next row's loads are in flight while this one is reduced
  float ya[K4][4], yb[K4][4];
  if (r0 < rl) load(ya, r0);
#pragma unroll 1
  for (int i = r0; i < rl; i += 2) {
    if (i + 1 < rl) load(yb, i + 1);
    process(ya, i, false);
    if (i + 1 >= rl) break;
    if (i + 2 < rl) load(ya, i + 2);
    process(yb, i + 1, false);
  }
  if (r0 <= M && M < r1) {
    float y[K4][4];
#pragma unroll
    for (int k = 0; k < K4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) y[k][e] = 256 * k + 4 * lane + e < Nr ? alpha : -INFINITY;
    process(y, M, true);
  }

#pragma unroll
  for (int half = W / 2; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) {
      float* dst = sbuf[wave - half];
#pragma unroll
      for (int k = 0; k < K4; ++k) {
        const int c = 256 * k + 4 * lane;
        if (VEC && c < N) {
          *reinterpret_cast<f32x4*>(dst + c) = f32x4{acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
        } else if (!VEC) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < N) dst[c + e] = acc[k][e];
        }
      }
      if (lane == 0) dst[N] = accb;
    }
    __syncthreads();
    if (wave < half) {
      const float* src = sbuf[wave];
#pragma unroll
      for (int k = 0; k < K4; ++k) {
        const int c = 256 * k + 4 * lane;
        if (VEC && c < N) {
          const f32x4 o = *reinterpret_cast<const f32x4*>(src + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[k][e] += o[e];
        } else if (!VEC) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < N) acc[k][e] += src[c + e];
        }
      }
      accb += src[N];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* dst = part + ((size_t)b * P + p) * (N + 1);
#pragma unroll
    for (int k = 0; k < K4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 256 * k + 4 * lane + e;
        if (c < N) dst[c] = acc[k][e];
      }
    if (lane == 0) dst[N] = accb;
  }
}

// v_j <- log_nu_j - (log S_j - v_j), S_j = sum of the P partials; flags S_j < 2^-100
// RAGGED: a padded column (j in [n, N)) has an empty sum -- it is not merged and cannot raise the
// flag; neither can any column of an empty pair
template <bool RAGGED = false>
__global__ void sinkhorn_scaled_merge_kernel(const float* part, float* v, int* flag, int B, int N, int P, float lm_in,
                                             float lm_bin, const SkPair* pairs = nullptr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  bool low = false;
  bool on = t < B * (N + 1);
  if constexpr (RAGGED) {
    if (on) {
      const SkPair pr = pairs[t / (N + 1)];
      const int j = t % (N + 1);
      on = pr.m > 0 && (j < pr.n || j == N);
      lm_in = pr.norm; lm_bin = pr.nu_bin;
    }
  }
  if (on) {
    const int b = t / (N + 1), j = t - b * (N + 1);
    const float* q = part + (size_t)b * P * (N + 1) + j;
    float S = 0.f;
#pragma unroll 8
    for (int p = 0; p < P; ++p) S += q[(size_t)p * (N + 1)];
    low = !(S >= 0x1p-100f);
    const float lse = logf(S) - v[t];
    v[t] = (j == N ? lm_bin : lm_in) - lse;
  }
  if (__ballot(low) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// The same merge with the P partials of a column spread over WAYS threads (fixed order: way w sums
// partials w, w + WAYS, ..., then the ways are added in order): a pair group of one or two pairs
// has P = 128-256 partials per column, whose sequential sum in one thread was latency-bound
// (one 4097-thread launch, 256 dependent-latency loads each).  grid (ceil((N+1)/64), B), block (64, WAYS).
template <int WAYS, bool RAGGED = false>
__global__ __launch_bounds__(64 * WAYS) void sinkhorn_scaled_merge_ways_kernel(const float* part, float* v, int* flag, int N,
                                                                               int P, float lm_in, float lm_bin,
                                                                               const SkPair* pairs = nullptr) {
  __shared__ float red[WAYS][64];
  const int tx = threadIdx.x, w = threadIdx.y;
  const int b = blockIdx.y, j = blockIdx.x * 64 + tx;
  bool on = j <= N;
  if constexpr (RAGGED) {
    const SkPair pr = pairs[b];
    on = on && pr.m > 0 && (j < pr.n || j == N);
    lm_in = pr.norm; lm_bin = pr.nu_bin;
  }
  float S = 0.f;
  if (on) {
    const float* q = part + (size_t)b * P * (N + 1) + j;
#pragma unroll 4
    for (int p = w; p < P; p += WAYS) S += q[(size_t)p * (N + 1)];
  }
  red[w][tx] = S;
  __syncthreads();
  if (w != 0) return;
  S = 0.f;
#pragma unroll
  for (int k = 0; k < WAYS; ++k) S += red[k][tx];
  bool low = false;
  if (on) {
    const size_t t = (size_t)b * (N + 1) + j;
    low = !(S >= 0x1p-100f);
    const float lse = logf(S) - v[t];
    v[t] = (j == N ? lm_bin : lm_in) - lse;
  }
  if (__ballot(low) != 0ull && tx == 0) atomicOr(flag, 1);
}

static void launch_scaled_merge(const float* part, float* v, int* flag, int B, int N, int P, float lm_in, float lm_bin,
                                const SkPair* pairs, hipStream_t st) {
  if (pairs) {
    if (P >= 64)
      hipLaunchKernelGGL((sinkhorn_scaled_merge_ways_kernel<8, true>), dim3((N + 1 + 63) / 64, B), dim3(64, 8), 0, st, part, v,
                         flag, N, P, lm_in, lm_bin, pairs);
    else
      hipLaunchKernelGGL(sinkhorn_scaled_merge_kernel<true>, dim3((B * (N + 1) + 255) / 256), dim3(256), 0, st, part, v, flag,
                         B, N, P, lm_in, lm_bin, pairs);
  } else if (P >= 64) {
    hipLaunchKernelGGL((sinkhorn_scaled_merge_ways_kernel<8, false>), dim3((N + 1 + 63) / 64, B), dim3(64, 8), 0, st, part, v,
                       flag, N, P, lm_in, lm_bin, (const SkPair*)nullptr);
  } else {
    hipLaunchKernelGGL(sinkhorn_scaled_merge_kernel<false>, dim3((B * (N + 1) + 255) / 256), dim3(256), 0, st, part, v, flag,
                       B, N, P, lm_in, lm_bin, (const SkPair*)nullptr);
  }
}

template <int K4>
static void launch_fused(const float* scores, const float* v, float* u, float2* part, int B, int M, int N,
                         const SkPlan& pl, float alpha, float lm_in, float mu_bin, const SkPair* pairs, hipStream_t st) {
  // 16 chunks per lane: a row (64) + column statistics (128) exceed the 256 registers of two
  // waves per SIMD, so those run 4 waves per workgroup at one wave per SIMD
  constexpr int W = sk_waves(K4, true);
  const dim3 grid(B * pl.p), block(W * 64);
  const SkPair* none = nullptr;
  if (pairs) {
    if (N % 4 == 0)
      hipLaunchKernelGGL((sinkhorn_fused_kernel<K4, true, W, false, true>), grid, block, 0, st, scores, v, u, part, M, N,
                         pl.rw, pl.p, alpha, lm_in, mu_bin, pairs);
    else
      hipLaunchKernelGGL((sinkhorn_fused_kernel<K4, false, W, false, true>), grid, block, 0, st, scores, v, u, part, M, N,
                         pl.rw, pl.p, alpha, lm_in, mu_bin, pairs);
  } else if (N % 4 == 0)
    hipLaunchKernelGGL((sinkhorn_fused_kernel<K4, true, W>), grid, block, 0, st, scores, v, u, part, M, N, pl.rw, pl.p,
                       alpha, lm_in, mu_bin, none);
  else
    hipLaunchKernelGGL((sinkhorn_fused_kernel<K4, false, W>), grid, block, 0, st, scores, v, u, part, M, N, pl.rw,
                       pl.p, alpha, lm_in, mu_bin, none);
}


template <int K4>
static void launch_scaled(const float* scores, const float* v, float* u, float* part, int B, int M, int N,
                          const SkPlan& pl, float alpha, float lm_in, float mu_bin, bool nt, const SkPair* pairs,
                          hipStream_t st) {
  constexpr int W = sk_waves(K4, false);
  const dim3 grid(B * pl.p), block(W * 64);
  const SkPair* none = nullptr;
  if (pairs) {
    if (N % 4 == 0) {
      if (nt)
        hipLaunchKernelGGL((sinkhorn_scaled_kernel<K4, true, W, true, true>), grid, block, 0, st, scores, v, u, part, M, N,
                           pl.rw, pl.p, alpha, lm_in, mu_bin, pairs);
      else
        hipLaunchKernelGGL((sinkhorn_scaled_kernel<K4, true, W, false, true>), grid, block, 0, st, scores, v, u, part, M, N,
                           pl.rw, pl.p, alpha, lm_in, mu_bin, pairs);
    } else {
      hipLaunchKernelGGL((sinkhorn_scaled_kernel<K4, false, W, false, true>), grid, block, 0, st, scores, v, u, part, M, N,
                         pl.rw, pl.p, alpha, lm_in, mu_bin, pairs);
    }
  } else if (N % 4 == 0) {
    if (nt)
      hipLaunchKernelGGL((sinkhorn_scaled_kernel<K4, true, W, true>), grid, block, 0, st, scores, v, u, part, M, N, pl.rw,
                         pl.p, alpha, lm_in, mu_bin, none);
    else
      hipLaunchKernelGGL((sinkhorn_scaled_kernel<K4, true, W, false>), grid, block, 0, st, scores, v, u, part, M, N,
                         pl.rw, pl.p, alpha, lm_in, mu_bin, none);
  } else {
    hipLaunchKernelGGL((sinkhorn_scaled_kernel<K4, false, W, false>), grid, block, 0, st, scores, v, u, part, M, N, pl.rw,
                       pl.p, alpha, lm_in, mu_bin, none);
  }
}

// Pair blocking (opt-in, LG_SK_GROUP=<pairs> or LG_SK_GROUP_MB=<MiB>): the scores of all B pairs
// (B*M*N*4 bytes; 537 MB at configs[4]) do not fit the 256 MiB Infinity Cache, so iterating over
// every pair streams them from HBM 50 times.  Pairs are independent, so they can run in groups
// whose scores fit, each group through all its iterations before the next, with normal (allocating)
// loads.  Measured at B = 8, N = 4096 (profiles/r03/sk_sweep.log): streaming 5.21 ms; groups of
// 1 / 2 / 4 pairs 11.5 / 7.5 / 6.0 ms on one stream, 7.1 / 5.3 / 5.5 ms on two streams.  A group's
// row kernel has only ~2 rows per wave, so its fixed costs (v staging, the 8-wave merge tree, the
// partial write, the merge launch) outweigh the faster Infinity-Cache reads; streaming stays the
// default.
// The schedule knobs are read from the environment ONCE per process (the workspace
// query and the run must agree, whatever the environment does in between).
struct SkEnv {
  int group = 0;        // LG_SK_GROUP (pairs; <= 0: unset)
  double group_mb = 0;  // LG_SK_GROUP_MB (MiB; <= 0: unset)
  int streams = 2;      // LG_SK_STREAMS
};
static const SkEnv& sk_env() {
  static const SkEnv env = [] {
    SkEnv x;
    if (const char* e = getenv("LG_SK_GROUP")) x.group = atoi(e) > 0 ? atoi(e) : -1;  // set, <= 0: every pair
    if (const char* e = getenv("LG_SK_GROUP_MB")) x.group_mb = atof(e);
    if (const char* e = getenv("LG_SK_STREAMS")) x.streams = atoi(e);
    return x;
  }();
  return env;
}
static int sk_group(int B, int M, int N) {
  const size_t per = (size_t)M * N * 4;
  const SkEnv& env = sk_env();
  if (env.group != 0) return env.group < 0 ? B : std::min(env.group, B);
  if (env.group_mb <= 0) return B;  // streaming schedule
  const size_t cap = (size_t)env.group_mb << 20;
  if ((size_t)B * per <= cap) return B;
  return (int)std::max<size_t>(1, std::min<size_t>(B, cap / per));
}

// Pair groups run on LG_SK_STREAMS (default 2) library-owned streams, forked from and joined back
// to the caller's stream with events: one group's small merge launch and launch gaps overlap the
// other group's row kernel, and both groups' scores share the Infinity Cache (2 x 67 MB at N =
// 4096).  Streams and events are created once per device and reused.
static int sk_streams_wanted(int groups) { return std::max(1, std::min({sk_env().streams, groups, 4})); }
// one fork..join at a time per process: the library-owned streams and the fork event are shared
static std::mutex g_sk_enqueue_mu;
struct SkStreams {
  hipStream_t s[4] = {};
  hipEvent_t fork = nullptr, join[4] = {};
  bool ok = false;
};
static hipError_t sk_streams_for_device(SkStreams*& out) {
  static std::mutex mu;
  static SkStreams per_dev[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lk(mu);
  SkStreams& x = per_dev[dev];
  if (!x.ok) {
    for (int i = 0; i < 4; ++i) {
      if ((e = hipStreamCreateWithFlags(&x.s[i], hipStreamNonBlocking)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&x.join[i], hipEventDisableTiming)) != hipSuccess) return e;
    }
    if ((e = hipEventCreateWithFlags(&x.fork, hipEventDisableTiming)) != hipSuccess) return e;
    x.ok = true;
  }
  out = &x;
  return hipSuccess;
}

// partial buffers (floats of (N+1)) one launch of pair group gb needs
static size_t sk_group_parts(int gb, int M, int N) { return (size_t)gb * sk_plan(gb, M, N, false).p; }

static std::atomic<long long> g_sk_reruns{0};
long long sinkhorn_exact_reruns() { return g_sk_reruns.load(); }
static std::atomic<int> g_sk_force_exact{0};
int sinkhorn_force_exact(int on) { return g_sk_force_exact.exchange(on ? 1 : 0); }

// the per-pair table of a ragged batch sits behind everything else
static size_t sk_pairs_floats(int B) { return (size_t)B * (sizeof(SkPair) / sizeof(float)) + 64; }
static size_t sk_base_floats(int B, int M, int N);
size_t sinkhorn_workspace_floats(int B, int M, int N) { return ((sk_base_floats(B, M, N) + 7) & ~size_t(7)) + sk_pairs_floats(B); }

static size_t sk_base_floats(int B, int M, int N) {
  if (sk_fused_ok(M, N)) {  // [u | v | partials (max, sum) B x P x (N+1) | flag]
    const int G = sk_group(B, M, N);
    const int ns = G < B ? sk_streams_wanted((B + G - 1) / G) : 1;
    const size_t parts = std::max((size_t)B * std::max(sk_plan(B, M, N, true).p, sk_plan(B, M, N, false).p),
                                  (size_t)ns * sk_group_parts(G, M, N));
    return (size_t)B * (M + 1) + 64 + (size_t)B * (N + 1) + 64 + 2 * parts * (N + 1) + 256 + 64;
  }
  return (size_t)B * M * N + (size_t)B * (M + 1) + (size_t)B * (N + 1) + 256;
}

hipError_t log_optimal_transport(const float* scores, float alpha, int B, int M, int N, int iters, float* Z, float* ws,
                                 hipStream_t st, const int* num0, const int* num1) {
  if (B == 0) return hipSuccess;
  if ((num0 == nullptr) != (num1 == nullptr) || (num0 && (M <= 0 || N <= 0))) return hipErrorInvalidValue;
  // log_mu / log_nu (superglue.py:194-197), computed in fp32 like the reference
  const float ms = (float)M, ns = (float)N;
  const float norm = -logf(ms + ns);
  const float mu_bin = logf(ns) + norm, nu_bin = logf(ms) + norm;
  const bool fused = sk_fused_ok(M, N);
  const SkPair* none = nullptr;
  float* sT = ws;
  float* u = fused ? ws : sT + (size_t)B * M * N;
  float* v = u + (size_t)B * (M + 1) + 64;
  hipError_t e;
  if ((e = hipMemsetAsync(u, 0, sizeof(float) * B * (M + 1), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(v, 0, sizeof(float) * B * (N + 1), st)) != hipSuccess) return e;
  // a ragged batch: the counts are clamped and the pairs' own marginals derived on the device
  SkPair* pairs = nullptr;
  if (num0) {
    pairs = reinterpret_cast<SkPair*>(ws + ((sk_base_floats(B, M, N) + 7) & ~size_t(7)));
    hipLaunchKernelGGL(sk_pairs_kernel, dim3((B + 255) / 256), dim3(256), 0, st, num0, num1, pairs, B, M, N, norm, mu_bin,
                       nu_bin);
  }
  if (fused) {
    float2* part = reinterpret_cast<float2*>(v + (size_t)B * (N + 1) + 64);
    const SkPlan pl = sk_plan(B, M, N, false), ple = sk_plan(B, M, N, true);
    const int G0 = sk_group(B, M, N);
    const int ns0 = G0 < B ? sk_streams_wanted((B + G0 - 1) / G0) : 1;
    const size_t parts = std::max((size_t)B * std::max(pl.p, ple.p), (size_t)ns0 * sk_group_parts(G0, M, N));
    int* flag = reinterpret_cast<int*>(part + parts * (N + 1)) + 64;
    const int k4 = (N + 255) / 256;
    int low = 0;
    const bool scaled = kSkScaled && !g_sk_force_exact.load();  // test instrumentation: the exact kernels alone
    if (scaled) {
      if ((e = hipMemsetAsync(flag, 0, sizeof(int), st)) != hipSuccess) return e;
      const int G = G0;
      // streaming schedule (one group of every pair): the scores pass the caches non-temporally;
      // pair-blocked groups keep theirs in the Infinity Cache
      const bool nt = LG_SK_NT && G == B;
      const int ns = ns0;
      SkStreams* ss = nullptr;
      std::unique_lock<std::mutex> enqueue_lock(g_sk_enqueue_mu, std::defer_lock);
      if (ns > 1) {
        enqueue_lock.lock();
        if ((e = sk_streams_for_device(ss)) != hipSuccess) return e;
        if ((e = hipEventRecord(ss->fork, st)) != hipSuccess) return e;
        for (int q = 0; q < ns; ++q)
          if ((e = hipStreamWaitEvent(ss->s[q], ss->fork, 0)) != hipSuccess) return e;
      }
      for (int b0 = 0, gi = 0; b0 < B; b0 += G, ++gi) {
        const int gb = std::min(G, B - b0);
        const int q = gi % ns;
        hipStream_t sq = ns > 1 ? ss->s[q] : st;
        float* fp = reinterpret_cast<float*>(part) + (size_t)q * sk_group_parts(G, M, N) * (N + 1);
        const SkPlan pg = sk_plan(gb, M, N, false);
        const float* sc = scores + (size_t)b0 * M * N;
        float* ug = u + (size_t)b0 * (M + 1);
        float* vg = v + (size_t)b0 * (N + 1);
        const SkPair* pgp = pairs ? pairs + b0 : nullptr;
        for (int it = 0; it < iters; ++it) {
          if (k4 <= 1) launch_scaled<1>(sc, vg, ug, fp, gb, M, N, pg, alpha, norm, mu_bin, nt, pgp, sq);
          else if (k4 <= 2) launch_scaled<2>(sc, vg, ug, fp, gb, M, N, pg, alpha, norm, mu_bin, nt, pgp, sq);
          else if (k4 <= 4) launch_scaled<4>(sc, vg, ug, fp, gb, M, N, pg, alpha, norm, mu_bin, nt, pgp, sq);
          else if (k4 <= 8) launch_scaled<8>(sc, vg, ug, fp, gb, M, N, pg, alpha, norm, mu_bin, nt, pgp, sq);
          else launch_scaled<16>(sc, vg, ug, fp, gb, M, N, pg, alpha, norm, mu_bin, nt, pgp, sq);
          launch_scaled_merge(fp, vg, flag, gb, N, pg.p, norm, nu_bin, pgp, sq);
        }
      }
      if (ns > 1) {
        for (int q = 0; q < ns; ++q) {
          if ((e = hipEventRecord(ss->join[q], ss->s[q])) != hipSuccess) return e;
          if ((e = hipStreamWaitEvent(st, ss->join[q], 0)) != hipSuccess) return e;
        }
        enqueue_lock.unlock();
      }
      if ((e = hipGetLastError()) != hipSuccess) return e;
      // the flag decides whether the exact kernel reruns: one 4-byte read-back
      if ((e = hipMemcpyAsync(&low, flag, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
      if (low) {
        g_sk_reruns.fetch_add(1);
        if ((e = hipMemsetAsync(u, 0, sizeof(float) * B * (M + 1), st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(v, 0, sizeof(float) * B * (N + 1), st)) != hipSuccess) return e;
      }
    }
    for (int it = 0; (!scaled || low) && it < iters; ++it) {
      if (k4 <= 1) launch_fused<1>(scores, v, u, part, B, M, N, ple, alpha, norm, mu_bin, pairs, st);
      else if (k4 <= 2) launch_fused<2>(scores, v, u, part, B, M, N, ple, alpha, norm, mu_bin, pairs, st);
      else if (k4 <= 4) launch_fused<4>(scores, v, u, part, B, M, N, ple, alpha, norm, mu_bin, pairs, st);
      else if (k4 <= 8) launch_fused<8>(scores, v, u, part, B, M, N, ple, alpha, norm, mu_bin, pairs, st);
      else launch_fused<16>(scores, v, u, part, B, M, N, ple, alpha, norm, mu_bin, pairs, st);
      if (pairs)
        hipLaunchKernelGGL(sinkhorn_colmerge_kernel<true>, dim3((B * (N + 1) + 255) / 256), dim3(256), 0, st, part, v, B, N,
                           ple.p, norm, nu_bin, pairs);
      else
        hipLaunchKernelGGL(sinkhorn_colmerge_kernel<false>, dim3((B * (N + 1) + 255) / 256), dim3(256), 0, st, part, v, B, N,
                           ple.p, norm, nu_bin, none);
    }
  } else {
    const dim3 tg((N + 63) / 64, (M + 63) / 64, B);
    if (pairs)
      hipLaunchKernelGGL(transpose_kernel<true>, tg, dim3(256), 0, st, scores, sT, M, N, pairs);
    else if (M > 0 && N > 0)
      hipLaunchKernelGGL(transpose_kernel<false>, tg, dim3(256), 0, st, scores, sT, M, N, none);
  }
  for (int it = 0; !fused && it < iters; ++it) {
    const dim3 gu((B * (M + 1) + 3) / 4), gv((B * (N + 1) + 3) / 4);
    if (pairs) {
      hipLaunchKernelGGL(lse_step_kernel<true>, gu, dim3(256), 0, st, scores, v, u, B, M, N, alpha, norm, mu_bin, pairs, 0);
      hipLaunchKernelGGL(lse_step_kernel<true>, gv, dim3(256), 0, st, sT, u, v, B, N, M, alpha, norm, nu_bin, pairs, 1);
    } else {
      hipLaunchKernelGGL(lse_step_kernel<false>, gu, dim3(256), 0, st, scores, v, u, B, M, N, alpha, norm, mu_bin, none, 0);
      hipLaunchKernelGGL(lse_step_kernel<false>, gv, dim3(256), 0, st, sT, u, v, B, N, M, alpha, norm, nu_bin, none, 0);
    }
  }
  const dim3 og(B * (M + 1), (N + 1 + 1023) / 1024);
  if (pairs)
    hipLaunchKernelGGL(sinkhorn_out_kernel<true>, og, dim3(256), 0, st, scores, u, v, Z, M, N, alpha, norm, pairs);
  else
    hipLaunchKernelGGL(sinkhorn_out_kernel<false>, og, dim3(256), 0, st, scores, u, v, Z, M, N, alpha, norm, none);
  return hipGetLastError();
}

}  // namespace lg
