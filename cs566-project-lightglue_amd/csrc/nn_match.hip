// Nearest-neighbour matcher on the fp16x3 matrix cores (gfx950): the reference's
// matchers/nearest_neighbor_matcher.py:16-72 with nothing of size M*N read back.
//
//   sim = d0 . d1^T                                              :53
//   matches0 / matches1 = find_nn(sim), find_nn(sim^T)           :16-25 (top-2, ratio / distance test)
//   mutual_check                                                 :28-35
//   la[:-1, :-1] = log_softmax_j(sim) + log_softmax_i(sim)       :61-62
//
// The descriptors become one fp16x3 plane image (image-0 rows of pair b at b*M, image-1 rows at
// B*M + b*N, columns zero-padded to a multiple of 32, range-scaled like the md planes so |d| <= 16).
//   pass A: per 256 x 256 tile, each row's (best, first index of the best, second best) over the
//           tile's columns and each column's over the tile's rows, reduced in registers (DPP /
//           permlane) and LDS; with the log assignment requested also their (max, sum exp); with
//           the similarity requested the fp32 tile is written
//   pass B: (log assignment only) the same tile again -- the same instructions on the same data,
//           so the same bits -- la = (s - rowlse) + (s - collse)
// Small kernels merge the tile partials in tile order, apply the thresholds and the mutual check.
// This translation unit is built with -ffp-contract=off: the threshold arithmetic is the
// reference's separate fp32 operations.
#include <algorithm>

#include "common.h"
#include "h3_pipeline.h"
#include "kernels.h"
#include "tile_reduce.h"

namespace lg {

namespace {
constexpr int kNnTile = 256;

// h3_pipeline.h h3_frag for a tile whose first plane-image row `ro` is no multiple of 16 (any M, N):
// the LDS-DMA copy is linear, so LDS row r holds image row ro + r, stored under that row's swizzle
__device__ __forceinline__ f16x8 nn_frag(const char* st, int t0, int r, int c, int ro) {
  return *reinterpret_cast<const f16x8*>(st + t0 + r * (kKB * 2) + ((c ^ plane_swz(r + ro)) << 4));
}

// (best value, first index of the best, second-best value) of a set of candidates.  Merge of two
// disjoint sets; equal bests keep the lower index, and the loser of the bests is a second best.
__device__ __forceinline__ void top2_merge(float& v1, int& i1, float& v2, float ov1, int oi1, float ov2) {
  v2 = fmaxf(fminf(v1, ov1), fmaxf(v2, ov2));
  if (ov1 > v1 || (ov1 == v1 && oi1 < i1)) {
    v1 = ov1;
    i1 = oi1;
  }
}
template <int C>
__device__ __forceinline__ void top2_dpp(float& v1, int& i1, float& v2) {
  const float ov1 = dppf<C>(v1), ov2 = dppf<C>(v2);
  const int oi1 = dppi<C>(i1);
  top2_merge(v1, i1, v2, ov1, oi1, ov2);
}
// over the 16 lanes of a DPP row (every step merges disjoint lane sets)
__device__ __forceinline__ void top2_row16(float& v1, int& i1, float& v2) {
  top2_dpp<0xB1>(v1, i1, v2);
  top2_dpp<0x4E>(v1, i1, v2);
  top2_dpp<0x141>(v1, i1, v2);
  top2_dpp<0x140>(v1, i1, v2);
}
// over the four 16-lane rows of the wave (lanes 16 and 32 apart)
__device__ __forceinline__ void top2_rows(float& v1, int& i1, float& v2) {
  {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v1), __float_as_uint(v1), false, false);
    const auto b = __builtin_amdgcn_permlane16_swap((unsigned)i1, (unsigned)i1, false, false);
    const auto c = __builtin_amdgcn_permlane16_swap(__float_as_uint(v2), __float_as_uint(v2), false, false);
    float x1 = __uint_as_float(a[0]), x2 = __uint_as_float(c[0]);
    int xi = (int)b[0];
    top2_merge(x1, xi, x2, __uint_as_float(a[1]), (int)b[1], __uint_as_float(c[1]));
    v1 = x1, i1 = xi, v2 = x2;
  }
  {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v1), __float_as_uint(v1), false, false);
    const auto b = __builtin_amdgcn_permlane32_swap((unsigned)i1, (unsigned)i1, false, false);
    const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(v2), __float_as_uint(v2), false, false);
    float x1 = __uint_as_float(a[0]), x2 = __uint_as_float(c[0]);
    int xi = (int)b[0];
    top2_merge(x1, xi, x2, __uint_as_float(a[1]), (int)b[1], __uint_as_float(c[1]));
    v1 = x1, i1 = xi, v2 = x2;
  }
}

}  // namespace

struct NnArgs {
  PlaneRef P;            // descriptor planes, K = 32 nk
  const unsigned* rtab;  // their range exponent at `slot`
  int slot, nk;
  int B, M, N;
  const int* Mb;  // per-pair counts (nullable, both or none)
  const int* Nb;
  int want_lse;
  float* sim;  // [B][M][N] or null (pass A)
  float* la;   // [B][M+1][N+1] (pass B)
  // pass A partials: rows [B][M][ntn], columns [B][ntm][N]
  float* rv1; int* ri1; float* rv2;
  float* cv1; int* ci1; float* cv2;
  float2* rowp; float* pmax; float* psum;
  // merged (nn_decide_kernel): log-sum-exp per row / column, thresholded neighbours
  float* rlse; float* clse;
  int* mm0; int* mm1;
};

// 256 x 256 similarity tile, 16 waves of 64 x 64 (assign_h3.hip sim_h3_kernel's geometry and
// k-loop, the k-tile count at run time).  PASS 0 = pass A, 1 = pass B.  RAGGED: rows / columns are
// bounded by the pair's own counts; M, N stay the layout capacities.
template <int PASS, bool RAGGED>
__global__ __launch_bounds__(1024) void nn_tile_kernel(NnArgs g) {
  constexpr int BM = kNnTile, BN = kNnTile, BK = kKB, NSTAGE = 2, NW = 16, WGN = 4;
  using S = H3Stage<BM, BN, NW>;
  constexpr int APT = S::APT, WPT = S::WPT, STAGE_BYTES = S::STAGE_BYTES, PPW = S::PPW;
  __shared__ __attribute__((aligned(1024))) char smem[NSTAGE * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / WGN) * 64, wn0 = (wave % WGN) * 64;
  const int M = g.M, N = g.N;
  const int ntm = (M + BM - 1) / BM, ntn = (N + BN - 1) / BN, T = ntm * ntn;
  // whole pairs per XCD when the batch allows it, else the tiles of a pair spread in panel order
  int b, tile;
  if (g.B % 8 == 0) {
    const int id = blockIdx.x, local = id >> 3;
    b = (id & 7) + 8 * (local / T);
    tile = local % T;
  } else {
    b = blockIdx.x / T;
    tile = xcd_remap(blockIdx.x % T, T);
  }
  const int tm = tile / ntn, tn = tile - tm * ntn;
  // the pair's bounds and the range exponent: read here -- h3_pipeline.h's counted wait allows no
  // load between a stage's issue and its wait
  int Mb = M, Nb = N;
  if constexpr (RAGGED) {
    Mb = min(max(g.Mb[b], 0), M);
    Nb = min(max(g.Nb[b], 0), N);
    // a tile wholly outside the pair's counts: no DMA is issued; neutral partials for the live rows
    // / columns it shares with other tiles
    if (tm * BM >= Mb || tn * BN >= Nb) {
      if constexpr (PASS == 0) {
        if (tid < 256) {
          const int i = tm * BM + tid;
          if (i < Mb) {
            const size_t o = ((size_t)b * M + i) * ntn + tn;
            g.rv1[o] = -INFINITY, g.ri1[o] = tn * BN, g.rv2[o] = -INFINITY;
            if (g.want_lse) g.rowp[o] = make_float2(-INFINITY, 0.f);
          }
        } else if (tid < 512) {
          const int j = tn * BN + tid - 256;
          if (j < Nb) {
            const size_t o = ((size_t)b * ntm + tm) * N + j;
            g.cv1[o] = -INFINITY, g.ci1[o] = tm * BM, g.cv2[o] = -INFINITY;
            if (g.want_lse) g.pmax[o] = -INFINITY, g.psum[o] = 0.f;
          }
        }
      }
      return;
    }
  }
  const int arow = b * M + tm * BM, wrow = g.B * M + b * N + tn * BN;  // plane-image rows
  const int aro = arow & 15, wro = wrow & 15;  // the swizzle has period 16: only the phase matters
  const float scale = ldexpf(1.f / kLoScale, 2 * range_slot_exp(g.rtab, g.slot));
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_char*)smem);
  const uint32_t voff = lane * 16;
  auto issue = [&](int kt, int stage) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int q = wave * PPW + i;  // [A h | A l | W h | W l], 16 pieces each
      const int pl = (q >> 4) & 1, pc = q & 15;
      const int r0 = q < 32 ? arow : wrow;
      const char* src = reinterpret_cast<const char*>(g.P.p + pl * g.P.ps + ((size_t)kt * g.P.rows_pad + r0) * BK) + pc * 1024;
      dma16(src, voff, lds0 + stage * STAGE_BYTES + q * 1024);
    }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = g.nk;
  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    ring_wait<NSTAGE, PPW>(0);
    lds_barrier();
    if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
    // h3_pipeline.h h3_mma_stage, kept in place as in sim_h3_kernel (registers)
    const char* st = smem + (kt & 1) * STAGE_BYTES;
    const int c = lane >> 4, r16 = lane & 15;
    f16x8 ah[4], al[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ah[i] = nn_frag(st, 0, wm0 + i * 16 + r16, c, aro);
      al[i] = nn_frag(st, APT, wm0 + i * 16 + r16, c, aro);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wn0 + j * 16 + r16;
      const f16x8 wh = nn_frag(st, 2 * APT, r, c, wro);
      const f16x8 wl = nn_frag(st, 2 * APT + WPT, r, c, wro);
      const f16x8 whs = wh * (_Float16)kLoScale;  // exact: |d_h| <= 16
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = mfma_h3_16(ah[i], al[i], whs, wl, wh, acc[i][j]);
    }
  }
  lds_barrier();

  // lane element (ti, tj, r): pair-local row i0 + 16 ti + r, column j0 + 16 tj
  const int i0 = tm * BM + wm0 + 4 * (lane >> 4), j0 = tn * BN + wn0 + (lane & 15);
  auto row_of = [&](int ti, int r) { return i0 + 16 * ti + r; };
  auto col_of = [&](int tj) { return j0 + 16 * tj; };
  // the tile's real elements to dst (row stride ld): 32-row passes through a per-wave LDS
  // transpose, one 256-byte row run per store
  auto write_tile = [&](float* dst, size_t ld) {
    float* ep = reinterpret_cast<float*>(smem) + wave * (32 * 64);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rr = a * 16 + 4 * (lane >> 4) + r, c = 16 * tj + (lane & 15);
            ep[rr * 64 + (c ^ ((rr & 1) << 2))] = acc[2 * p + a][tj][r];
          }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int j = tn * BN + wn0 + lane;
#pragma unroll 4
      for (int rr = 0; rr < 32; ++rr) {
        const int i = tm * BM + wm0 + 32 * p + rr;
        const float v = ep[rr * 64 + (lane ^ ((rr & 1) << 2))];
        if (i < Mb && j < Nb) st_stream(dst + i * ld + j, v);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  };

  if constexpr (PASS == 0) {
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[ti][tj][r] = (row_of(ti, r) < Mb && col_of(tj) < Nb) ? acc[ti][tj][r] * scale : -INFINITY;
    if (g.sim) {
      write_tile(g.sim + (size_t)b * M * N, (size_t)N);
      __syncthreads();  // the transpose buffers become the reduction tables
    }
    // LDS tables: rows [256][4 column waves], columns [4 row waves][256]
    float* t_rv1 = reinterpret_cast<float*>(smem);
    int* t_ri1 = reinterpret_cast<int*>(smem + 4096);
    float* t_rv2 = reinterpret_cast<float*>(smem + 8192);
    float* t_cv1 = reinterpret_cast<float*>(smem + 12288);
    int* t_ci1 = reinterpret_cast<int*>(smem + 16384);
    float* t_cv2 = reinterpret_cast<float*>(smem + 20480);
    float2* red = reinterpret_cast<float2*>(smem + 32768);  // [256][4] then [4][256] (max, sum)
    // rows: the wave's 64 columns (lane-local over tj in column order, then the 16 lanes of the row)
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v1 = acc[ti][0][r], v2 = -INFINITY;
        int i1 = col_of(0);
#pragma unroll
        for (int tj = 1; tj < 4; ++tj) top2_merge(v1, i1, v2, acc[ti][tj][r], col_of(tj), -INFINITY);
        top2_row16(v1, i1, v2);
        if ((lane & 15) == 0) {
          const int o = (wm0 + 16 * ti + 4 * (lane >> 4) + r) * 4 + (wave % WGN);
          t_rv1[o] = v1, t_ri1[o] = i1, t_rv2[o] = v2;
        }
      }
    // columns: the wave's 64 rows (lane-local over ti, r in row order, then the four 16-lane rows)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      float v1 = -INFINITY, v2 = -INFINITY;
      int i1 = row_of(0, 0);
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) top2_merge(v1, i1, v2, acc[ti][tj][r], row_of(ti, r), -INFINITY);
      top2_rows(v1, i1, v2);
      if (lane < 16) {
        const int o = (wave / WGN) * 256 + wn0 + 16 * tj + lane;
        t_cv1[o] = v1, t_ci1[o] = i1, t_cv2[o] = v2;
      }
    }
    if (g.want_lse) {  // assign_h3.hip's statistics pass
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float m = fmaxf(fmaxf(acc[ti][0][r], acc[ti][1][r]), fmaxf(acc[ti][2][r], acc[ti][3][r]));
          m = row16_max(m);
          float s = 0.f;
          if (m != -INFINITY)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) s += fast_exp(acc[ti][tj][r] - m);
          s = row16_sum(s);
          if ((lane & 15) == 0) red[(wm0 + 16 * ti + 4 * (lane >> 4) + r) * 4 + (wave % WGN)] = make_float2(m, s);
        }
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) {
        float m = -INFINITY;
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
          for (int r = 0; r < 4; ++r) m = fmaxf(m, acc[ti][tj][r]);
        float s = 0.f;
        if (m != -INFINITY)
#pragma unroll
          for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) s += fast_exp(acc[ti][tj][r] - m);
        lse_merge_rows(m, s);
        if (lane < 16) red[1024 + (wave / WGN) * 256 + wn0 + 16 * tj + lane] = make_float2(m, s);
      }
    }
    __syncthreads();
    if (tid < 256) {
      const int i = tm * BM + tid;
      float v1 = t_rv1[tid * 4], v2 = t_rv2[tid * 4];
      int i1 = t_ri1[tid * 4];
      for (int w = 1; w < 4; ++w) top2_merge(v1, i1, v2, t_rv1[tid * 4 + w], t_ri1[tid * 4 + w], t_rv2[tid * 4 + w]);
      if (i < Mb) {
        const size_t o = ((size_t)b * M + i) * ntn + tn;
        g.rv1[o] = v1, g.ri1[o] = i1, g.rv2[o] = v2;
      }
    } else if (tid < 512) {
      const int cl = tid - 256, j = tn * BN + cl;
      float v1 = t_cv1[cl], v2 = t_cv2[cl];
      int i1 = t_ci1[cl];
      for (int w = 1; w < 4; ++w) top2_merge(v1, i1, v2, t_cv1[w * 256 + cl], t_ci1[w * 256 + cl], t_cv2[w * 256 + cl]);
      if (j < Nb) {
        const size_t o = ((size_t)b * ntm + tm) * N + j;
        g.cv1[o] = v1, g.ci1[o] = i1, g.cv2[o] = v2;
      }
    } else if (tid < 768) {
      if (g.want_lse) {
        const int rl = tid - 512, i = tm * BM + rl;
        float m = red[rl * 4].x, s = red[rl * 4].y;
        for (int w = 1; w < 4; ++w) lse_merge(m, s, red[rl * 4 + w].x, red[rl * 4 + w].y);
        if (i < Mb) g.rowp[((size_t)b * M + i) * ntn + tn] = make_float2(m, s);
      }
    } else {
      if (g.want_lse) {
        const int cl = tid - 768, j = tn * BN + cl;
        float m = red[1024 + cl].x, s = red[1024 + cl].y;
        for (int w = 1; w < 4; ++w) lse_merge(m, s, red[1024 + w * 256 + cl].x, red[1024 + w * 256 + cl].y);
        if (j < Nb) {
          g.pmax[((size_t)b * ntm + tm) * N + j] = m;
          g.psum[((size_t)b * ntm + tm) * N + j] = s;
        }
      }
    }
  } else {
    // la = (s - rowlse_i) + (s - collse_j); s as pass A formed it (acc * scale)
    float cl[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) cl[tj] = g.clse[(size_t)b * N + min(col_of(tj), Nb - 1)];  // a live column: Nb >= 1 here
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float rl = g.rlse[(size_t)b * M + min(row_of(ti, r), Mb - 1)];
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
          const float x = acc[ti][tj][r] * scale;
          acc[ti][tj][r] = (x - rl) + (x - cl[tj]);
        }
      }
    write_tile(g.la + (size_t)b * (M + 1) * (N + 1), (size_t)(N + 1));
  }
}

// Merge the tile partials in tile order and apply find_nn (:16-25) in fp32 as written: one thread
// per row of image 0, then per row of image 1.  flags: 1 ratio test, 2 distance test.
__global__ void nn_decide_kernel(NnArgs g, int flags, float r2, float d2) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int M = g.M, N = g.N, BMt = g.B * M;
  if (t >= BMt + g.B * N) return;
  const int ntm = (M + kNnTile - 1) / kNnTile, ntn = (N + kNnTile - 1) / kNnTile;
  const bool side0 = t < BMt;
  const int u = side0 ? t : t - BMt;
  const int b = side0 ? u / M : u / N, e = side0 ? u - b * M : u - b * N;
  const int Mb = g.Mb ? min(max(g.Mb[b], 0), M) : M, Nb = g.Nb ? min(max(g.Nb[b], 0), N) : N;
  const int own = side0 ? Mb : Nb, cand = side0 ? Nb : Mb;
  int* mm = side0 ? g.mm0 : g.mm1;
  if (e >= own || cand < 1) {  // a padded point, or nothing to scan
    mm[u] = -1;
    return;
  }
  const int nt = side0 ? ntn : ntm;
  const size_t base = side0 ? (size_t)u * ntn : (size_t)b * ntm * N + e, step = side0 ? 1 : (size_t)N;
  const float* pv1 = side0 ? g.rv1 : g.cv1;
  const int* pi1 = side0 ? g.ri1 : g.ci1;
  const float* pv2 = side0 ? g.rv2 : g.cv2;
  float v1 = pv1[base], v2 = pv2[base];
  int i1 = pi1[base];
  for (int k = 1; k < nt; ++k) top2_merge(v1, i1, v2, pv1[base + k * step], pi1[base + k * step], pv2[base + k * step]);
  const float dist0 = 2.f * (1.f - v1);
  bool keep = true;
  if (flags & 1) keep = cand >= 2 && dist0 <= r2 * (2.f * (1.f - v2));
  if (flags & 2) keep = keep && dist0 <= d2;
  keep = keep && (unsigned)i1 < (unsigned)cand;  // NaN similarities order nothing: no neighbour
  mm[u] = keep ? i1 : -1;
  if (g.want_lse) {
    float m, s;
    if (side0) {
      m = g.rowp[base].x, s = g.rowp[base].y;
      for (int k = 1; k < nt; ++k) lse_merge<false>(m, s, g.rowp[base + k].x, g.rowp[base + k].y);
      g.rlse[u] = m + logf(s);
    } else {
      m = g.pmax[base], s = g.psum[base];
      for (int k = 1; k < nt; ++k) lse_merge<false>(m, s, g.pmax[base + k * step], g.psum[base + k * step]);
      g.clse[u] = m + logf(s);
    }
  }
}

// mutual_check (:28-35) and the outputs: matches as int64, scores (m > -1) as fp32
__global__ void nn_finish_kernel(const int* mm0, const int* mm1, int B, int M, int N, int mutual, int64_t* m0, int64_t* m1,
                                 float* s0, float* s1) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * (M + N)) return;
  if (t < B * M) {
    const int b = t / M, i = t - b * M;
    int m = mm0[t];
    if (mutual && m > -1 && mm1[b * N + m] != i) m = -1;
    m0[t] = m;
    s0[t] = m > -1 ? 1.f : 0.f;
  } else {
    const int u = t - B * M, b = u / N, j = u - b * N;
    int m = mm1[u];
    if (mutual && m > -1 && mm0[b * M + m] != j) m = -1;
    m1[u] = m;
    s1[u] = m > -1 ? 1.f : 0.f;
  }
}

// What the tile passes do not write.  One block per (pair, row) of the [rows][ld] tensor with
// `border` extra row and column (1: the log assignment, border 0 and -inf outside the pair's real
// block; 0: the similarity, `fill` = 0 outside it).
__global__ void nn_fill_kernel(float* dst, int M, int N, int border, float fill, const int* Mbp, const int* Nbp) {
  const int rows = M + border, ld = N + border;
  const int b = blockIdx.x / rows, i = blockIdx.x - b * rows;
  float* row = dst + ((size_t)b * rows + i) * ld;
  if (i == M) {  // the border row
    for (int j = threadIdx.x; j < ld; j += blockDim.x) row[j] = 0.f;
    return;
  }
  if (border && threadIdx.x == 0) row[N] = 0.f;
  if (!Mbp) return;
  const int Mb = min(max(Mbp[b], 0), M), Nb = min(max(Nbp[b], 0), N);
  for (int j = (i < Mb ? Nb : 0) + threadIdx.x; j < N; j += blockDim.x) row[j] = fill;
}

// fp32 rows [R][D] -> [R][Dpad], zero-padded columns (widths that are no multiple of 32)
__global__ void nn_pad_rows_kernel(const float* x0, int r0, const float* x1, int r1, int D, int Dpad, float* out) {
  const size_t n = (size_t)(r0 + r1) * Dpad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / Dpad), c = (int)(i - (size_t)r * Dpad);
    out[i] = c < D ? (r < r0 ? x0[(size_t)r * D + c] : x1[(size_t)(r - r0) * D + c]) : 0.f;
  }
}

namespace {
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
struct NnLayout {
  int Dpad, rows_pad, ntm, ntn;
  size_t tab, planes, stage, rv1, ri1, rv2, cv1, ci1, cv2, rowp, pmax, psum, rlse, clse, mm0, mm1, total;
};
NnLayout nn_layout(int B, int M, int N, int D) {
  NnLayout L;
  L.Dpad = (D + kKB - 1) / kKB * kKB;
  L.rows_pad = (int)(((size_t)B * (M + N) + kNnTile + 255) / 256 * 256);
  L.ntm = (M + kNnTile - 1) / kNnTile;
  L.ntn = (N + kNnTile - 1) / kNnTile;
  const size_t R = (size_t)B * (M + N), rp = (size_t)B * M * L.ntn * 4, cp = (size_t)B * L.ntm * N * 4;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += up256(bytes);
    return at;
  };
  L.tab = take(2 * kRangeStride * sizeof(unsigned));
  L.planes = take(2 * (size_t)L.rows_pad * L.Dpad * sizeof(_Float16));
  L.stage = take(D % kKB ? R * L.Dpad * sizeof(float) : 0);
  L.rv1 = take(rp), L.ri1 = take(rp), L.rv2 = take(rp);
  L.cv1 = take(cp), L.ci1 = take(cp), L.cv2 = take(cp);
  L.rowp = take(2 * rp), L.pmax = take(cp), L.psum = take(cp);
  L.rlse = take((size_t)B * M * 4), L.clse = take((size_t)B * N * 4);
  L.mm0 = take((size_t)B * M * 4), L.mm1 = take((size_t)B * N * 4);
  L.total = o;
  return L;
}
}  // namespace

size_t nn_workspace_bytes(int B, int M, int N, int D) { return nn_layout(B, M, N, D).total; }

hipError_t nn_match(const NnCall& c, void* workspace, hipStream_t st) {
  const int B = c.B, M = c.M, N = c.N, D = c.D;
  const NnLayout L = nn_layout(B, M, N, D);
  char* ws = static_cast<char*>(workspace);
  auto at = [&](size_t off) { return ws + off; };
  unsigned* tab = reinterpret_cast<unsigned*>(at(L.tab));
  _Float16* planes = reinterpret_cast<_Float16*>(at(L.planes));
  const int R = B * (M + N);
#define NN_HIP(x)                     \
  do {                                \
    const hipError_t e_ = (x);        \
    if (e_ != hipSuccess) return e_;  \
  } while (0)
  NN_HIP(hipMemsetAsync(tab, 0, 2 * kRangeStride * sizeof(unsigned), st));
  const float* d0 = c.desc0;
  const float* d1 = c.desc1;
  if (D % kKB) {
    float* stage = reinterpret_cast<float*>(at(L.stage));
    const size_t n = (size_t)R * L.Dpad;
    hipLaunchKernelGGL(nn_pad_rows_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, d0, B * M,
                       d1, B * N, D, L.Dpad, stage);
    NN_HIP(hipGetLastError());
    d0 = stage;
    d1 = stage + (size_t)B * M * L.Dpad;
  }
  // the planes' range: |d| 2^-E <= 16 (the "y" operand bound), E = 0 for normalised descriptors
  NN_HIP(range_absmax2(d0, (size_t)B * M * L.Dpad, d1, (size_t)B * N * L.Dpad, tab, 0, st));
  const RangeOut ro{tab, 0, -1, 1.f, 0.f, 0.f, 1, 0, 11};
  NN_HIP(rows_to_planes2(d0, B * M, d1, B * N, L.Dpad, L.Dpad, planes, L.rows_pad, 0, ro, st));
  // the slack rows: zero, so that no NaN bit pattern reaches an MFMA
  NN_HIP(sp_zero_rows(planes, (long long)L.rows_pad * L.Dpad, L.rows_pad, L.Dpad, R, st));

  NnArgs g{};
  g.P = PlaneRef{planes, (long long)L.rows_pad * L.Dpad, L.rows_pad};
  g.rtab = tab, g.slot = 1, g.nk = L.Dpad / kKB;
  g.B = B, g.M = M, g.N = N, g.Mb = c.num0, g.Nb = c.num1;
  g.want_lse = c.la != nullptr;
  g.sim = c.sim, g.la = c.la;
  g.rv1 = (float*)at(L.rv1), g.ri1 = (int*)at(L.ri1), g.rv2 = (float*)at(L.rv2);
  g.cv1 = (float*)at(L.cv1), g.ci1 = (int*)at(L.ci1), g.cv2 = (float*)at(L.cv2);
  g.rowp = (float2*)at(L.rowp), g.pmax = (float*)at(L.pmax), g.psum = (float*)at(L.psum);
  g.rlse = (float*)at(L.rlse), g.clse = (float*)at(L.clse);
  g.mm0 = (int*)at(L.mm0), g.mm1 = (int*)at(L.mm1);
  const bool ragged = c.num0 != nullptr;
  const dim3 grid(L.ntm * L.ntn * B), block(1024);
  if (c.sim && ragged) {
    hipLaunchKernelGGL(nn_fill_kernel, dim3(B * M), dim3(256), 0, st, c.sim, M, N, 0, 0.f, c.num0, c.num1);
    NN_HIP(hipGetLastError());
  }
  if (ragged) hipLaunchKernelGGL((nn_tile_kernel<0, true>), grid, block, 0, st, g);
  else hipLaunchKernelGGL((nn_tile_kernel<0, false>), grid, block, 0, st, g);
  NN_HIP(hipGetLastError());
  hipLaunchKernelGGL(nn_decide_kernel, dim3((R + 255) / 256), dim3(256), 0, st, g, c.flags & 3, c.r2, c.d2);
  NN_HIP(hipGetLastError());
  hipLaunchKernelGGL(nn_finish_kernel, dim3((R + 255) / 256), dim3(256), 0, st, g.mm0, g.mm1, B, M, N, (c.flags >> 2) & 1,
                     c.m0, c.m1, c.s0, c.s1);
  NN_HIP(hipGetLastError());
  if (c.la) {
    hipLaunchKernelGGL(nn_fill_kernel, dim3(B * (M + 1)), dim3(256), 0, st, c.la, M, N, 1, -INFINITY, c.num0, c.num1);
    NN_HIP(hipGetLastError());
    if (ragged) hipLaunchKernelGGL((nn_tile_kernel<1, true>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((nn_tile_kernel<1, false>), grid, block, 0, st, g);
    NN_HIP(hipGetLastError());
  }
#undef NN_HIP
  return hipSuccess;
}

}  // namespace lg
