// Training (autograd) kernels for gfx950: the LightGlue backward pass (reference
// gluefactory/models/matchers/lightglue.py:159-315 differentiated by torch autograd in
// gluefactory/train.py:450) and the activation-saving training forward it needs.
//
// Arithmetic: fp32 in, fp32 accumulation, fp32 out, so a gradient of any magnitude is represented
// as fp32 represents it: no range scaling.  Which products run as bf16x6 (three bf16 pieces per
// operand, common.h) and which on the f32-input MFMA (v_mfma_f32_32x32x2_f32, exact fp32 products)
// follows from shape and alignment alone: train.h lists the routes.  Lane map of the f32 MFMA
// (common.h row32): A[l&31][l>>5], B[l>>5][l&31], accumulator register r of lane l =
// C[row32(r, l>>5)][l&31].
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "train.h"

namespace lg {

namespace {

constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// ============================================================================ GEMM
// 128 x 128 x 32 block tile, 4 waves of 64 x 64 (2 x 2 tiles of 32 x 32).  Both operands are
// staged in LDS k-major ([k][128 + 32]): a lane reads column (tile base + lane&31) of k-row
// 2s + (lane>>5); the 160-float row pitch puts the two lane halves on disjoint bank halves.
// Operands stored the other way round (m-major in memory) are transposed on the LDS write.
#ifndef LG_TG_BK
#define LG_TG_BK 16  // k-tile of the training GEMM (16: 40 KiB of LDS, several workgroups per CU)
#endif
constexpr int TG_BM = 128, TG_BN = 128, TG_BK = LG_TG_BK, TG_P = 160;
constexpr int TG_Q = TG_BK / 8;  // float4 loads per thread per operand and k-tile

struct TGemmK {
  TGemm g;
  int ksplit, kchunk;
  int vecA, vecB;
  float* part;   // [batch][ksplit][M][N] when ksplit > 1
  float* cpart;  // [batch][ksplit][M] column-sum partials (g.colsumA, ksplit > 1)
};

// X(i, k) for i in [i0, i0 + 128), k in [k0, k0 + 32): KMAJ -> X[k*ld + i], else X[i*ld + k]
template <bool KMAJ>
__device__ __forceinline__ void tg_load(const float* X, long long ld, int i0, int D, int k0, int kend, int vec, int t,
                                        f32x4 (&r)[TG_Q]) {
  if (KMAJ) {  // TG_BK k-rows of 128 i: thread t -> k-row (t >> 5) + 8q, i 4(t & 31) .. +3
    const int kr = t >> 5, i = i0 + (t & 31) * 4;
#pragma unroll
    for (int q = 0; q < TG_Q; ++q) {
      const int k = k0 + kr + 8 * q;
      if (vec && k < kend && i + 3 < D) {
        r[q] = *reinterpret_cast<const f32x4*>(X + (long long)k * ld + i);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[q][e] = (k < kend && i + e < D) ? X[(long long)k * ld + i + e] : 0.f;
      }
    }
  } else {  // 128 i-rows of TG_BK k: thread t -> row (t / (TG_BK/4)) + (1024/TG_BK) q, k 4(t % (TG_BK/4)) .. +3
    constexpr int KQ = TG_BK / 4, RS = 256 / KQ;
    const int ir = t / KQ, k = k0 + (t % KQ) * 4;
#pragma unroll
    for (int q = 0; q < TG_Q; ++q) {
      const int i = i0 + ir + RS * q;
      if (vec && i < D && k + 3 < kend) {
        r[q] = *reinterpret_cast<const f32x4*>(X + (long long)i * ld + k);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[q][e] = (i < D && k + e < kend) ? X[(long long)i * ld + k + e] : 0.f;
      }
    }
  }
}

template <bool KMAJ>
__device__ __forceinline__ void tg_store(float* S, int t, const f32x4 (&r)[TG_Q]) {
  if (KMAJ) {
    const int kr = t >> 5, i4 = (t & 31) * 4;
#pragma unroll
    for (int q = 0; q < TG_Q; ++q) *reinterpret_cast<f32x4*>(S + (kr + 8 * q) * TG_P + i4) = r[q];
  } else {
    constexpr int KQ = TG_BK / 4, RS = 256 / KQ;
    const int ir = t / KQ, k4 = (t % KQ) * 4;
#pragma unroll
    for (int q = 0; q < TG_Q; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) S[(k4 + e) * TG_P + ir + RS * q] = r[q][e];
  }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void tgemm_kernel(TGemmK p) {
  __shared__ __attribute__((aligned(16))) float As[2][TG_BK * TG_P];
  __shared__ __attribute__((aligned(16))) float Bs[2][TG_BK * TG_P];
  const TGemm& g = p.g;
  const int t = threadIdx.x;
  const int z = blockIdx.z, bat = z / p.ksplit, ks = z - bat * p.ksplit;
  const float* A = g.A + bat * g.sA;
  const float* B = g.B + bat * g.sB;
  const int m0 = blockIdx.x * TG_BM, n0 = blockIdx.y * TG_BN;
  const int kbeg = ks * p.kchunk, kend = min(g.K, kbeg + p.kchunk);
  const int nk = kend > kbeg ? (kend - kbeg + TG_BK - 1) / TG_BK : 0;
  const int w = t >> 6, l = t & 63, h = l >> 5, l32 = l & 31;
  const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  f32x4 ra[TG_Q], rb[TG_Q];
  if (nk > 0) {
    tg_load<TA>(A, g.lda, m0, g.M, kbeg, kend, p.vecA, t, ra);
    tg_load<!TB>(B, g.ldb, n0, g.N, kbeg, kend, p.vecB, t, rb);
    tg_store<TA>(As[0], t, ra);
    tg_store<!TB>(Bs[0], t, rb);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      const int k0 = kbeg + (kt + 1) * TG_BK;
      tg_load<TA>(A, g.lda, m0, g.M, k0, kend, p.vecA, t, ra);
      tg_load<!TB>(B, g.ldb, n0, g.N, k0, kend, p.vecB, t, rb);
    }
    const float* as = As[cur] + wm + l32;
    const float* bs = Bs[cur] + wn + l32;
#pragma unroll
    for (int s = 0; s < TG_BK / 2; ++s) {
      const int kk = (2 * s + h) * TG_P;
      const float a0 = as[kk], a1 = as[kk + 32], b0 = bs[kk], b1 = bs[kk + 32];
      acc[0][0] = mfma32(a0, b0, acc[0][0]);
      acc[0][1] = mfma32(a0, b1, acc[0][1]);
      acc[1][0] = mfma32(a1, b0, acc[1][0]);
      acc[1][1] = mfma32(a1, b1, acc[1][1]);
    }
    if (kt + 1 < nk) {
      tg_store<TA>(As[cur ^ 1], t, ra);
      tg_store<!TB>(Bs[cur ^ 1], t, rb);
    }
    __syncthreads();
  }
  float* C = g.C + bat * g.sC;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + 32 * j + l32;
      if (col >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + 32 * i + row32(r, h);
        if (row >= g.M) continue;
        const float v = acc[i][j][r];
        if (p.ksplit > 1) {
          p.part[((long long)z * g.M + row) * g.N + col] = v;
        } else {
          float o = g.alpha * (g.bias ? v + g.bias[col] : v);
          float* cp = C + (long long)row * g.ldc + col;
          if (g.beta != 0.f) o = fmaf(g.beta, *cp, o);
          *cp = o;
        }
      }
    }
}

// Weight-gradient product on bf16 matrix cores: C[M][N] = alpha (sum_k A[k][m] B[k][n]) (+ ...)
// for (ta, tb) = (1, 0), both operands stored k-major (k = the rows the gradient sums over).  A
// 16-deep k-tile of each operand is loaded one m (or n) column per thread -- eight scalar loads
// down k, coalesced across the lanes -- split into three bf16 pieces (common.h split3) and
// written m-major to LDS as one 16-byte chunk of 8 consecutive k per piece (the eval GEMM's
// chunk swizzle), so a lane reads its MFMA operand with one ds_read_b128; each 32 x 32 block
// takes the six v_mfma_f32_32x32x16_bf16 of mfma_x6.  Split-k partials as tgemm_kernel.
constexpr int X6_BM = 128, X6_BN = 128, X6_BK = 16;
#ifndef LG_X6T_PROBE
// tools/kbench_tgemm_x6t.hip only (0 in the library): 1 = no piece split, 2 = no MFMAs, 3 = no global
// loads past the first k-tile (timing probes; wrong results)
#define LG_X6T_PROBE 0
#endif

__global__ __launch_bounds__(256) void tgemm_x6t_kernel(TGemmK p) {
  // [stage][operand][piece][128 rows][16 k] bf16 = 2 x 2 x 3 x 4 KiB
  __shared__ __attribute__((aligned(16))) __bf16 S[2][2][3][X6_BM * X6_BK];
  const TGemm& g = p.g;
  const int t = threadIdx.x;
  const int z = blockIdx.z, bat = z / p.ksplit, ks = z - bat * p.ksplit;
  const float* A = g.A + bat * g.sA;
  const float* B = g.B + bat * g.sB;
  const int m0 = blockIdx.x * X6_BM, n0 = blockIdx.y * X6_BN;
  const int kbeg = ks * p.kchunk, kend = min(g.K, kbeg + p.kchunk);
  const int nk = kend > kbeg ? (kend - kbeg + X6_BK - 1) / X6_BK : 0;
  const int w = t >> 6, l = t & 63, half = l >> 5, l32 = l & 31;
  const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
  // staging: thread t owns column c = t & 127 of the tile and k-half kh = t >> 7 (8 rows)
  const int sc = t & 127, kh = t >> 7;
  const bool am = m0 + sc < g.M, bn = n0 + sc < g.N;
  // g.colsumA: the first column of tiles also sums its A column over the k range it stages
  // (fp32, in k order; the two k halves and the split-k partials combine in order after)
  const bool do_cs = g.colsumA != nullptr && blockIdx.y == 0;
  float csum = 0.f;
  float ra[8], rb[8];
  auto gload = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + 8 * kh + j;
      const bool kin = k < kend;
      ra[j] = (kin && am) ? A[(long long)k * g.lda + m0 + sc] : 0.f;
      rb[j] = (kin && bn) ? B[(long long)k * g.ldb + n0 + sc] : 0.f;
    }
    if (do_cs) {
#pragma unroll
      for (int j = 0; j < 8; ++j) csum += ra[j];
    }
  };
  auto sstore = [&](int st) {
    const int off = sc * X6_BK + ((kh ^ ((sc >> 3) & 1)) * 8);
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const float* r = o ? rb : ra;
      bf16x8 h, m, lo;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 a, b, c;
#if LG_X6T_PROBE == 1
        a = b = c = (__bf16)r[e];
#else
        split3(r[e], a, b, c);
#endif
        h[e] = a;
        m[e] = b;
        lo[e] = c;
      }
      *reinterpret_cast<bf16x8*>(&S[st][o][0][off]) = h;
      *reinterpret_cast<bf16x8*>(&S[st][o][1][off]) = m;
      *reinterpret_cast<bf16x8*>(&S[st][o][2][off]) = lo;
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  if (nk > 0) {
    gload(kbeg);
    sstore(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk && (LG_X6T_PROBE != 3 || kt == 0)) gload(kbeg + (kt + 1) * X6_BK);
    bf16x8 fa[2][3], fb[2][3];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ra_ = wm + 32 * i + l32, rb_ = wn + 32 * i + l32;
        fa[i][pc] = *reinterpret_cast<const bf16x8*>(&S[cur][0][pc][ra_ * X6_BK + ((half ^ ((ra_ >> 3) & 1)) * 8)]);
        fb[i][pc] = *reinterpret_cast<const bf16x8*>(&S[cur][1][pc][rb_ * X6_BK + ((half ^ ((rb_ >> 3) & 1)) * 8)]);
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#if LG_X6T_PROBE == 2
        acc[i][j][0] += (float)fa[i][0][0] + (float)fa[i][1][1] + (float)fa[i][2][2] + (float)fb[j][0][3] +
                        (float)fb[j][1][4] + (float)fb[j][2][5];
#else
        acc[i][j] = mfma_x6(fa[i][0], fa[i][1], fa[i][2], fb[j][0], fb[j][1], fb[j][2], acc[i][j]);
#endif
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }
  if (do_cs) {  // k half 1 hands its sums to k half 0 through the (now idle) staging buffer
    float* red = reinterpret_cast<float*>(&S[0][0][0][0]);
    if (kh == 1) red[sc] = csum;
    __syncthreads();
    if (kh == 0 && am) {
      const float v = csum + red[sc];
      if (p.ksplit > 1) p.cpart[(long long)z * g.M + m0 + sc] = v;
      else g.colsumA[(long long)bat * g.M + m0 + sc] = v;
    }
  }
  float* C = g.C + bat * g.sC;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + 32 * j + l32;
      if (col >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + 32 * i + row32(r, half);
        if (row >= g.M) continue;
        const float v = acc[i][j][r];
        if (p.ksplit > 1) {
          p.part[((long long)z * g.M + row) * g.N + col] = v;
        } else {
          float o = g.alpha * (g.bias ? v + g.bias[col] : v);
          float* cp = C + (long long)row * g.ldc + col;
          if (g.beta != 0.f) o = fmaf(g.beta, *cp, o);
          *cp = o;
        }
      }
    }
}

// The same product with 16-byte loads (round 5): the k-major operands are loaded as rows of the
// tile -- thread t takes columns 4 (t & 31) .. +3 of k-rows t >> 5 and 8 + (t >> 5) of both operands
// (four global_load_dwordx4 per k-tile instead of sixteen dword loads) -- split into the three bf16
// pieces and written k-major, [k][128 columns] per piece (256-byte rows, 16-byte chunks XOR-swizzled
// as the guide's dual-use image (b)), and the MFMA fragments (8 consecutive k of one column) come
// out of ds_read_b64_tr_b16 (two per fragment and piece).  Same k order per accumulator.
typedef short tg_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x4 tg_tr_read(const __bf16* p) {
  const tg_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tg_s16x4*)(p));
  return __builtin_bit_cast(bf16x4, v);
}
// byte offset (in bf16 elements) of 16-byte chunk ch of k-row r in a [16][128] piece image
__device__ __forceinline__ int tgv_off(int r, int ch) { return 128 * r + 8 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); }

__global__ __launch_bounds__(256) void tgemm_x6tv_kernel(TGemmK p) {
  __shared__ __attribute__((aligned(16))) __bf16 S[2][2][3][X6_BK * X6_BM];  // [stage][operand][piece][k][col]
  const TGemm& g = p.g;
  const int t = threadIdx.x;
  // XCD-aware tile order: workgroups are dispatched round-robin over the 8 XCDs, so a contiguous
  // range of tiles -- whole k-chunks with all their (m, n) tiles, which read the same operand rows --
  // goes to one XCD and shares its L2
  const int nx = gridDim.x, ny = gridDim.y;
  const int ntile = nx * ny * gridDim.z;
  const int lin = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
  const int xcd = lin & 7, loc = lin >> 3, base8 = ntile >> 3, extra8 = ntile & 7;
  const int tile = xcd * base8 + (xcd < extra8 ? xcd : extra8) + loc;
  const int bx = tile % nx, by = (tile / nx) % ny, z = tile / (nx * ny);
  const int bat = z / p.ksplit, ks = z - bat * p.ksplit;
  const float* A = g.A + bat * g.sA;
  const float* B = g.B + bat * g.sB;
  const int m0 = bx * X6_BM, n0 = by * X6_BN;
  // a two-source B (g.B1): tiles at n0 >= N0 read B1 (N0 % 128 == 0, so no tile straddles)
  const bool b1 = g.B1 != nullptr && n0 >= g.N0;
  const float* Bt = b1 ? g.B1 + (n0 - g.N0) : B + n0;
  const long long ldbt = b1 ? g.ldb1 : g.ldb;
  const int kbeg = ks * p.kchunk, kend = min(g.K, kbeg + p.kchunk);
  const int nk = kend > kbeg ? (kend - kbeg + X6_BK - 1) / X6_BK : 0;
  const int w = t >> 6, l = t & 63, half = l >> 5, l32 = l & 31;
  const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
  const int c4 = 4 * (t & 31), kr = t >> 5;  // staging: columns c4 .. c4 + 3, k-rows kr and kr + 8
  const bool am = m0 + c4 < g.M, bn = n0 + c4 < g.N;  // M, N % 4 == 0 (launcher): whole quads in or out
  const bool do_cs = g.colsumA != nullptr && by == 0;
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
  f32x4 ra[2], rb[2];
  auto gload = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + kr + 8 * j;
      const bool kin = k < kend;
      ra[j] = (kin && am) ? *reinterpret_cast<const f32x4*>(A + (long long)k * g.lda + m0 + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
      rb[j] = (kin && bn) ? *reinterpret_cast<const f32x4*>(Bt + (long long)k * ldbt + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (do_cs) csum += ra[0] + ra[1];  // per column: this thread's two rows, k-rows in order of the tile
  };
  auto sstore = [&](int st) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x4& r = o ? rb[j] : ra[j];
        bf16x4 h, m, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          __bf16 a, b, c;
          split3(r[e], a, b, c);
          h[e] = a;
          m[e] = b;
          lo[e] = c;
        }
        const int off = tgv_off(kr + 8 * j, c4 >> 3) + (c4 & 4);
        *reinterpret_cast<bf16x4*>(&S[st][o][0][off]) = h;
        *reinterpret_cast<bf16x4*>(&S[st][o][1][off]) = m;
        *reinterpret_cast<bf16x4*>(&S[st][o][2][off]) = lo;
      }
  };
  // fragment (8 consecutive k of column `col`, k-half `half`) of a piece image: the lane of the
  // 16-lane group that reads block (k0 + q, columns 16 cb ..) supplies row k0 + q, chunk 2 cb + (p >> 1)
  const int gq = (l & 15) >> 2, gp = l & 3;
  auto frag = [&](const __bf16* img, int col0) {  // col0: first of the 32 columns of this MFMA tile
    const int cb = (col0 + 16 * ((l >> 4) & 1)) >> 4;  // 16-column block of this lane's group
    bf16x8 f;
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      const int k0 = 8 * half + 4 * rd;
      const bf16x4 v = tg_tr_read(img + tgv_off(k0 + gq, 2 * cb + (gp >> 1)) + 4 * (gp & 1));
#pragma unroll
      for (int e = 0; e < 4; ++e) f[4 * rd + e] = v[e];
    }
    return f;
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  if (nk > 0) {
    gload(kbeg);
    sstore(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload(kbeg + (kt + 1) * X6_BK);
    bf16x8 fa[2][3], fb[2][3];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i][pc] = frag(&S[cur][0][pc][0], wm + 32 * i);
        fb[i][pc] = frag(&S[cur][1][pc][0], wn + 32 * i);
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = mfma_x6(fa[i][0], fa[i][1], fa[i][2], fb[j][0], fb[j][1], fb[j][2], acc[i][j]);
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }
  if (do_cs) {  // the eight k-row groups' column sums, in group order, through the idle staging buffer
    float* red = reinterpret_cast<float*>(&S[0][0][0][0]);  // [8][128]
#pragma unroll
    for (int e = 0; e < 4; ++e) red[kr * 128 + c4 + e] = csum[e];
    __syncthreads();
    if (t < 128 && m0 + t < g.M) {
      float v = red[t];
      for (int q = 1; q < 8; ++q) v += red[q * 128 + t];
      if (p.ksplit > 1) p.cpart[(long long)z * g.M + m0 + t] = v;
      else g.colsumA[(long long)bat * g.M + m0 + t] = v;
    }
  }
  float* C = g.C + bat * g.sC;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + 32 * j + l32;
      if (col >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + 32 * i + row32(r, half);
        if (row >= g.M) continue;
        const float v = acc[i][j][r];
        if (p.ksplit > 1) {
          p.part[((long long)z * g.M + row) * g.N + col] = v;
        } else {
          float o = g.alpha * (g.bias ? v + g.bias[col] : v);
          float* cp = C + (long long)row * g.ldc + col;
          if (g.beta != 0.f) o = fmaf(g.beta, *cp, o);
          *cp = o;
        }
      }
    }
}

// the column sums of A from their split-k partials: one wave per (batch, column), lanes strided
// over the splits, then a fixed-order wave reduction (workgroup `wg` of that part)
__device__ __forceinline__ void tgemm_colsum_reduce(const TGemmK& p, long long wg) {
  const TGemm& g = p.g;
  const long long w = wg * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= (long long)g.M * g.batch) return;
  const int bat = (int)(w / g.M), m = (int)(w - (long long)bat * g.M);
  const float* cs = p.cpart + (long long)bat * p.ksplit * g.M + m;
  float c = 0.f;
  for (int s = lane; s < p.ksplit; s += 64) c += cs[(long long)s * g.M];
  c = wave_sum(c);
  if (lane == 0) g.colsumA[w] = c;
}

// C from the split-k partials (workgroups < nmain); workgroups from nmain on reduce the column-sum
// partials (g.colsumA) -- one launch for both
__global__ __launch_bounds__(256) void tgemm_reduce_kernel(TGemmK p, int nmain) {
  if ((int)blockIdx.x >= nmain) {
    tgemm_colsum_reduce(p, (long long)blockIdx.x - nmain);
    return;
  }
  const TGemm& g = p.g;
  const long long MN = (long long)g.M * g.N;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= MN * g.batch) return;
  const int bat = (int)(idx / MN);
  const long long e = idx - bat * MN;
  const int row = (int)(e / g.N), col = (int)(e - (long long)row * g.N);
  const float* src = p.part + (long long)bat * p.ksplit * MN + e;
  float v = 0.f;
  int s = 0;
  for (; s + 8 <= p.ksplit; s += 8) {  // eight loads in flight, then the adds in split order
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = src[(long long)(s + u) * MN];
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  for (; s < p.ksplit; ++s) v += src[(long long)s * MN];
  float o = g.alpha * (g.bias ? v + g.bias[col] : v);
  float* cp = g.C + bat * g.sC + (long long)row * g.ldc + col;
  if (g.beta != 0.f) o = fmaf(g.beta, *cp, o);
  *cp = o;
}

int tgemm_split(int M, int N, int K, int batch, int& kchunk) {
  const long long tiles = (long long)((M + TG_BM - 1) / TG_BM) * ((N + TG_BN - 1) / TG_BN) * batch;
  int ks = 1;
  if (tiles < 512 && K >= 1024) {
    ks = (int)std::min<long long>((1024 + tiles - 1) / tiles, K / 512);
    ks = std::max(ks, 1);
    // bound the partial buffer (32 Mi floats)
    while (ks > 1 && (long long)ks * M * N * batch > (32ll << 20)) --ks;
  }
  kchunk = ((K + ks - 1) / ks + TG_BK - 1) / TG_BK * TG_BK;
  ks = (K + kchunk - 1) / kchunk;
  return std::max(ks, 1);
}

// ============================================================================ attention
// Forward: a workgroup = W waves x 32 queries of one (pair, head); the query sits on the MFMA
// lane (S^T = K Q^T), so the online softmax runs in-register per lane (the two lane halves hold
// different keys of the same query: one v_permlane32_swap per max) and P^T is directly the B
// operand of O^T = V^T P^T (the permuted key order row32 on both operands).
// Both products run on bf16 matrix cores (bf16x6, common.h): S^T = K Q^T and O^T = V^T P^T as six
// v_mfma_f32_32x32x16_bf16 per 32 x 32 x 16 block, every operand split into three bf16 pieces
// (the fp32-accurate product at the bf16 rate).  The query's pieces sit in registers (scaled by
// scale log2 e before the split); a 64-key tile of K is staged [key][dim] and of V
// transposed [dim][key] as three bf16 planes each, 16-byte chunks XOR-swizzled by row.  The V^T
// chunks hold the keys in the accumulator's row32 order, so P^T goes from the S^T accumulators
// straight into the B operand (split per value).  One LDS buffer: the next tile waits in
// registers and lands between two barriers.
__device__ __forceinline__ int x6_sw(int row, int chunk) { return (chunk ^ (row & 7)) * 8; }

template <int W>  // waves per workgroup (32 queries each): every K / V tile is split once per workgroup
__global__ __launch_bounds__(64 * W, 8 / W) void tattn_fwd_x6_kernel(TAttn a) {
  __shared__ __attribute__((aligned(16))) __bf16 Kp[3][64 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 Vt[3][64 * 64];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, h = l >> 5, l32 = l & 31;
  const int item = blockIdx.y, b = item / a.H, hd = item - b * a.H;
  const float* Q = a.Q + (long long)b * a.Nq * a.ldq + hd * 64;
  const float* K = a.K + (long long)b * a.Nk * a.ldk + hd * 64;
  const float* V = a.V + (long long)b * a.Nk * a.ldv + hd * 64;
  const int qrow = blockIdx.x * (32 * W) + w * 32 + l32;
  const bool qv = qrow < a.Nq;
  const float c = a.scale * kLog2e;
  bf16x8 qf[4][3];  // dims 16 ks + 8 h .. +7 of this lane's query, three pieces
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (qv) {
      const float* qp = Q + (long long)qrow * a.ldq + 16 * ks + 8 * h;
      v0 = *reinterpret_cast<const f32x4*>(qp);
      v1 = *reinterpret_cast<const f32x4*>(qp + 4);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      __bf16 x0, x1, x2;
      split3((e < 4 ? v0[e] : v1[e - 4]) * c, x0, x1, x2);
      qf[ks][0][e] = x0;
      qf[ks][1][e] = x1;
      qf[ks][2][e] = x2;
    }
  }
  // staging, a 64-key tile per step:
  // W = 4: K row t >> 2, dims 16 (t & 3) ..; V^T row (dim) t & 63, key chunks 2 (t >> 6), +1
  // W = 8: K row t >> 3, dims 8 (t & 7) ..;  V^T row (dim) t & 63, key chunk t >> 6
  constexpr int KQ = 16 / W, VC = 8 / W;  // float4 loads of K per thread, V^T chunks per thread
  const int kr = t / (16 / KQ), kc = t % (16 / KQ), vd = t & 63, vc = VC * (t >> 6);
  f32x4 rk[KQ];
  float rv[8 * VC];
  auto chunk_key = [](int ch, int e) {  // key (within the tile) of element e of V^T chunk ch
    return 32 * (ch >> 2) + row32(8 * ((ch >> 1) & 1) + e, ch & 1);
  };
  auto gload = [&](int kt) {
    const int key = kt * 64 + kr;
#pragma unroll
    for (int q = 0; q < KQ; ++q)
      rk[q] = key < a.Nk ? *reinterpret_cast<const f32x4*>(K + (long long)key * a.ldk + 4 * KQ * kc + 4 * q)
                         : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < VC; ++cc)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k2 = kt * 64 + chunk_key(vc + cc, e);
        rv[8 * cc + e] = k2 < a.Nk ? V[(long long)k2 * a.ldv + vd] : 0.f;
      }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int hh = 0; hh < KQ / 2; ++hh) {
      bf16x8 p0, p1, p2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 x0, x1, x2;
        split3(rk[2 * hh + (e >> 2)][e & 3], x0, x1, x2);
        p0[e] = x0;
        p1[e] = x1;
        p2[e] = x2;
      }
      const int off = kr * 64 + x6_sw(kr, (KQ / 2) * kc + hh);
      *reinterpret_cast<bf16x8*>(&Kp[0][off]) = p0;
      *reinterpret_cast<bf16x8*>(&Kp[1][off]) = p1;
      *reinterpret_cast<bf16x8*>(&Kp[2][off]) = p2;
    }
#pragma unroll
    for (int cc = 0; cc < VC; ++cc) {
      bf16x8 p0, p1, p2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 x0, x1, x2;
        split3(rv[8 * cc + e], x0, x1, x2);
        p0[e] = x0;
        p1[e] = x1;
        p2[e] = x2;
      }
      const int off = vd * 64 + x6_sw(vd, vc + cc);
      *reinterpret_cast<bf16x8*>(&Vt[0][off]) = p0;
      *reinterpret_cast<bf16x8*>(&Vt[1][off]) = p1;
      *reinterpret_cast<bf16x8*>(&Vt[2][off]) = p2;
    }
  };
  const int nkt = (a.Nk + 63) / 64;
  float m = -INFINITY, lsum = 0.f;
  f32x16 ot[2] = {zero16(), zero16()};
  gload(0);
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();  // every wave is done with the previous tile
    sstore();
    __syncthreads();
    if (kt + 1 < nkt) gload(kt + 1);
    f32x16 st[2] = {zero16(), zero16()};
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int row = 32 * tt + l32, off = row * 64 + x6_sw(row, 2 * ks + h);
        const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(&Kp[0][off]);
        const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(&Kp[1][off]);
        const bf16x8 k2 = *reinterpret_cast<const bf16x8*>(&Kp[2][off]);
        st[tt] = mfma_x6(k0, k1, k2, qf[ks][0], qf[ks][1], qf[ks][2], st[tt]);
      }
    if (kt * 64 + 64 > a.Nk) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * 64 + 32 * tt + row32(r, h) >= a.Nk) st[tt][r] = -INFINITY;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[tt][r]);
    mx = max_xor32(mx);
    const float mn = fmaxf(m, mx);
    const float base = mn == -INFINITY ? 0.f : mn;
    const float f = __builtin_amdgcn_exp2f(m - base);  // v_exp_f32; exp2(-inf) = 0
    lsum *= f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      ot[0][r] *= f;
      ot[1][r] *= f;
    }
    m = mn;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {  // keys of step s2: st[s2 >> 1][8 (s2 & 1) + e]
      bf16x8 pb0, pb1, pb2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float pv = __builtin_amdgcn_exp2f(st[s2 >> 1][8 * (s2 & 1) + e] - base);
        lsum += pv;
        __bf16 x0, x1, x2;
        split3(pv, x0, x1, x2);
        pb0[e] = x0;
        pb1[e] = x1;
        pb2[e] = x2;
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int row = 32 * dt + l32, off = row * 64 + x6_sw(row, 2 * s2 + h);
        const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(&Vt[0][off]);
        const bf16x8 v1 = *reinterpret_cast<const bf16x8*>(&Vt[1][off]);
        const bf16x8 v2 = *reinterpret_cast<const bf16x8*>(&Vt[2][off]);
        ot[dt] = mfma_x6(v0, v1, v2, pb0, pb1, pb2, ot[dt]);
      }
    }
  }
  lsum = sum_xor32(lsum);
  if (!qv) return;
  const float inv = 1.f / lsum;
  float* O = a.O + ((long long)b * a.Nq + qrow) * a.ldo + hd * 64;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ot[dt][4 * g4 + e] * inv;
      *reinterpret_cast<f32x4*>(O + 32 * dt + 8 * g4 + 4 * h) = v;
    }
  if (h == 0) a.lse[(long long)item * a.Nq + qrow] = m + log2f(lsum);
}

// Backward: a workgroup = 8 waves x 32 keys (256 keys) of one (pair, head); the key sits on the
// lane, so S and dP come out with their columns = keys and are directly the B operands of
// dV^T += dO^T P and dK^T += Q^T dS (permuted query order row32 on both operands).  Row constants
// seed the accumulators (S' = Q (cK)^T - lse, dP' = dO V^T - delta), so p = exp2(S') and
// dS = p * dP' need no further VALU.  dQ: dS crosses LDS once; each wave owns one 16 x 16 tile
// (16 queries x 16 dims) of the 32 x 64 dQ tile and sums it over all 256 keys with
// v_mfma_f32_16x16x4_f32, so every dQ element gets ONE float atomic per workgroup (four 64-B row
// segments per instruction).  Against 4 waves x 128 keys with 32 x 32 dQ quarters: a quarter of
// the atomic bytes, and two waves per SIMD.
constexpr int TB_W = 8, TB_KEYS = 32 * TB_W;
constexpr int TB_DP = TB_KEYS + 4;

// S, dP, dV^T and dK^T run on bf16 matrix cores (bf16x6, common.h): the key's
// K (scaled by scale log2 e) and V sit in registers as three bf16 pieces; a query tile is staged
// [query][dim] (A operand of S = Q K^T and dP = dO V^T) and [dim][query] (A operand of dV^T and
// dK^T, the queries of each 16-byte chunk in the row32 order the S / dP accumulators hold them
// in), three bf16 planes each.  P and dS go from the accumulators into the B operands split per
// value.  dQ stays on v_mfma_f32_16x16x4_f32 over fp32 dS / K.
__device__ __forceinline__ int x6_swt(int row, int chunk) { return (chunk ^ ((row >> 2) & 3)) * 8; }

#ifndef LG_TB_PROBE
// tools/kbench_tattn.hip only (0 in the library): 1 = the dQ float atomics as plain stores, 2 = no
// dQ products and no dQ atomics (timing probes; wrong dQ)
#define LG_TB_PROBE 0
#endif

__global__ __launch_bounds__(64 * TB_W) void tattn_bwd_x6_kernel(TAttn a) {
  __shared__ __attribute__((aligned(16))) __bf16 Qp[3][32 * 64];   // [query][dim]
  __shared__ __attribute__((aligned(16))) __bf16 dOp[3][32 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 QTp[3][64 * 32];  // [dim][query, row32 chunks]
  __shared__ __attribute__((aligned(16))) __bf16 dOTp[3][64 * 32];
  __shared__ __attribute__((aligned(16))) float KT[64 * TB_DP];  // the workgroup's keys, [dim][key]
  __shared__ __attribute__((aligned(16))) float dSs[32 * TB_DP];
  __shared__ float lse_s[32], del_s[32];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, h = l >> 5, l32 = l & 31;
  const int item = blockIdx.y, b = item / a.H, hd = item - b * a.H;
  const float* Q = a.Q + (long long)b * a.Nq * a.ldq + hd * 64;
  const float* dO = a.dO + (long long)b * a.Nq * a.ldo + hd * 64;
  const float* K = a.K + (long long)b * a.Nk * a.ldk + hd * 64;
  const float* V = a.V + (long long)b * a.Nk * a.ldv + hd * 64;
  const float* lse = a.lse + (long long)item * a.Nq;
  const float* del = a.delta + (long long)item * a.Nq;
  const int kb0 = blockIdx.x * TB_KEYS;
  const int key = kb0 + w * 32 + l32;
  const bool kv = key < a.Nk;
  const float c = a.scale * kLog2e;
  bf16x8 kf[4][3];  // dims 16 ks + 8 h .. +7 of this lane's key: K (scaled) in three pieces,
  f32x4 vr[4][2];   // V in fp32, split per query tile
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    f32x4 k0 = {0.f, 0.f, 0.f, 0.f}, k1 = k0, v0 = k0, v1 = k0;
    if (kv) {
      const float* kp = K + (long long)key * a.ldk + 16 * ks + 8 * h;
      const float* vp = V + (long long)key * a.ldv + 16 * ks + 8 * h;
      k0 = *reinterpret_cast<const f32x4*>(kp);
      k1 = *reinterpret_cast<const f32x4*>(kp + 4);
      v0 = *reinterpret_cast<const f32x4*>(vp);
      v1 = *reinterpret_cast<const f32x4*>(vp + 4);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      __bf16 x0, x1, x2;
      split3((e < 4 ? k0[e] : k1[e - 4]) * c, x0, x1, x2);
      kf[ks][0][e] = x0;
      kf[ks][1][e] = x1;
      kf[ks][2][e] = x2;
    }
    vr[ks][0] = v0;
    vr[ks][1] = v1;
  }
  {  // the workgroup's 256 keys (unscaled) for dQ, transposed
    const int sr = t >> 4, sc = (t & 15) * 4;
#pragma unroll
    for (int q = 0; q < TB_KEYS / 32; ++q) {
      const int k = kb0 + sr + 32 * q;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (k < a.Nk) v = *reinterpret_cast<const f32x4*>(K + (long long)k * a.ldk + sc);
#pragma unroll
      for (int e = 0; e < 4; ++e) KT[(sc + e) * TB_DP + sr + 32 * q] = v[e];
    }
  }
  // query tiles: thread t -> query sr = t >> 4, dims sc = 4 (t & 15) .. +3; in the transposed
  // planes query sr sits in chunk 2 (sr >> 4) + ((sr >> 2) & 1) at position (sr & 3) + 4 ((sr >> 3) & 1)
  const int sr = t >> 4, sc = (t & 15) * 4;
  const int tch = 2 * (sr >> 4) + ((sr >> 2) & 1), tpos = (sr & 3) + 4 * ((sr >> 3) & 1);
  f32x4 rq, rd;
  float rl = 0.f, rdl = 0.f;
  auto load_q = [&](int qt) {
    const int qi = qt * 32 + sr;
    if (qi < a.Nq) {
      rq = *reinterpret_cast<const f32x4*>(Q + (long long)qi * a.ldq + sc);
      rd = *reinterpret_cast<const f32x4*>(dO + (long long)qi * a.ldo + sc);
    } else {
      rq = f32x4{0.f, 0.f, 0.f, 0.f};
      rd = rq;
    }
    if (t < 32) {
      const int qj = qt * 32 + t;
      rl = qj < a.Nq ? lse[qj] : INFINITY;  // padded queries: p = exp2(-inf) = 0
      rdl = qj < a.Nq ? del[qj] : 0.f;
    }
  };
  auto store_q = [&]() {
    const int off = sr * 64 + x6_sw(sr, sc >> 3) + (sc & 4);
    bf16x4 q0, q1, q2, d0, d1, d2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      __bf16 x0, x1, x2;
      split3(rq[e], x0, x1, x2);
      q0[e] = x0;
      q1[e] = x1;
      q2[e] = x2;
      const int to = (sc + e) * 32 + x6_swt(sc + e, tch) + tpos;
      QTp[0][to] = x0;
      QTp[1][to] = x1;
      QTp[2][to] = x2;
      split3(rd[e], x0, x1, x2);
      d0[e] = x0;
      d1[e] = x1;
      d2[e] = x2;
      dOTp[0][to] = x0;
      dOTp[1][to] = x1;
      dOTp[2][to] = x2;
    }
    *reinterpret_cast<bf16x4*>(&Qp[0][off]) = q0;
    *reinterpret_cast<bf16x4*>(&Qp[1][off]) = q1;
    *reinterpret_cast<bf16x4*>(&Qp[2][off]) = q2;
    *reinterpret_cast<bf16x4*>(&dOp[0][off]) = d0;
    *reinterpret_cast<bf16x4*>(&dOp[1][off]) = d1;
    *reinterpret_cast<bf16x4*>(&dOp[2][off]) = d2;
    if (t < 32) {
      lse_s[t] = rl;
      del_s[t] = rdl;
    }
  };
  f32x16 dvt[2] = {zero16(), zero16()}, dkt[2] = {zero16(), zero16()};
  const int nqt = (a.Nq + 31) / 32;
  const int qh = w & 1, dq = w >> 1;  // this wave's dQ tile: queries 16 qh .., dims 16 dq ..
  const int l16 = l & 15, lk = l >> 4;
  float* dQ = a.dQ + (long long)b * a.Nq * a.ldq + hd * 64 + 16 * dq + l16;
  load_q(0);
  store_q();
  __syncthreads();
  for (int qt = 0; qt < nqt; ++qt) {
    f32x16 sacc, pacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sacc[r] = -lse_s[row32(r, h)];
      pacc[r] = -del_s[row32(r, h)];
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int off = l32 * 64 + x6_sw(l32, 2 * ks + h);
      const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(&Qp[0][off]);
      const bf16x8 q1 = *reinterpret_cast<const bf16x8*>(&Qp[1][off]);
      const bf16x8 q2 = *reinterpret_cast<const bf16x8*>(&Qp[2][off]);
      sacc = mfma_x6(q0, q1, q2, kf[ks][0], kf[ks][1], kf[ks][2], sacc);
      const bf16x8 d0 = *reinterpret_cast<const bf16x8*>(&dOp[0][off]);
      const bf16x8 d1 = *reinterpret_cast<const bf16x8*>(&dOp[1][off]);
      const bf16x8 d2 = *reinterpret_cast<const bf16x8*>(&dOp[2][off]);
      bf16x8 v0, v1, v2;
      asm volatile("" : "+v"(vr[ks][0]), "+v"(vr[ks][1]));  // split per tile, not hoisted out of the loop
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 x0, x1, x2;
        split3(vr[ks][e >> 2][e & 3], x0, x1, x2);
        v0[e] = x0;
        v1[e] = x1;
        v2[e] = x2;
      }
      pacc = mfma_x6(d0, d1, d2, v0, v1, v2, pacc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = kv ? __builtin_amdgcn_exp2f(sacc[r]) : 0.f;  // v_exp_f32 (tiny p flush to 0)
      sacc[r] = p;
      pacc[r] *= p;  // dS (w.r.t. the scaled scores)
      dSs[row32(r, h) * TB_DP + w * 32 + l32] = pacc[r];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // queries of step s: accumulator values 8 s .. 8 s + 7
      bf16x8 p0, p1, p2, g0, g1, g2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 x0, x1, x2;
        split3(sacc[8 * s + e], x0, x1, x2);
        p0[e] = x0;
        p1[e] = x1;
        p2[e] = x2;
        split3(pacc[8 * s + e], x0, x1, x2);
        g0[e] = x0;
        g1[e] = x1;
        g2[e] = x2;
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int row = 32 * dt + l32, off = row * 32 + x6_swt(row, 2 * s + h);
        const bf16x8 o0 = *reinterpret_cast<const bf16x8*>(&dOTp[0][off]);
        const bf16x8 o1 = *reinterpret_cast<const bf16x8*>(&dOTp[1][off]);
        const bf16x8 o2 = *reinterpret_cast<const bf16x8*>(&dOTp[2][off]);
        dvt[dt] = mfma_x6(o0, o1, o2, p0, p1, p2, dvt[dt]);
        const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(&QTp[0][off]);
        const bf16x8 q1 = *reinterpret_cast<const bf16x8*>(&QTp[1][off]);
        const bf16x8 q2 = *reinterpret_cast<const bf16x8*>(&QTp[2][off]);
        dkt[dt] = mfma_x6(q0, q1, q2, g0, g1, g2, dkt[dt]);
      }
    }
    __syncthreads();
    if (qt + 1 < nqt) load_q(qt + 1);  // lands under the dQ products
    f32x4 qacc = {0.f, 0.f, 0.f, 0.f};  // k index lk of step s: key 64 lk + s (16-byte reads of 4 steps)
    const float* ds_row = dSs + (16 * qh + l16) * TB_DP + 64 * lk;
    const float* k_row = KT + (16 * dq + l16) * TB_DP + 64 * lk;
#if LG_TB_PROBE != 2
#pragma unroll 4
    for (int s4 = 0; s4 < TB_KEYS / 16; ++s4) {
      const f32x4 dv = *reinterpret_cast<const f32x4*>(ds_row + 4 * s4);
      const f32x4 kv4 = *reinterpret_cast<const f32x4*>(k_row + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) qacc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[e], kv4[e], qacc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = qt * 32 + 16 * qh + 4 * lk + r;
#if LG_TB_PROBE == 1
      if (qi < a.Nq) dQ[(long long)qi * a.ldq] = qacc[r] * a.scale;
#else
      if (qi < a.Nq) atomicAdd(dQ + (long long)qi * a.ldq, qacc[r] * a.scale);
#endif
    }
#else
    asm volatile("" ::"v"(ds_row), "v"(k_row));
#endif
    if (qt + 1 < nqt) store_q();  // every wave is past this tile's reads (barrier above)
    __syncthreads();
  }
  if (!kv) return;
  float* dK = a.dK + ((long long)b * a.Nk + key) * a.ldk + hd * 64;
  float* dV = a.dV + ((long long)b * a.Nk + key) * a.ldv + hd * 64;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = 32 * dt + 8 * g4 + 4 * h;
      f32x4 vk, vv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vk[e] = dkt[dt][4 * g4 + e] * a.scale;
        vv[e] = dvt[dt][4 * g4 + e];
      }
      if (a.accum_kv) {
        vk += *reinterpret_cast<const f32x4*>(dK + d0);
        vv += *reinterpret_cast<const f32x4*>(dV + d0);
      }
      *reinterpret_cast<f32x4*>(dK + d0) = vk;
      *reinterpret_cast<f32x4*>(dV + d0) = vv;
    }
}

// one wave per query row: lanes 16h'..16h'+15 hold head h' (4 columns each)
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* O, const float* dO, int ldo, int B, int H, int Nq,
                                                         float* delta) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= B * Nq) return;
  const int b = row / Nq, q = row - b * Nq;
  float s = 0.f;
  if (4 * l < 64 * H) {
    const f32x4 o = *reinterpret_cast<const f32x4*>(O + (long long)row * ldo + 4 * l);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dO + (long long)row * ldo + 4 * l);
    s = (o[0] * d[0] + o[1] * d[1]) + (o[2] * d[2] + o[3] * d[3]);
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  const int hh = l >> 4;
  if ((l & 15) == 0 && hh < H) delta[((long long)b * H + hh) * Nq + q] = s;
}

// ============================================================================ rotary
// thread per (row, head, frequency f): dims 2f, 2f+1 of q, k, v are 6 consecutive floats of the
// reference layout (column h*192 + d*3 + t)
__global__ __launch_bounds__(256) void rotary_split_kernel(const float* qkv, const float* cosb, const float* sinb,
                                                           int R, int H, float* Q, float* K, float* V) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)R * H * 32) return;
  const int f = (int)(id & 31);
  const long long rh = id >> 5;
  const int hd = (int)(rh % H);
  const long long row = rh / H;
  const float* x = qkv + row * (192ll * H) + hd * 192 + 6 * f;
  const float c = cosb[row * 32 + f], s = sinb[row * 32 + f];
  const float q0 = x[0], k0 = x[1], v0 = x[2], q1 = x[3], k1 = x[4], v1 = x[5];
  const long long o = row * (64ll * H) + hd * 64 + 2 * f;
  // t * cos + rotate_half(t) * sin (lightglue.py:36-43), unfused like the reference's ATen ops
  *reinterpret_cast<f32x2*>(Q + o) = f32x2{__fadd_rn(__fmul_rn(q0, c), __fmul_rn(-q1, s)), __fadd_rn(__fmul_rn(q1, c), __fmul_rn(q0, s))};
  *reinterpret_cast<f32x2*>(K + o) = f32x2{__fadd_rn(__fmul_rn(k0, c), __fmul_rn(-k1, s)), __fadd_rn(__fmul_rn(k1, c), __fmul_rn(k0, s))};
  *reinterpret_cast<f32x2*>(V + o) = f32x2{v0, v1};
}

// thread per (row, f), looping over heads: gQKV and the encoding gradients (no atomics)
__global__ __launch_bounds__(256) void rotary_split_bwd_kernel(const float* gQ, const float* gK, const float* gV,
                                                               const float* Q, const float* K, const float* cosb,
                                                               const float* sinb, int R, int H, float* gQKV,
                                                               float* gcos, float* gsin) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)R * 32) return;
  const int f = (int)(id & 31);
  const long long row = id >> 5;
  const float c = cosb[id], s = sinb[id];
  float gc = 0.f, gs = 0.f;
  for (int hd = 0; hd < H; ++hd) {
    const long long o = row * (64ll * H) + hd * 64 + 2 * f;
    const f32x2 gq = *reinterpret_cast<const f32x2*>(gQ + o), gk = *reinterpret_cast<const f32x2*>(gK + o);
    const f32x2 gv = *reinterpret_cast<const f32x2*>(gV + o);
    const f32x2 qr = *reinterpret_cast<const f32x2*>(Q + o), kr = *reinterpret_cast<const f32x2*>(K + o);
    // pre-rotation values t = R(-theta) out
    const float q0 = qr[0] * c + qr[1] * s, q1 = qr[1] * c - qr[0] * s;
    const float k0 = kr[0] * c + kr[1] * s, k1 = kr[1] * c - kr[0] * s;
    gc += gq[0] * q0 + gq[1] * q1 + gk[0] * k0 + gk[1] * k1;
    gs += gq[1] * q0 - gq[0] * q1 + gk[1] * k0 - gk[0] * k1;
    float* x = gQKV + row * (192ll * H) + hd * 192 + 6 * f;
    x[0] = gq[0] * c + gq[1] * s;
    x[1] = gk[0] * c + gk[1] * s;
    x[2] = gv[0];
    x[3] = gq[1] * c - gq[0] * s;
    x[4] = gk[1] * c - gk[0] * s;
    x[5] = gv[1];
  }
  gcos[id] += gc;
  gsin[id] += gs;
}

// ============================================================================ positional encoding
__global__ __launch_bounds__(256) void pe_train_kernel(TPE p) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int f = gid & 31, pt = gid >> 5;
  if (pt >= p.B * p.n) return;
  const int b = pt / p.n;
  const float w = p.size[b * 2], hh = p.size[b * 2 + 1];
  const float scale = __fdiv_rn(fmaxf(w, hh), 2.f);  // normalize_keypoints (lightglue.py:29-32)
  float x[4];
  x[0] = __fdiv_rn(__fsub_rn(p.kpts[(long long)pt * 2], __fdiv_rn(w, 2.f)), scale);
  x[1] = __fdiv_rn(__fsub_rn(p.kpts[(long long)pt * 2 + 1], __fdiv_rn(hh, 2.f)), scale);
  x[2] = p.m_in == 4 ? p.scales[pt] : 0.f;
  x[3] = p.m_in == 4 ? p.oris[pt] : 0.f;
  const float* wr = p.Wr + f * p.m_in;
  float pr = __fmul_rn(x[0], wr[0]);
  for (int k = 1; k < p.m_in; ++k) pr = __fmaf_rn(x[k], wr[k], pr);
  pr = __fadd_rn(pr, __fadd_rn(__fmul_rn((float)p.n, p.Wc[f]), p.bc[f]));  // + Lin(relu(n)) (:70-74)
  p.cosb[(long long)pt * 32 + f] = cosf(pr);
  p.sinb[(long long)pt * 32 + f] = sinf(pr);
  if (f < 4) p.x[(long long)pt * 4 + f] = x[f];
}

constexpr int PE_ROWS = 256;  // rows per partial block
// block: 256 threads = 8 row groups x 32 frequencies; partial [blk][32][6] = (gWr[0..3], gWc, gbc)
__global__ __launch_bounds__(256) void pe_bwd_part_kernel(const float* x, const float* cosb, const float* sinb,
                                                          const float* gcos, const float* gsin, int R, int R0, float n0,
                                                          float n1, float* part) {
  __shared__ float red[8][32][6];
  const int f = threadIdx.x & 31, g = threadIdx.x >> 5;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int r0 = blockIdx.x * PE_ROWS;
  for (int r = r0 + g; r < min(R, r0 + PE_ROWS); r += 8) {
    const long long i = (long long)r * 32 + f;
    const float gp = cosb[i] * gsin[i] - sinb[i] * gcos[i];  // d/dproj of (cos proj, sin proj)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += gp * x[(long long)r * 4 + k];
    acc[4] += gp * (r < R0 ? n0 : n1);
    acc[5] += gp;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) red[g][f][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < 32 * 6) {
    const int ff = threadIdx.x / 6, k = threadIdx.x - ff * 6;
    float s = 0.f;
#pragma unroll
    for (int gg = 0; gg < 8; ++gg) s += red[gg][ff][k];
    part[((long long)blockIdx.x * 32 + ff) * 6 + k] = s;
  }
}

__global__ void pe_bwd_final_kernel(const float* part, int nblk, int m_in, float* gWr, float* gWc, float* gbc) {
  const int id = threadIdx.x;  // 32 x 6
  if (id >= 32 * 6) return;
  const int f = id / 6, k = id - f * 6;
  float s = 0.f;
  for (int i = 0; i < nblk; ++i) s += part[((long long)i * 32 + f) * 6 + k];
  // each output is optional: a frozen parameter (null gradient) is skipped, the others written
  if (k < m_in) {
    if (gWr) gWr[f * m_in + k] = s;
  } else if (k == 4) {
    if (gWc) gWc[f] = s;
  } else if (k == 5) {
    if (gbc) gbc[f] = s;
  }
}

// ============================================================================ LayerNorm + GELU
__device__ __forceinline__ float gelu_exact(float y) { return 0.5f * y * (1.f + erff(y * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad(float y) {
  return 0.5f * (1.f + erff(y * 0.70710678118654752f)) + y * 0.3989422804014327f * expf(-0.5f * y * y);
}

// one wave per row; lane holds columns [4l, 4l+4) and [256+4l, 256+4l+4)
__global__ __launch_bounds__(256) void lngelu_fwd_kernel(const float* hin, const float* gamma, const float* beta,
                                                         int R, float* out, float* stats) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= R) return;
  const float* x = hin + (long long)row * 512;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + 4 * l), v1 = *reinterpret_cast<const f32x4*>(x + 256 + 4 * l);
  const float mean = wave_sum((v0[0] + v0[1]) + (v0[2] + v0[3]) + (v1[0] + v1[1]) + (v1[2] + v1[3])) * (1.f / 512.f);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) q += (v0[i] - mean) * (v0[i] - mean) + (v1[i] - mean) * (v1[i] - mean);
  const float rstd = 1.f / sqrtf(wave_sum(q) * (1.f / 512.f) + 1e-5f);
  const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + 4 * l), g1 = *reinterpret_cast<const f32x4*>(gamma + 256 + 4 * l);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + 4 * l), b1 = *reinterpret_cast<const f32x4*>(beta + 256 + 4 * l);
  f32x4 o0, o1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o0[i] = gelu_exact((v0[i] - mean) * rstd * g0[i] + b0[i]);
    o1[i] = gelu_exact((v1[i] - mean) * rstd * g1[i] + b1[i]);
  }
  float* y = out + (long long)row * 512;
  *reinterpret_cast<f32x4*>(y + 4 * l) = o0;
  *reinterpret_cast<f32x4*>(y + 256 + 4 * l) = o1;
  if (l == 0) *reinterpret_cast<f32x2*>(stats + 2ll * row) = f32x2{mean, rstd};
}

constexpr int LN_ROWS = 64;  // rows per workgroup (16 per wave) in the backward
__global__ __launch_bounds__(256) void lngelu_bwd_kernel(const float* gout, const float* hin, const float* stats,
                                                         const float* gamma, const float* beta, int R, float* gh,
                                                         float* part) {
  __shared__ float red[4][2][512];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + 4 * l), g1 = *reinterpret_cast<const f32x4*>(gamma + 256 + 4 * l);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + 4 * l), b1 = *reinterpret_cast<const f32x4*>(beta + 256 + 4 * l);
  f32x4 dg0 = {0.f, 0.f, 0.f, 0.f}, dg1 = dg0, db0 = dg0, db1 = dg0;
  const int r0 = blockIdx.x * LN_ROWS + w * (LN_ROWS / 4);
  for (int row = r0; row < min(R, r0 + LN_ROWS / 4); ++row) {
    const float* x = hin + (long long)row * 512;
    const float* go = gout + (long long)row * 512;
    const f32x2 st = *reinterpret_cast<const f32x2*>(stats + 2ll * row);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + 4 * l), v1 = *reinterpret_cast<const f32x4*>(x + 256 + 4 * l);
    const f32x4 o0 = *reinterpret_cast<const f32x4*>(go + 4 * l), o1 = *reinterpret_cast<const f32x4*>(go + 256 + 4 * l);
    f32x4 xh0, xh1, gx0, gx1;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xh0[i] = (v0[i] - st[0]) * st[1];
      xh1[i] = (v1[i] - st[0]) * st[1];
      const float gy0 = o0[i] * gelu_grad(xh0[i] * g0[i] + b0[i]);
      const float gy1 = o1[i] * gelu_grad(xh1[i] * g1[i] + b1[i]);
      dg0[i] += gy0 * xh0[i];
      dg1[i] += gy1 * xh1[i];
      db0[i] += gy0;
      db1[i] += gy1;
      gx0[i] = gy0 * g0[i];
      gx1[i] = gy1 * g1[i];
      s1 += gx0[i] + gx1[i];
      s2 += gx0[i] * xh0[i] + gx1[i] * xh1[i];
    }
    s1 = wave_sum(s1) * (1.f / 512.f);
    s2 = wave_sum(s2) * (1.f / 512.f);
    f32x4 r0v, r1v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r0v[i] = st[1] * (gx0[i] - s1 - xh0[i] * s2);
      r1v[i] = st[1] * (gx1[i] - s1 - xh1[i] * s2);
    }
    float* y = gh + (long long)row * 512;
    *reinterpret_cast<f32x4*>(y + 4 * l) = r0v;
    *reinterpret_cast<f32x4*>(y + 256 + 4 * l) = r1v;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[w][0][4 * l + i] = dg0[i];
    red[w][0][256 + 4 * l + i] = dg1[i];
    red[w][1][4 * l + i] = db0[i];
    red[w][1][256 + 4 * l + i] = db1[i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const int k = i >> 9, cidx = i & 511;
    part[((long long)blockIdx.x * 2 + k) * 512 + cidx] = (red[0][k][cidx] + red[1][k][cidx]) + (red[2][k][cidx] + red[3][k][cidx]);
  }
}

// ============================================================================ column sums
// out[c] = sum_r s[r] G[r][c]: workgroups of 4 row lanes x 64 columns (a wave reads 256 contiguous
// bytes of one row per load), ~2048 workgroups over (column blocks, row chunks), fixed-order
// partials, then the same kernel again over the partials until one row is left.
constexpr int CS_TARGET_WG = 2048;
__global__ __launch_bounds__(256) void colsum_part_kernel(const float* G, long long ld, int rows, int cols,
                                                          const float* s, int rpb, float* part, long long sG = 0,
                                                          long long sP = 0) {
  __shared__ float red[4][64];
  G += blockIdx.z * sG;
  part += blockIdx.z * sP;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const int r0 = blockIdx.y * rpb, r1 = min(rows, r0 + rpb);
  float a0 = 0.f, a1 = 0.f;
  if (c < cols) {
    int r = r0 + g;
    for (; r + 4 < r1; r += 8) {
      const float v0 = G[(long long)r * ld + c], v1 = G[(long long)(r + 4) * ld + c];
      a0 = s ? fmaf(s[r], v0, a0) : a0 + v0;
      a1 = s ? fmaf(s[r + 4], v1, a1) : a1 + v1;
    }
    if (r < r1) {
      const float v0 = G[(long long)r * ld + c];
      a0 = s ? fmaf(s[r], v0, a0) : a0 + v0;
    }
  }
  red[g][threadIdx.x & 63] = a0 + a1;
  __syncthreads();
  if (g == 0 && c < cols) {
    const int t = threadIdx.x;
    part[(long long)blockIdx.y * cols + c] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  }
}

// column logsumexp of sim [B][M][N] in row chunks: (max, sum) partials [B][chunks][N], merged in
// chunk order
constexpr int LSE_ROWS = 64;
__global__ __launch_bounds__(256) void sim_lse_col_part_kernel(const float* sim, int M, int N, float2* part) {
  __shared__ float2 red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6, b = blockIdx.z;
  const int r0 = blockIdx.y * LSE_ROWS, r1 = min(M, r0 + LSE_ROWS);
  float m = -INFINITY, acc = 0.f;
  if (c < N) {
    const float* s = sim + (long long)b * M * N + c;
    for (int r = r0 + g; r < r1; r += 4) {
      const float v = s[(long long)r * N];
      if (v > m) {
        acc = acc * expf(m - v) + 1.f;
        m = v;
      } else {
        acc += expf(v - m);
      }
    }
  }
  red[g][threadIdx.x & 63] = make_float2(m, acc);
  __syncthreads();
  if (g == 0 && c < N) {
    float mm = -INFINITY, ss = 0.f;
    for (int k = 0; k < 4; ++k) {
      const float2 o = red[k][threadIdx.x];
      const float mx = fmaxf(mm, o.x);
      if (mx > -INFINITY) {
        ss = ss * expf(mm - mx) + o.y * expf(o.x - mx);
        mm = mx;
      }
    }
    part[((long long)b * gridDim.y + blockIdx.y) * N + c] = make_float2(mm, ss);
  }
}
// the same partials with four columns per thread (16-byte loads; N % 4 == 0): every column sees
// exactly the operations of sim_lse_col_part_kernel in the same order
__global__ __launch_bounds__(256) void sim_lse_col_part4_kernel(const float* sim, int M, int N, float2* part) {
  __shared__ f32x4 redm[4][64], reds[4][64];
  const int c = 4 * (blockIdx.x * 64 + (threadIdx.x & 63)), g = threadIdx.x >> 6, b = blockIdx.z;
  const int r0 = blockIdx.y * LSE_ROWS, r1 = min(M, r0 + LSE_ROWS);
  f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, acc = {0.f, 0.f, 0.f, 0.f};
  if (c < N) {
    const float* s = sim + (long long)b * M * N + c;
    for (int r = r0 + g; r < r1; r += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(s + (long long)r * N);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (v[e] > m[e]) {
          acc[e] = acc[e] * expf(m[e] - v[e]) + 1.f;
          m[e] = v[e];
        } else {
          acc[e] += expf(v[e] - m[e]);
        }
      }
    }
  }
  redm[g][threadIdx.x & 63] = m;
  reds[g][threadIdx.x & 63] = acc;
  __syncthreads();
  if (g == 0 && c < N) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float mm = -INFINITY, ss = 0.f;
      for (int k = 0; k < 4; ++k) {
        const float ox = redm[k][threadIdx.x][e], oy = reds[k][threadIdx.x][e];
        const float mx = fmaxf(mm, ox);
        if (mx > -INFINITY) {
          ss = ss * expf(mm - mx) + oy * expf(ox - mx);
          mm = mx;
        }
      }
      part[((long long)b * gridDim.y + blockIdx.y) * N + c + e] = make_float2(mm, ss);
    }
  }
}
// Row and column log-sum-exp in ONE read of the similarity (SLF_ROWS rows per workgroup; N % 4
// == 0, N <= 1024 QN): wave w owns the column quarter [w CW, (w + 1) CW), each lane QN 16-byte
// column groups of it.  Per row, each wave's (max, sum of exp) over its quarter goes to LDS and
// the four are merged after the row loop; per column, the lane's running (max, sum) over the
// workgroup's rows is the partial sim_lse_col_final_kernel merges.  The next row's values are
// loaded while the current one is reduced.
constexpr int SLF_ROWS = 32;
// RP rows per step, the next RP prefetched; only RP = 1 is instantiated (measured per launch at
// N = 2048: RP 1 172 us, 2 193 us, 4 199 us; the two-pass kernels 137 + 123 us, profiles/r05/lse_fused/)
template <int QN, int RP>
__global__ __launch_bounds__(256) void sim_lse_fused_kernel(const float* sim, int M, int N, float* lser, float2* part) {
  __shared__ float2 rst[SLF_ROWS][4];
  const int b = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int r0 = blockIdx.x * SLF_ROWS, r1 = min(M, r0 + SLF_ROWS);
  const int cw = ((N + 15) / 16) * 4;  // columns per wave, a multiple of 4
  const int cend = min(N, (w + 1) * cw);
  const float* sb = sim + (long long)b * M * N;
  const f32x4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int col[QN];
  bool ok[QN];
#pragma unroll
  for (int q = 0; q < QN; ++q) {
    col[q] = w * cw + 4 * (l + 64 * q);
    ok[q] = col[q] < cend;
  }
  f32x4 cm[QN], cs[QN], xn[RP][QN];
#pragma unroll
  for (int q = 0; q < QN; ++q) {
    cm[q] = ninf;
    cs[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto load_rows = [&](int r) {  // rows r .. r + RP - 1 (rows >= r1 read as -inf)
#pragma unroll
    for (int u = 0; u < RP; ++u)
#pragma unroll
      for (int q = 0; q < QN; ++q)
        xn[u][q] = (ok[q] && r + u < r1) ? *reinterpret_cast<const f32x4*>(sb + (long long)(r + u) * N + col[q]) : ninf;
  };
  load_rows(r0);
  for (int r = r0; r < r1; r += RP) {
    f32x4 x[RP][QN];
#pragma unroll
    for (int u = 0; u < RP; ++u)
#pragma unroll
      for (int q = 0; q < QN; ++q) x[u][q] = xn[u][q];
    if (r + RP < r1) load_rows(r + RP);
#pragma unroll
    for (int u = 0; u < RP; ++u) {
      if (r + u >= r1) break;
      // the row: max, then sum of exp over the wave's quarter
      float m = -INFINITY;
#pragma unroll
      for (int q = 0; q < QN; ++q) m = fmaxf(m, fmaxf(fmaxf(x[u][q][0], x[u][q][1]), fmaxf(x[u][q][2], x[u][q][3])));
      m = wave_max(m);
      float acc = 0.f;
      if (m > -INFINITY) {
#pragma unroll
        for (int q = 0; q < QN; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc += expf(x[u][q][e] - m);  // -inf pads add 0
      }
      acc = wave_sum(acc);
      if (l == 0) rst[r + u - r0][w] = make_float2(m, acc);
      // the columns: running (max, sum), one exp per value
#pragma unroll
      for (int q = 0; q < QN; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = x[u][q][e];
          if (v > cm[q][e]) {
            cs[q][e] = cs[q][e] * expf(cm[q][e] - v) + 1.f;
            cm[q][e] = v;
          } else if (v > -INFINITY) {
            cs[q][e] += expf(v - cm[q][e]);
          }
        }
    }
  }
#pragma unroll
  for (int q = 0; q < QN; ++q)
    if (ok[q]) {
      float2* pp = part + ((long long)b * gridDim.x + blockIdx.x) * N + col[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[e] = make_float2(cm[q][e], cs[q][e]);
    }
  __syncthreads();
  if ((int)threadIdx.x < r1 - r0) {
    float mm = -INFINITY, ss = 0.f;
    for (int k = 0; k < 4; ++k) {
      const float2 o = rst[threadIdx.x][k];
      const float mx = fmaxf(mm, o.x);
      if (mx > -INFINITY) {
        ss = ss * expf(mm - mx) + o.y * expf(o.x - mx);
        mm = mx;
      }
    }
    lser[(long long)b * M + r0 + threadIdx.x] = mm + logf(ss);
  }
}
__global__ __launch_bounds__(256) void sim_lse_col_final_kernel(const float2* part, int nch, int B, int N, float* lsec) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)B * N) return;
  const long long b = id / N, c = id - b * N;
  float mm = -INFINITY, ss = 0.f;
  const float2* p = part + b * nch * N + c;
  for (int k0 = 0; k0 < nch; k0 += 4) {
    float2 o4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) o4[u] = k0 + u < nch ? p[(long long)(k0 + u) * N] : make_float2(-INFINITY, 0.f);
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // the chunks in order; a padded one changes nothing
      const float2 o = o4[u];
      const float mx = fmaxf(mm, o.x);
      if (mx > -INFINITY) {
        ss = ss * expf(mm - mx) + o.y * expf(o.x - mx);
        mm = mx;
      }
    }
  }
  lsec[id] = mm + logf(ss);
}

// dst[b][c][r] = src[b][r][c]: 32 x 32 tiles through LDS (padded row), coalesced both ways
__global__ __launch_bounds__(256) void transpose_batched_kernel(const float* src, int rows, int cols, float* dst) {
  __shared__ float tile[32][33];
  const long long off = (long long)blockIdx.z * rows * cols;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + 8 * k][tx] = src[off + (long long)r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k, r = r0 + tx;
    if (r < rows && c < cols) dst[off + (long long)c * rows + r] = tile[tx][ty + 8 * k];
  }
}

// The gradients of up to two 256 -> 1 linears on the same input X [rows][256] (the assignment
// head's matchability and TokenConfidence's token linear, lightglue.py:96-122,306-315) in ONE read
// of X: part[blk] = (sum_r X[r][:] s0[r], sum_r X[r][:] s1[r], sum_r s0[r], sum_r s1[r]) over the
// workgroup's rows (4 row lanes of 64 x 4 columns, combined in lane order), then one ordered pass
// over the partials.  The sums run in fp64 (s0 / s1 are gradients whose row sums cancel heavily,
// e.g. the matchability bias); s1 nullable.
constexpr int HVG_ROWS = 256, HVG_W = 2 * 256 + 2;
__global__ __launch_bounds__(256) void head_vec_grads_part_kernel(const float* X, int rows, const float* s0,
                                                                  const float* s1, double* part) {
  __shared__ double r0[4][256], r1[4][256];
  __shared__ double rb[4][2];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int i0 = blockIdx.x * HVG_ROWS, i1 = min(rows, i0 + HVG_ROWS);
  double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
  double b0 = 0.0, b1 = 0.0;
  for (int r = i0 + w; r < i1; r += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(X + (long long)r * 256 + 4 * l);
    const double u = s0[r], v = s1 ? s1[r] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a0[e] = fma((double)x[e], u, a0[e]);
      a1[e] = fma((double)x[e], v, a1[e]);
    }
    b0 += u;
    b1 += v;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r0[w][4 * l + e] = a0[e];
    r1[w][4 * l + e] = a1[e];
  }
  if (l == 0) {
    rb[w][0] = b0;
    rb[w][1] = b1;
  }
  __syncthreads();
  double* pp = part + (long long)blockIdx.x * HVG_W;
  const int t = threadIdx.x;
  pp[t] = ((r0[0][t] + r0[1][t]) + r0[2][t]) + r0[3][t];
  pp[256 + t] = ((r1[0][t] + r1[1][t]) + r1[2][t]) + r1[3][t];
  if (t < 2) pp[512 + t] = ((rb[0][t] + rb[1][t]) + rb[2][t]) + rb[3][t];
}
__global__ __launch_bounds__(256) void head_vec_grads_final_kernel(const double* part, int nb, float* gw0, float* gb0,
                                                                   float* gw1, float* gb1) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= HVG_W) return;
  float* dst = j < 256 ? (gw0 ? gw0 + j : nullptr)
               : j < 512 ? (gw1 ? gw1 + (j - 256) : nullptr)
               : j == 512 ? gb0 : gb1;
  if (!dst) return;
  double a = 0.0;
  int k = 0;
  for (; k + 8 <= nb; k += 8) {  // eight loads in flight, the adds in block order
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = part[(long long)(k + u) * HVG_W + j];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += t[u];
  }
  for (; k < nb; ++k) a += part[(long long)k * HVG_W + j];
  *dst = (float)a;
}

// ============================================================================ small row ops
__global__ __launch_bounds__(256) void gemv256_kernel(const float* x, int rows, const float* w, const float* b,
                                                      float* y) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= rows) return;
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + (long long)row * 256 + 4 * l);
  const f32x4 u = *reinterpret_cast<const f32x4*>(w + 4 * l);
  const float s = wave_sum((v[0] * u[0] + v[1] * u[1]) + (v[2] * u[2] + v[3] * u[3]));
  if (l == 0) y[row] = s + b[0];
}

__global__ __launch_bounds__(256) void rank1_add256_kernel(float* G, int rows, const float* s, const float* w) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)rows * 64) return;
  const long long row = id >> 6;
  const int c4 = (int)(id & 63) * 4;
  f32x4* p = reinterpret_cast<f32x4*>(G + row * 256 + c4);
  const f32x4 u = *reinterpret_cast<const f32x4*>(w + c4);
  const float sv = s[row];
  f32x4 v = *p;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = fmaf(sv, u[e], v[e]);
  *p = v;
}

__global__ __launch_bounds__(256) void add_rows256_kernel(const float* A, long long lda, const float* B, long long ldb,
                                                          float* C, long long ldc, int rows) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)rows * 64) return;
  const long long row = id >> 6;
  const int c4 = (int)(id & 63) * 4;
  const f32x4 a = *reinterpret_cast<const f32x4*>(A + row * lda + c4);
  const f32x4 b = *reinterpret_cast<const f32x4*>(B + row * ldb + c4);
  *reinterpret_cast<f32x4*>(C + row * ldc + c4) = a + b;
}

// ============================================================================ assignment head
// row logsumexp: one wave per (pair, row)
__global__ __launch_bounds__(256) void sim_lse_row_kernel(const float* sim, int rows, int N, float* lser) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = sim + (long long)row * N;
  float m = -INFINITY, acc = 0.f;
  if (N <= 2048) {  // the row read once into registers; the same operations in the same order
    float x[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) x[q] = s[min(l + 64 * q, N - 1)];  // unconditional: all in flight
#pragma unroll
    for (int q = 0; q < 32; ++q) {
      if (l + 64 * q >= N) x[q] = -INFINITY;
      m = fmaxf(m, x[q]);
    }
    m = wave_max(m);
#pragma unroll
    for (int q = 0; q < 32; ++q)
      if (l + 64 * q < N) acc += expf(x[q] - m);
  } else {
    for (int j = l; j < N; j += 64) m = fmaxf(m, s[j]);
    m = wave_max(m);
    for (int j = l; j < N; j += 64) acc += expf(s[j] - m);
  }
  acc = wave_sum(acc);
  if (l == 0) lser[row] = m + logf(acc);
}
__global__ __launch_bounds__(256) void la_row_sums_kernel(const float* T, const float* s_in, const float* s_dust, int B,
                                                          int M, int N, float* rs, float* gd0) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= B * M) return;
  const int b = row / M, i = row - b * M;
  const float* t = T + ((long long)b * (M + 1) + i) * (N + 1);
  float acc = 0.f;
  for (int j = l; j < N; j += 64) acc += t[j];
  acc = wave_sum(acc);
  if (l == 0) {
    rs[row] = acc * (s_in ? s_in[b] : 1.f);
    gd0[row] = t[N] * (s_dust ? s_dust[b] : 1.f);
  }
}
__global__ __launch_bounds__(256) void la_col_final_kernel(const float* part, int nb, const float* T, const float* s_in,
                                                           const float* s_dust, int B, int M, int N, float* cs,
                                                           float* gd1) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= N) return;
  const float* p = part + (long long)b * nb * N + j;
  float acc = 0.f;
  for (int k = 0; k < nb; ++k) acc += p[(long long)k * N];
  cs[(long long)b * N + j] = acc * (s_in ? s_in[b] : 1.f);
  gd1[(long long)b * N + j] = T[(long long)b * (M + 1) * (N + 1) + (long long)M * (N + 1) + j] * (s_dust ? s_dust[b] : 1.f);
}

// d(loss)/d(sim) of one entry: 2 g - softmax_row * rs - softmax_col * cs, with the rounding
// spelled out (explicit fused multiply-adds) so every kernel below gives the same bits
__device__ __forceinline__ float la_gsim(float g, float x, float lr, float r, float lc, float c) {
  const float e1 = expf(x - lr), e2 = expf(x - lc);
  return __fmaf_rn(-e2, c, __fmaf_rn(-e1, r, 2.f * g));
}

// one workgroup per similarity row (b, i): per-row values loaded once, the row swept by 256 lanes
__global__ __launch_bounds__(256) void la_grad_sim_kernel(float* sim, const float* T, const float* s_in,
                                                          const float* lser, const float* lsec, const float* rs,
                                                          const float* cs, const float* gext, int B, int M, int N) {
  const int row = blockIdx.x, b = row / M, i = row - b * M;
  const float sc = s_in ? s_in[b] : 1.f, lr = lser[row], r = rs[row];
  const float* t = T + ((long long)b * (M + 1) + i) * (N + 1);
  const float* lc = lsec + (long long)b * N;
  const float* c = cs + (long long)b * N;
  float* s = sim + (long long)row * N;
  const float* ge = gext ? gext + (long long)row * N : nullptr;
  for (int j = threadIdx.x; j < N; j += 256) {
    const float g = t[j] * sc, x = s[j];
    // la = s - lse_row + s - lse_col + ...  (lightglue.py:288-293)
    float v = la_gsim(g, x, lr, r, lc[j], c[j]);
    if (ge) v += ge[j];
    s[j] = v;
  }
}

// The NLL's weights (losses.py:62-73) straight from the ground truth, never formed as a dense
// [B][M+1][N+1] tensor: inner w = gta (uint8 0/1), dustbin column w[i][N] = (gt0[i] == -1),
// dustbin row w[M][j] = (gt1[j] == -1) (the reference writes it at [:, -1, :m], so M == N).
// Every sum below adds 0/1 values (exact integers in fp32), and every product is the same
// (float weight) * scale as with the dense weights, so the results equal la_grad_sums +
// la_grad_sim on nll_weights bit for bit.
// Column counts of gta per chunk of rows: 4 waves x 64 lanes x 4 columns (one 32-bit load each).
__global__ __launch_bounds__(256) void la_gt_col_part_kernel(const uint8_t* gta, int M, int N, int rpb, float* part) {
  __shared__ float red[4][256];
  const int b = blockIdx.z, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int j0 = blockIdx.x * 256 + 4 * l;
  const int r0 = blockIdx.y * rpb, r1 = min(M, r0 + rpb);
  const uint8_t* g = gta + (long long)b * M * N;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  if ((N & 3) == 0 && j0 + 3 < N) {
#pragma unroll 8
    for (int r = r0 + w; r < r1; r += 4) {
      const unsigned v = *(const unsigned*)(g + (long long)r * N + j0);
      c0 += v & 0xff;
      c1 += (v >> 8) & 0xff;
      c2 += (v >> 16) & 0xff;
      c3 += v >> 24;
    }
  } else {
    for (int r = r0 + w; r < r1; r += 4) {
      const uint8_t* p = g + (long long)r * N;
      if (j0 < N) c0 += p[j0];
      if (j0 + 1 < N) c1 += p[j0 + 1];
      if (j0 + 2 < N) c2 += p[j0 + 2];
      if (j0 + 3 < N) c3 += p[j0 + 3];
    }
  }
  red[w][4 * l] = (float)c0;
  red[w][4 * l + 1] = (float)c1;
  red[w][4 * l + 2] = (float)c2;
  red[w][4 * l + 3] = (float)c3;
  __syncthreads();
  const int t = threadIdx.x, j = blockIdx.x * 256 + t;
  if (j < N) part[((long long)b * gridDim.y + blockIdx.y) * N + j] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}
__global__ __launch_bounds__(256) void la_gt_col_final_kernel(const float* part, int nb, const int64_t* gt1,
                                                              const float* s_in, const float* s_dust, int B, int N,
                                                              float* cs, float* gd1) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= N) return;
  const float* p = part + (long long)b * nb * N + j;
  float acc = 0.f;
  for (int k = 0; k < nb; ++k) acc += p[(long long)k * N];
  const long long o = (long long)b * N + j;
  cs[o] = acc * s_in[b];
  gd1[o] = (gt1[o] == -1 ? 1.f : 0.f) * s_dust[b];
}
// la_grad_sim_kernel with g = gta * s_in; the row's count (rs) and dustbin entry (gd0) are
// formed here from the row itself (la_row_sums_kernel's outputs).  GT_IT > 0 (N % 4 == 0,
// N <= 1024 GT_IT): each lane holds 4 columns per step in registers -- its gta word, similarity,
// column LSEs and column sums are all loaded before the count's reduction, so the row costs one
// memory round trip; GT_IT == 0: any N, one column per lane and step.
template <int GT_IT>
__global__ __launch_bounds__(256) void la_grad_sim_gt_kernel(float* sim, const uint8_t* gta, const int64_t* gt0,
                                                             const float* s_in, const float* s_dust, const float* lser,
                                                             const float* lsec, const float* cs, int B, int M, int N,
                                                             float* rs, float* gd0) {
  __shared__ float red[4];
  const int row = blockIdx.x, b = row / M, t = threadIdx.x;
  const uint8_t* g = gta + (long long)row * N;
  const float* lc = lsec + (long long)b * N;
  const float* c = cs + (long long)b * N;
  float* s = sim + (long long)row * N;
  float cnt = 0.f;
  unsigned gw[GT_IT > 0 ? GT_IT : 1];
  f32x4 sv[GT_IT > 0 ? GT_IT : 1], lv[GT_IT > 0 ? GT_IT : 1], cv[GT_IT > 0 ? GT_IT : 1];
  if constexpr (GT_IT > 0) {
#pragma unroll
    for (int it = 0; it < GT_IT; ++it) {
      const int j = 4 * (t + 256 * it);
      if (j < N) {
        gw[it] = *reinterpret_cast<const unsigned*>(g + j);
        sv[it] = *reinterpret_cast<const f32x4*>(s + j);
        lv[it] = *reinterpret_cast<const f32x4*>(lc + j);
        cv[it] = *reinterpret_cast<const f32x4*>(c + j);
        cnt += (float)((gw[it] & 0xff) + ((gw[it] >> 8) & 0xff) + ((gw[it] >> 16) & 0xff) + (gw[it] >> 24));
      }
    }
  } else {
    for (int j = t; j < N; j += 256) cnt += (float)g[j];
  }
  cnt = wave_sum(cnt);
  if ((t & 63) == 0) red[t >> 6] = cnt;
  __syncthreads();
  const float sc = s_in[b], lr = lser[row], r = ((red[0] + red[1]) + (red[2] + red[3])) * sc;
  if (t == 0) {
    rs[row] = r;
    gd0[row] = (gt0[row] == -1 ? 1.f : 0.f) * s_dust[b];
  }
  if constexpr (GT_IT > 0) {
#pragma unroll
    for (int it = 0; it < GT_IT; ++it) {
      const int j = 4 * (t + 256 * it);
      if (j < N) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gwv = (float)((gw[it] >> (8 * e)) & 0xff) * sc, x = sv[it][e];
          o[e] = la_gsim(gwv, x, lr, r, lv[it][e], cv[it][e]);
        }
        *reinterpret_cast<f32x4*>(s + j) = o;
      }
    }
  } else {
    for (int j = t; j < N; j += 256) {
      const float gwv = (float)g[j] * sc, x = s[j];
      s[j] = la_gsim(gwv, x, lr, r, lc[j], c[j]);
    }
  }
}

// sigmoid_log_double_softmax (lightglue.py:284-296) from sim [B][M][N], its row / column
// logsumexp and the matchability logits z0 [B*M] / z1 [B*N]: la [B][M+1][N+1]
__global__ __launch_bounds__(256) void la_forward_kernel(const float* sim, const float* lser, const float* lsec,
                                                         const float* z0, const float* z1, int B, int M, int N,
                                                         float* la) {
  const int row = blockIdx.x, b = row / (M + 1), i = row - b * (M + 1);  // one workgroup per la row
  float* out = la + (long long)row * (N + 1);
  const float* zb = z1 + (long long)b * N;
  if (i < M) {
    const long long ri = (long long)b * M + i;
    const float* s = sim + ri * N;
    const float* lc = lsec + (long long)b * N;
    const float lr = lser[ri], l0 = log_sigmoid(z0[ri]);
    for (int j = threadIdx.x; j < N; j += 256) {
      const float x = s[j];
      const float cert = l0 + log_sigmoid(zb[j]);
      out[j] = ((x - lr) + (x - lc[j])) + cert;
    }
    if (threadIdx.x == 0) out[N] = log_sigmoid(-z0[ri]);
  } else {
    for (int j = threadIdx.x; j < N; j += 256) out[j] = log_sigmoid(-zb[j]);
    if (threadIdx.x == 0) out[N] = 0.f;
  }
}

// the same with LA_R rows of one pair per workgroup (N <= LA_NMAX): the column terms lsec and
// logsigmoid(z1) staged once in LDS instead of a logsigmoid per element; identical arithmetic
constexpr int LA_R = 8, LA_NMAX = 4096;
__global__ __launch_bounds__(256) void la_forward_rows_kernel(const float* sim, const float* lser, const float* lsec,
                                                              const float* z0, const float* z1, int B, int M, int N,
                                                              float* la) {
  __shared__ float lc_s[LA_NMAX], ls_s[LA_NMAX];
  const int b = blockIdx.y, i0 = blockIdx.x * LA_R, i1 = min(M + 1, i0 + LA_R);
  const float* zb = z1 + (long long)b * N;
  const float* lcb = lsec + (long long)b * N;
  for (int j = threadIdx.x; j < N; j += 256) {
    lc_s[j] = lcb[j];
    ls_s[j] = log_sigmoid(zb[j]);
  }
  __syncthreads();
  for (int i = i0; i < i1; ++i) {
    float* out = la + ((long long)b * (M + 1) + i) * (N + 1);
    if (i < M) {
      const long long ri = (long long)b * M + i;
      const float* s = sim + ri * N;
      const float lr = lser[ri], l0 = log_sigmoid(z0[ri]);
      if (N <= 2048) {  // the thread's 8 values loaded together (clamped column), then written
        float xv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) xv[k] = s[min((int)threadIdx.x + 256 * k, N - 1)];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int j = threadIdx.x + 256 * k;
          if (j < N) out[j] = ((xv[k] - lr) + (xv[k] - lc_s[j])) + (l0 + ls_s[j]);
        }
      } else {
        for (int j = threadIdx.x; j < N; j += 256) {
          const float x = s[j];
          const float cert = l0 + ls_s[j];
          out[j] = ((x - lr) + (x - lc_s[j])) + cert;
        }
      }
      if (threadIdx.x == 0) out[N] = log_sigmoid(-z0[ri]);
    } else {
      for (int j = threadIdx.x; j < N; j += 256) out[j] = log_sigmoid(-zb[j]);
      if (threadIdx.x == 0) out[N] = 0.f;
    }
  }
}

// A loss head without its log assignment stored (LightGlue.loss, lightglue.py:614-663, needs only
// the NLL of each head's log assignment and, for TokenConfidence.loss, its row / column argmaxes):
// LN_R rows per workgroup, each value formed exactly as la_forward_rows_kernel forms it, then
//   * the inner positives of the NLL (losses.py:41-44): fp64 sum and count per workgroup,
//   * the row argmax over the N + 1 columns (first maximum) of rows < M,
//   * per column, the maximum over the workgroup's rows (first maximum; row M = the dustbin row
//     joins it), merged over the workgroups by la_nll_cols_kernel.
constexpr int LN_R = 32;
int ln_blocks(int M) { return (M + 1 + LN_R - 1) / LN_R; }

__device__ __forceinline__ void argmax_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// KC: columns per thread / 256 (N <= 256 KC; the column tables in LDS sized to it, so more
// workgroups fit a CU).  PF: the next row's similarity and ground truth are loaded while the
// current row is reduced (one row's memory latency in flight behind another's arithmetic); only
// PF = true is instantiated.
template <int KC, bool PF>
__global__ __launch_bounds__(256) void la_nll_rows_kernel(const float* sim, const float* lser, const float* lsec,
                                                          const float* z0, const float* z1, int B, int M, int N,
                                                          const uint8_t* gta, double* part, int64_t* am0, float* cval,
                                                          int* cidx) {
  __shared__ float lc_s[PF ? 256 * KC : LA_NMAX], ls_s[PF ? 256 * KC : LA_NMAX];
  __shared__ float rv[LN_R][4];  // per row, each wave's (max, first index): merged after the row loop
  __shared__ int ri_[LN_R][4];
  __shared__ double rd[2][4];
  const int b = blockIdx.y, blk = blockIdx.x, i0 = blk * LN_R, i1 = min(M + 1, i0 + LN_R);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const float* zb = z1 + (long long)b * N;
  const float* lcb = lsec + (long long)b * N;
  for (int j = t; j < N; j += 256) {
    lc_s[j] = lcb[j];
    ls_s[j] = log_sigmoid(zb[j]);
  }
  __syncthreads();
  float cm[KC];
  int ci[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    cm[k] = -INFINITY;
    ci[k] = 0x7fffffff;
  }
  double pos = 0.0, npos = 0.0;
  // rows i0 .. min(i1, M) - 1 of the similarity; xn / gn = the next row's values (PF)
  const int ie = min(i1, M);
  float xn[KC];
  uint8_t gn[KC];
  auto load_row = [&](int i) {
    const long long r = (long long)b * M + i;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int j = t + 256 * k;
      xn[k] = j < N ? sim[r * N + j] : 0.f;
      gn[k] = j < N ? gta[r * N + j] : 0;
    }
  };
  if (PF && i0 < ie) load_row(i0);
  for (int i = i0; i < i1; ++i) {
    float v[KC];
    if (i < M) {
      const long long r = (long long)b * M + i;
      float xc[KC];
      uint8_t gc[KC];
      if (!PF) load_row(i);
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        xc[k] = xn[k];
        gc[k] = gn[k];
      }
      if (PF && i + 1 < ie) load_row(i + 1);
      const float lr = lser[r], l0 = log_sigmoid(z0[r]);
      float bv = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const int j = t + 256 * k;
        if (j < N) {
          const float x = xc[k];
          v[k] = ((x - lr) + (x - lc_s[j])) + (l0 + ls_s[j]);
          if (gc[k]) {
            pos += v[k];
            npos += 1.0;
          }
          if (v[k] > bv) {  // j increases with k: the first maximum of the thread
            bv = v[k];
            bi = j;
          }
        } else {
          v[k] = -INFINITY;
        }
      }
      if (t == 0) argmax_merge(bv, bi, log_sigmoid(-z0[r]), N);  // the dustbin column
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        argmax_merge(bv, bi, ov, oi);
      }
      if (lane == 0) {
        rv[i - i0][w] = bv;
        ri_[i - i0][w] = bi;
      }
    } else {  // the dustbin row: logsigmoid(-z1)
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const int j = t + 256 * k;
        v[k] = j < N ? log_sigmoid(-zb[j]) : -INFINITY;
      }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (v[k] > cm[k]) {  // rows increase: the first maximum of the workgroup
        cm[k] = v[k];
        ci[k] = i;
      }
  }
  const int nblk = gridDim.x;
  __syncthreads();
  if (t < min(i1, M) - i0) {  // the rows' argmaxes over the four waves
    float bv = rv[t][0];
    int bi = ri_[t][0];
    for (int q = 1; q < 4; ++q) argmax_merge(bv, bi, rv[t][q], ri_[t][q]);
    am0[(long long)b * M + i0 + t] = bi;
  }
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int j = t + 256 * k;
    if (j < N) {
      cval[((long long)b * nblk + blk) * N + j] = cm[k];
      cidx[((long long)b * nblk + blk) * N + j] = ci[k];
    }
  }
  // the positives' fp64 sums: waves, then the four waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pos += __shfl_xor(pos, o);
    npos += __shfl_xor(npos, o);
  }
  if (lane == 0) {
    rd[0][w] = pos;
    rd[1][w] = npos;
  }
  __syncthreads();
  if (t == 0) {
    part[((long long)b * nblk + blk) * 2] = ((rd[0][0] + rd[0][1]) + rd[0][2]) + rd[0][3];
    part[((long long)b * nblk + blk) * 2 + 1] = ((rd[1][0] + rd[1][1]) + rd[1][2]) + rd[1][3];
  }
}

// the column argmaxes from the per-workgroup maxima (workgroups in row order: the first maximum)
__global__ __launch_bounds__(256) void la_nll_cols_kernel(const float* cval, const int* cidx, int B, int N, int nblk,
                                                          int64_t* am1) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * N) return;
  const int b = (int)(e / N), j = (int)(e - (long long)b * N);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  const long long o0 = (long long)b * nblk * N + j;
  int q = 0;
  for (; q + 8 <= nblk; q += 8) {  // eight workgroups' maxima loaded ahead, merged in row order
    float v8[8];
    int i8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v8[u] = cval[o0 + (long long)(q + u) * N];
      i8[u] = cidx[o0 + (long long)(q + u) * N];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) argmax_merge(bv, bi, v8[u], i8[u]);
  }
  for (; q < nblk; ++q) argmax_merge(bv, bi, cval[o0 + (long long)q * N], cidx[o0 + (long long)q * N]);
  am1[e] = bi;
}

// the NLL terms of each pair from the positives' partials and the dustbin entries, which are
// logsigmoid(-z0) / logsigmoid(-z1) (la_forward's values); the arithmetic of sg_nll_kernel
__global__ __launch_bounds__(256) void la_nll_final_kernel(const float* z0, const float* z1, int M, int N, const double* part,
                                                           int nblk, const int64_t* gt0, const int64_t* gt1, int mode,
                                                           float bal, int B, float* out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  double neg0 = 0.0, n0 = 0.0, neg1 = 0.0, n1 = 0.0;
  for (int i = tid; i < M; i += blockDim.x)
    if (gt0[(size_t)b * M + i] == -1) {
      neg0 += log_sigmoid(-z0[(size_t)b * M + i]);
      n0 += 1.0;
    }
  for (int j = tid; j < N; j += blockDim.x)
    if (gt1[(size_t)b * N + j] == -1) {
      neg1 += log_sigmoid(-z1[(size_t)b * N + j]);
      n1 += 1.0;
    }
  __shared__ double red[4][256];
  red[0][tid] = neg0;
  red[1][tid] = n0;
  red[2][tid] = neg1;
  red[3][tid] = n1;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if (tid < s2)
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s2];
    __syncthreads();
  }
  if (tid == 0) {
    double P = 0.0, NPd = 0.0;
    for (int c = 0; c < nblk; ++c) {
      P += part[((size_t)b * nblk + c) * 2];
      NPd += part[((size_t)b * nblk + c) * 2 + 1];
    }
    const float NP = (float)NPd, G0 = (float)red[0][0], C0 = (float)red[1][0];
    const float G1 = (float)red[2][0], C1 = (float)red[3][0];
    const float num_pos = fmaxf(NP, 1.f), nll_pos = -(float)P / num_pos;
    float nll_neg, num_neg;
    if (mode == 0) {
      num_neg = fmaxf(C0 + C1, 1.f);
      nll_neg = (-G0 + -G1) / num_neg;
    } else {
      const float a0 = fmaxf(C0, 1.f), a1 = fmaxf(C1, 1.f);
      nll_neg = (-G0 + -G1) / (a0 + a1);
      num_neg = (a0 + a1) / 2.f;
    }
    out[0 * B + b] = bal * nll_pos + (1.f - bal) * nll_neg;
    out[1 * B + b] = nll_pos;
    out[2 * B + b] = nll_neg;
    out[3 * B + b] = num_pos;
    out[4 * B + b] = num_neg;
  }
}

// d/dz of logsigmoid(z) (inner entries, summed: rs) and logsigmoid(-z) (the dustbin entry gd)
__global__ __launch_bounds__(256) void la_grad_z_kernel(const float* z, const float* rs, const float* gd, int rows,
                                                        float* gz) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const float sp = 1.f / (1.f + expf(-z[i]));  // sigmoid(z)
  gz[i] = (1.f - sp) * rs[i] - sp * gd[i];
}

// GX[r] += G_layer[pair][layer][point] for the layer-descriptor gradients [B][L][M or N][256]
__global__ __launch_bounds__(256) void add_layer_rows_kernel(float* GX, const float* g0, const float* g1, int B, int M,
                                                             int N, int L, int layer) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long R0 = (long long)B * M;
  if (id >= (R0 + (long long)B * N) * 64) return;
  const long long row = id >> 6;
  const int c4 = (int)(id & 63) * 4;
  const float* src;
  if (row < R0) {
    if (!g0) return;
    const long long b = row / M, n = row - b * M;
    src = g0 + ((b * L + layer) * M + n) * 256;
  } else {
    if (!g1) return;
    const long long r2 = row - R0, b = r2 / N, n = r2 - b * N;
    src = g1 + ((b * L + layer) * N + n) * 256;
  }
  f32x4* d = reinterpret_cast<f32x4*>(GX + row * 256 + c4);
  *d = *d + *reinterpret_cast<const f32x4*>(src + c4);
}

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

// ============================================================================ launchers
size_t tgemm_ws_floats(int M, int N, int K, int batch) {
  int kc = 0;
  const int ks = tgemm_split(M, N, K, batch, kc);
  return ks > 1 ? (size_t)ks * M * (N + 1) * batch : 0;  // + the column-sum partials
}

// The products whose operands both run along k in memory -- a linear layer's forward
// (ta = 0, tb = 1), and its input gradient (ta = 0, tb = 0) once the weight is transposed into
// `ws` -- go to gemm.hip's bf16x6 kernel: both fp32 operands split into three bf16 pieces, six
// v_mfma_f32_32x32x16_bf16 per 32 x 32 x 16 block (the fp32-accurate product of common.h at
// 2.5 PF/s bf16 instead of the 157 TF/s f32 MFMA); error per product ~2^-24 like an f32 fma chain.
static bool tgemm_x6(const TGemm& g, bool ta, bool tb, float* ws, size_t ws_floats, hipStream_t st, hipError_t& err) {
  if (ta || g.K < 16 || g.K % 16 || (g.beta != 0.f && g.beta != 1.f)) return false;
  auto al = [](const void* ptr, long long ld, long long sb) {
    return ((uintptr_t)ptr % 16 == 0) && ld % 4 == 0 && sb % 4 == 0;
  };
  GemmArgs x{};
  x.A0 = g.A;
  x.lda0 = (int)g.lda;
  x.K0 = g.K;
  x.K = g.K;
  if (g.A1) {  // [A | A1] along k
    if (!tb || g.batch != 1 || g.K0 <= 0 || g.K0 % 16 || g.K0 >= g.K || !al(g.A1, g.lda1, 0)) return false;
    x.K0 = g.K0;
    x.A1 = g.A1;
    x.lda1 = (int)g.lda1;
  }
  x.bias = g.bias;
  x.res = g.R ? g.R : g.beta != 0.f ? g.C : nullptr;  // Y = res + (acc + bias) alpha
  x.ldr = (int)(g.R ? g.ldr : g.ldc);
  if (g.R && (g.beta != 1.f || g.batch != 1 || !al(g.R, g.ldr, 0))) return false;
  // gemm_x6 reads `res` without a per-batch stride: a batched beta C would add batch 0's C everywhere
  if (g.beta != 0.f && g.batch != 1 && !g.R) return false;
  x.Y = g.C;
  x.ldy = (int)g.ldc;
  x.out_scale = g.alpha;
  x.R = g.M;
  x.Nout = g.N;
  x.sA = g.sA;
  x.sY = g.sC;
  if (!al(g.A, g.lda, g.sA)) return false;
  if (tb) {
    if (!al(g.B, g.ldb, g.sB)) return false;
    x.W = g.B;
    x.ldw = (int)g.ldb;
    x.sW = g.sB;
  } else {
    // B [K][N] -> B^T [N][K] in ws (a weight: small)
    if (g.batch != 1 || g.ldb != g.N || !ws || ws_floats < (size_t)g.N * g.K + 4) return false;
    err = sg_transpose(g.B, g.K, g.N, ws, st);
    if (err != hipSuccess) return true;
    x.W = ws;
    x.ldw = g.K;
  }
  err = gemm_x6(x, EPI_STORE, g.batch, st);
  return true;
}

hipError_t tgemm(const TGemm& g_in, bool ta, bool tb, float* ws, size_t ws_floats, hipStream_t st) {
  TGemm g = g_in;
  if (!(ta && !tb)) g.colsumA = nullptr;  // only the bf16x6 weight-gradient kernels sum
  if (g.M <= 0 || g.N <= 0 || g.batch <= 0) return hipSuccess;
  if (g.colsumA && g.K <= 0) return hipMemsetAsync(g.colsumA, 0, sizeof(float) * g.M * g.batch, st);
  hipError_t xe = hipSuccess;
  if (tgemm_x6(g, ta, tb, ws, ws_floats, st, xe)) return xe;
  if (g.A1) return hipErrorInvalidValue;  // the two-source A exists on the bf16x6 route only
  if (g.B1 && (g.batch != 1 || g.N0 % X6_BN || !ta || tb)) return hipErrorInvalidValue;
  if (g.R) {  // the f32 kernels read the beta term from C: put the residual there first
    if (g.batch != 1) return hipErrorInvalidValue;
    const hipError_t e = hipMemcpy2DAsync(g.C, g.ldc * sizeof(float), g.R, g.ldr * sizeof(float), g.N * sizeof(float), g.M,
                                          hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
    g.R = nullptr;
  }
  TGemmK p{};
  p.g = g;
  int kc = 0;
  p.ksplit = tgemm_split(g.M, g.N, std::max(g.K, 1), g.batch, kc);
  p.kchunk = kc;
  const size_t need = (size_t)p.ksplit * g.M * g.N * g.batch + (g.colsumA ? (size_t)p.ksplit * g.M * g.batch : 0);
  if (p.ksplit > 1 && (!ws || need > ws_floats)) {
    p.ksplit = 1;
    p.kchunk = std::max(g.K, 1);
  }
  p.part = ws;
  p.cpart = ws ? ws + (size_t)p.ksplit * g.M * g.N * g.batch : nullptr;
  auto aligned = [](const float* ptr, long long ld, long long sb) {
    return ((uintptr_t)ptr % 16 == 0) && ld % 4 == 0 && sb % 4 == 0;
  };
  p.vecA = aligned(g.A, g.lda, g.sA);
  p.vecB = aligned(g.B, g.ldb, g.sB);
  const dim3 grid(cdiv(g.M, TG_BM), cdiv(g.N, TG_BN), g.batch * p.ksplit);
  if (ta && !tb) {  // weight gradients on bf16x6: the vectorised kernel, tgemm_x6t_kernel for unaligned operands
    const bool vec = g.M % 4 == 0 && g.N % 4 == 0 && g.lda % 4 == 0 && g.ldb % 4 == 0 &&
                     g.sA % 4 == 0 && g.sB % 4 == 0 && (uintptr_t)g.A % 16 == 0 && (uintptr_t)g.B % 16 == 0;
    if (g.B1 && !(vec && (uintptr_t)g.B1 % 16 == 0 && g.ldb1 % 4 == 0)) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL(tgemm_x6tv_kernel, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(tgemm_x6t_kernel, grid, dim3(256), 0, st, p);
    if (p.ksplit > 1) {
      const int nmain = (int)cdiv((long long)g.M * g.N * g.batch, 256);
      const int ncs = g.colsumA ? (int)cdiv((long long)g.M * g.batch, 4) : 0;
      hipLaunchKernelGGL(tgemm_reduce_kernel, dim3(nmain + ncs), dim3(256), 0, st, p, nmain);
    }
    return hipGetLastError();
  }
  if (!ta && !tb) hipLaunchKernelGGL((tgemm_kernel<false, false>), grid, dim3(256), 0, st, p);
  else if (!ta && tb) hipLaunchKernelGGL((tgemm_kernel<false, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((tgemm_kernel<true, true>), grid, dim3(256), 0, st, p);
  if (p.ksplit > 1)
    hipLaunchKernelGGL(tgemm_reduce_kernel, dim3(cdiv((long long)g.M * g.N * g.batch, 256)), dim3(256), 0, st, p,
                       (int)cdiv((long long)g.M * g.N * g.batch, 256));
  return hipGetLastError();
}

hipError_t tattn_forward(const TAttn& a, hipStream_t st) {
  if (a.B * a.H == 0 || a.Nq == 0) return hipSuccess;
  hipLaunchKernelGGL(tattn_fwd_x6_kernel<8>, dim3(cdiv(a.Nq, 256), a.B * a.H), dim3(512), 0, st, a);
  return hipGetLastError();
}

// Nq == 0 (no query tiles): dK / dV are written as zeros, or left as they are under accum_kv
hipError_t tattn_backward(const TAttn& a, hipStream_t st) {
  if (a.B * a.H == 0 || a.Nk == 0) return hipSuccess;
  hipLaunchKernelGGL(tattn_bwd_x6_kernel, dim3(cdiv(a.Nk, TB_KEYS), a.B * a.H), dim3(64 * TB_W), 0, st, a);
  return hipGetLastError();
}

hipError_t attn_delta(const float* O, const float* dO, int ldo, int B, int H, int Nq, float* delta, hipStream_t st) {
  if (B * Nq == 0) return hipSuccess;
  hipLaunchKernelGGL(attn_delta_kernel, dim3(cdiv((long long)B * Nq, 4)), dim3(256), 0, st, O, dO, ldo, B, H, Nq, delta);
  return hipGetLastError();
}

hipError_t rotary_split(const float* qkv, const float* cosb, const float* sinb, int R, int H, float* Q, float* K,
                        float* V, hipStream_t st) {
  if (R == 0) return hipSuccess;
  hipLaunchKernelGGL(rotary_split_kernel, dim3(cdiv((long long)R * H * 32, 256)), dim3(256), 0, st, qkv, cosb, sinb, R, H, Q,
                     K, V);
  return hipGetLastError();
}

hipError_t rotary_split_bwd(const float* gQ, const float* gK, const float* gV, const float* Q, const float* K,
                            const float* cosb, const float* sinb, int R, int H, float* gQKV, float* gcos, float* gsin,
                            hipStream_t st) {
  if (R == 0) return hipSuccess;
  hipLaunchKernelGGL(rotary_split_bwd_kernel, dim3(cdiv((long long)R * 32, 256)), dim3(256), 0, st, gQ, gK, gV, Q, K, cosb,
                     sinb, R, H, gQKV, gcos, gsin);
  return hipGetLastError();
}

hipError_t pe_train(const TPE& p, hipStream_t st) {
  if (p.B * p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(pe_train_kernel, dim3(cdiv((long long)p.B * p.n * 32, 256)), dim3(256), 0, st, p);
  return hipGetLastError();
}

size_t pe_bwd_part_floats(int R) { return (size_t)cdiv(std::max(R, 1), PE_ROWS) * 32 * 6; }

hipError_t pe_backward(const float* x, const float* cosb, const float* sinb, const float* gcos, const float* gsin,
                       int R, int R0, float n0, float n1, int m_in, float* part, float* gWr, float* gWc, float* gbc,
                       hipStream_t st) {
  const int nblk = (int)cdiv(std::max(R, 1), PE_ROWS);
  hipLaunchKernelGGL(pe_bwd_part_kernel, dim3(nblk), dim3(256), 0, st, x, cosb, sinb, gcos, gsin, R, R0, n0, n1, part);
  hipLaunchKernelGGL(pe_bwd_final_kernel, dim3(1), dim3(256), 0, st, part, nblk, m_in, gWr, gWc, gbc);
  return hipGetLastError();
}

hipError_t lngelu_fwd(const float* h, const float* gamma, const float* beta, int R, float* out, float* stats,
                      hipStream_t st) {
  if (R == 0) return hipSuccess;
  hipLaunchKernelGGL(lngelu_fwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, st, h, gamma, beta, R, out, stats);
  return hipGetLastError();
}

size_t lngelu_bwd_part_floats(int R) {
  const int nblk = (int)cdiv(std::max(R, 1), LN_ROWS);
  return (size_t)nblk * 1024 + colsum_part_floats(nblk, 512);
}

hipError_t lngelu_bwd(const float* gout, const float* h, const float* stats, const float* gamma, const float* beta,
                      int R, float* gh, float* part, float* dgamma, float* dbeta, hipStream_t st) {
  const int nblk = (int)cdiv(std::max(R, 1), LN_ROWS);
  hipLaunchKernelGGL(lngelu_bwd_kernel, dim3(nblk), dim3(256), 0, st, gout, h, stats, gamma, beta, R, gh, part);
  // dgamma = sum of the even partial rows, dbeta of the odd ones: [blk][2][512] read as [blk*2][512]
  hipError_t e = hipGetLastError();
  // dgamma / dbeta: column sums of the partial rows [blk][2][512] (read as two 512-wide windows of
  // [blk][1024]); the sums' own partials go after the LN partials
  float* cs_part = part + (size_t)nblk * 1024;
  if (e == hipSuccess && dgamma) e = colsum(part, 1024, nblk, 512, nullptr, cs_part, dgamma, st);
  if (e == hipSuccess && dbeta) e = colsum(part + 512, 1024, nblk, 512, nullptr, cs_part, dbeta, st);
  return e;
}

namespace {
int cs_chunks(int rows, int cols) {
  const int cb = (cols + 63) / 64;
  return std::max(1, std::min((rows + 15) / 16, CS_TARGET_WG / cb));
}
}  // namespace

size_t colsum_part_floats(int rows, int cols) {
  size_t total = 0;
  for (int nb = cs_chunks(std::max(rows, 1), cols); nb > 1; nb = cs_chunks(nb, cols)) total += (size_t)nb * std::max(cols, 1);
  return total + std::max(cols, 1);
}

hipError_t colsum(const float* G, long long ld, int rows, int cols, const float* s, float* part, float* out,
                  hipStream_t st) {
  if (cols == 0) return hipSuccess;
  if (rows == 0) return hipMemsetAsync(out, 0, sizeof(float) * cols, st);
  const int cb = (cols + 63) / 64;
  const float* src = G;
  long long sld = ld;
  const float* sc = s;
  int n = rows;
  float* p = part;
  while (true) {
    const int nb = cs_chunks(n, cols);
    const int rpb = (n + nb - 1) / nb;
    const int m = (n + rpb - 1) / rpb;
    float* dst = m == 1 ? out : p;
    hipLaunchKernelGGL(colsum_part_kernel, dim3(cb, m), dim3(256), 0, st, src, sld, n, cols, sc, rpb, dst);
    if (m == 1) break;
    src = p;
    sld = cols;
    sc = nullptr;
    n = m;
    p += (size_t)m * cols;
  }
  return hipGetLastError();
}

size_t head_vec_grads_part_floats(int rows) { return 2 * (size_t)cdiv(std::max(rows, 1), HVG_ROWS) * HVG_W + 4; }

hipError_t head_vec_grads(const float* X, int rows, const float* s0, const float* s1, float* part, float* gw0, float* gb0,
                          float* gw1, float* gb1, hipStream_t st) {
  if (rows <= 0) return hipErrorInvalidValue;
  const int nb = (int)cdiv(rows, HVG_ROWS);
  double* dp = reinterpret_cast<double*>(((uintptr_t)part + 7) & ~(uintptr_t)7);  // fp64 partials
  hipLaunchKernelGGL(head_vec_grads_part_kernel, dim3(nb), dim3(256), 0, st, X, rows, s0, s1, dp);
  hipLaunchKernelGGL(head_vec_grads_final_kernel, dim3(cdiv(HVG_W, 256)), dim3(256), 0, st, dp, nb, gw0, gb0, gw1, gb1);
  return hipGetLastError();
}

hipError_t gemv256(const float* x, int rows, const float* w, const float* b, float* y, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(gemv256_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, rows, w, b, y);
  return hipGetLastError();
}

hipError_t rank1_add256(float* G, int rows, const float* s, const float* w, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(rank1_add256_kernel, dim3(cdiv((long long)rows * 64, 256)), dim3(256), 0, st, G, rows, s, w);
  return hipGetLastError();
}

hipError_t add_rows256(const float* A, long long lda, const float* B, long long ldb, float* C, long long ldc, int rows,
                       hipStream_t st) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(add_rows256_kernel, dim3(cdiv((long long)rows * 64, 256)), dim3(256), 0, st, A, lda, B, ldb, C, ldc,
                     rows);
  return hipGetLastError();
}

hipError_t add_layer_rows(float* GX, const float* g0, const float* g1, int B, int M, int N, int L, int layer,
                          hipStream_t st) {
  const long long n = (long long)B * (M + N) * 64;
  if (n == 0 || (!g0 && !g1)) return hipSuccess;
  hipLaunchKernelGGL(add_layer_rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, GX, g0, g1, B, M, N, L, layer);
  return hipGetLastError();
}

size_t sim_lse_part_floats(int B, int M, int N) {
  return 2 * (size_t)B * cdiv(std::max(M, 1), std::min(LSE_ROWS, SLF_ROWS)) * N;
}

hipError_t sim_lse(const float* sim, int B, int M, int N, float* lser, float* lsec, float* part, hipStream_t st) {
  if (B * M == 0 || N == 0) return hipSuccess;
  if (N % 4 == 0 && N <= 4096 && (reinterpret_cast<uintptr_t>(sim) & 15) == 0) {
    const int nch = (int)cdiv(M, SLF_ROWS);
    float2* p2 = reinterpret_cast<float2*>(part);
#define LG_SLF(QN) hipLaunchKernelGGL((sim_lse_fused_kernel<QN, 1>), dim3(nch, B), dim3(256), 0, st, sim, M, N, lser, p2)
    if (N <= 1024) LG_SLF(1);
    else if (N <= 2048) LG_SLF(2);
    else LG_SLF(4);
#undef LG_SLF
    hipLaunchKernelGGL(sim_lse_col_final_kernel, dim3(cdiv((long long)B * N, 256)), dim3(256), 0, st, p2, nch, B, N, lsec);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(sim_lse_row_kernel, dim3(cdiv((long long)B * M, 4)), dim3(256), 0, st, sim, B * M, N, lser);
  const int nch = (int)cdiv(M, LSE_ROWS);
  float2* p2 = reinterpret_cast<float2*>(part);
  if (N % 4 == 0 && (reinterpret_cast<uintptr_t>(sim) & 15) == 0)
    hipLaunchKernelGGL(sim_lse_col_part4_kernel, dim3(cdiv(N, 256), nch, B), dim3(256), 0, st, sim, M, N, p2);
  else
    hipLaunchKernelGGL(sim_lse_col_part_kernel, dim3(cdiv(N, 64), nch, B), dim3(256), 0, st, sim, M, N, p2);
  hipLaunchKernelGGL(sim_lse_col_final_kernel, dim3(cdiv((long long)B * N, 256)), dim3(256), 0, st, p2, nch, B, N, lsec);
  return hipGetLastError();
}

size_t la_grad_sums_part_floats(int B, int M, int N) {
  const int cb = (int)cdiv(std::max(N, 1), 64);
  const int nb = std::max(1, std::min((int)cdiv(std::max(M, 1), 16), std::max(1, CS_TARGET_WG / (cb * std::max(B, 1)))));
  return (size_t)B * nb * std::max(N, 1);
}

hipError_t la_grad_sums(const float* T, const float* s_in, const float* s_dust, int B, int M, int N, float* rs,
                        float* cs, float* gd0, float* gd1, float* part, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (M > 0)
    hipLaunchKernelGGL(la_row_sums_kernel, dim3(cdiv((long long)B * M, 4)), dim3(256), 0, st, T, s_in, s_dust, B, M, N, rs,
                       gd0);
  if (N > 0) {
    // inner column sums per pair: batched two-pass column sums (partials [B][nb][N]), then one
    // scaling pass that also picks up the dustbin-row entries
    const int cb = (int)cdiv(N, 64);
    const int nb = std::max(1, std::min((int)cdiv(std::max(M, 1), 16), std::max(1, CS_TARGET_WG / (cb * B))));
    const int rpb = (int)cdiv(std::max(M, 1), nb);
    const int m = (int)cdiv(std::max(M, 1), rpb);
    hipLaunchKernelGGL(colsum_part_kernel, dim3(cb, m, B), dim3(256), 0, st, T, (long long)(N + 1), M, N,
                       (const float*)nullptr, rpb, part, (long long)(M + 1) * (N + 1), (long long)m * N);
    hipLaunchKernelGGL(la_col_final_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, st, part, m, T, s_in, s_dust, B, M, N, cs,
                       gd1);
  }
  return hipGetLastError();
}

hipError_t la_grad_sim(float* sim, const float* T, const float* s_in, const float* lser, const float* lsec,
                       const float* rs, const float* cs, const float* gsim_ext, int B, int M, int N, hipStream_t st) {
  const long long n = (long long)B * M * N;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(la_grad_sim_kernel, dim3(B * M), dim3(256), 0, st, sim, T, s_in, lser, lsec, rs, cs, gsim_ext, B, M,
                     N);
  return hipGetLastError();
}

namespace {
int la_gt_chunks(int B, int M, int N) {
  const int cb = (int)cdiv(std::max(N, 1), 256);
  return std::max(1, std::min((int)cdiv(std::max(M, 1), 64), std::max(1, CS_TARGET_WG / (cb * std::max(B, 1)))));
}
}  // namespace

size_t la_grad_gt_part_floats(int B, int M, int N) {
  return (size_t)std::max(B, 0) * la_gt_chunks(B, M, N) * std::max(N, 1);
}

hipError_t la_grad_gt(float* sim, const uint8_t* gta, const int64_t* gt0, const int64_t* gt1, const float* s_in,
                      const float* s_dust, const float* lser, const float* lsec, int B, int M, int N, float* rs, float* cs,
                      float* gd0, float* gd1, float* part, hipStream_t st) {
  if (B <= 0 || M <= 0 || N <= 0) return hipSuccess;
  const int nb0 = la_gt_chunks(B, M, N);
  const int rpb = (int)cdiv(M, nb0), nb = (int)cdiv(M, rpb);
  hipLaunchKernelGGL(la_gt_col_part_kernel, dim3(cdiv(N, 256), nb, B), dim3(256), 0, st, gta, M, N, rpb, part);
  hipLaunchKernelGGL(la_gt_col_final_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, st, part, nb, gt1, s_in, s_dust, B, N,
                     cs, gd1);
#define LG_GT_SIM(IT)                                                                                        \
  hipLaunchKernelGGL(la_grad_sim_gt_kernel<IT>, dim3(B * M), dim3(256), 0, st, sim, gta, gt0, s_in, s_dust, lser, lsec, cs, \
                     B, M, N, rs, gd0)
  // the 16-byte paths need 16-byte aligned rows: N % 4 == 0 and aligned bases
  const bool vec = N % 4 == 0 && ((uintptr_t)sim | (uintptr_t)gta | (uintptr_t)lsec | (uintptr_t)cs) % 16 == 0;
  if (vec && N <= 1024) LG_GT_SIM(1);
  else if (vec && N <= 2048) LG_GT_SIM(2);
  else if (vec && N <= 4096) LG_GT_SIM(4);
  else LG_GT_SIM(0);
#undef LG_GT_SIM
  return hipGetLastError();
}

hipError_t la_forward(const float* sim, const float* lser, const float* lsec, const float* z0, const float* z1, int B, int M,
                      int N, float* la, hipStream_t st) {
  const long long n = (long long)B * (M + 1) * (N + 1);
  if (n == 0) return hipSuccess;
  if (N <= LA_NMAX)
    hipLaunchKernelGGL(la_forward_rows_kernel, dim3(cdiv(M + 1, LA_R), B), dim3(256), 0, st, sim, lser, lsec, z0, z1, B, M,
                       N, la);
  else
    hipLaunchKernelGGL(la_forward_kernel, dim3(B * (M + 1)), dim3(256), 0, st, sim, lser, lsec, z0, z1, B, M, N, la);
  return hipGetLastError();
}

size_t la_nll_part_floats(int B, int M, int N) {
  // fp64 partials [B][nblk][2] (as 4 floats each) + column maxima and their rows [B][nblk][N] x 2
  const size_t nb = (size_t)std::max(B, 0) * ln_blocks(std::max(M, 0));
  return 4 * nb + 2 * nb * std::max(N, 0) + 16;
}

hipError_t la_nll(const float* sim, const float* lser, const float* lsec, const float* z0, const float* z1, int B, int M,
                  int N, const uint8_t* gta, const int64_t* gt0, const int64_t* gt1, int mode, float bal, float* out,
                  int64_t* am0, int64_t* am1, float* part, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (N > LA_NMAX || M <= 0 || N <= 0) return hipErrorInvalidValue;
  const int nblk = ln_blocks(M);
  double* dp = reinterpret_cast<double*>(part);
  float* cval = part + 4 * (size_t)B * nblk;
  int* cidx = reinterpret_cast<int*>(cval + (size_t)B * nblk * N);
#define LG_NLL_ROWS(KC)                                                                                                \
  hipLaunchKernelGGL((la_nll_rows_kernel<KC, true>), dim3(nblk, B), dim3(256), 0, st, sim, lser, lsec, z0, z1, B, M, N, gta, \
                     dp, am0, cval, cidx)
  if (N <= 1024) LG_NLL_ROWS(4);
  else if (N <= 2048) LG_NLL_ROWS(8);
  else LG_NLL_ROWS(16);
#undef LG_NLL_ROWS
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(la_nll_cols_kernel, dim3(cdiv((long long)B * N, 256)), dim3(256), 0, st, cval, cidx, B, N, nblk, am1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(la_nll_final_kernel, dim3(B), dim3(256), 0, st, z0, z1, M, N, dp, nblk, gt0, gt1, mode, bal, B, out);
  return hipGetLastError();
}

hipError_t transpose_batched(const float* src, int rows, int cols, int batch, float* dst, hipStream_t st) {
  if (rows <= 0 || cols <= 0 || batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(transpose_batched_kernel, dim3(cdiv(cols, 32), cdiv(rows, 32), batch), dim3(256), 0, st, src, rows, cols,
                     dst);
  return hipGetLastError();
}

hipError_t la_grad_z(const float* z, const float* rs, const float* gd, int rows, float* gz, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(la_grad_z_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, z, rs, gd, rows, gz);
  return hipGetLastError();
}

}  // namespace lg
