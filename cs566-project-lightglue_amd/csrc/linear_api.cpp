// C-ABI of the kernel-level linear entry (include/lightglue_mi355x.h: lg_linear, lg_plane_roundtrip):
// one launch of gemm_h3 / gemm_x6 on plain fp32 tensors, prepared inside the caller's workspace the
// way the forward prepares them (lightglue_api.cpp forward_pass / lg_load_weights).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

#include "common.h"

namespace {
using namespace lg;

constexpr int kSlots = 8;  // 0/1: max|A0|, max|A1|; 2/3: their images; 4: output; 5: values; 6: max|res|
enum { S_IN0 = 0, S_IN1 = 1, S_A0 = 2, S_A1 = 3, S_OUT = 4, S_OUTV = 5, S_RES = 6 };

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

struct Layout {
  int RP;
  size_t rtab, stats, a0, a1, w, h1, rtmp, ytmp, qtmp, cos1, sin0, bytes;
};
Layout carve(int R, int K0, int K, int Nout) {
  Layout L;
  L.RP = (R + 255) / 256 * 256;
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += align256(n);
    return o;
  };
  L.rtab = take((size_t)kSlots * kRangeStride * sizeof(unsigned));
  L.stats = take(16 * sizeof(float));
  L.a0 = take((size_t)2 * L.RP * K0 * 2);
  L.a1 = take((size_t)2 * L.RP * (K - K0) * 2);
  L.w = take((size_t)2 * Nout * K * 2);
  L.h1 = take((size_t)R * Nout * 4);    // LN routes: the fp32 pre-activations
  L.rtmp = take((size_t)R * Nout * 4);  // bf16x6: res | res2 as one array
  L.ytmp = take((size_t)R * Nout * 4);  //         Y | Y2 as one array
  L.qtmp = take((size_t)R * 256 * 4);   //         q when the caller wants planes only
  L.cos1 = take((size_t)R * 32 * 4);    //         identity rotary tables (no-rotary QKV)
  L.sin0 = take((size_t)R * 32 * 4);
  L.bytes = off;
  return L;
}

const char* shape_error(int64_t R, int64_t K0, int64_t K, int64_t Nout) {
  if (R < 0 || K <= 0 || Nout <= 0) return "negative or empty size";
  if (Nout % 256) return "Nout must be a multiple of 256";
  if (K % 32 || K0 % 32) return "K and K0 must be multiples of 32";
  if (K0 <= 0 || K0 > K) return "K0 must be in (0, K]";
  if (R > (1 << 20) || K > 4096 || Nout > 4096) return "shape too large for the kernel-level entry";
  return nullptr;
}

__global__ void fill_f32_kernel(float* p, float v, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// rows of a plane image that hold no live row (dead rows of the mask, padding rows [R, rows_pad)):
// finite fp16 garbage of magnitude 3e4 .. 6.3e4, both planes
__global__ void poison_rows_kernel(_Float16* planes, long long ps, int rows_pad, int K, int R, RowMask rm) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows_pad * K) return;
  const int r = (int)(i / K), k = (int)(i % K);
  if (r < R && row_live(rm, r)) return;
  const unsigned hsh = (unsigned)i * 2654435761u;
  const float v = (30000.f + (float)((hsh >> 8) & 0x7fff)) * ((hsh >> 31) ? -1.f : 1.f);
  const size_t off = plane_off(r, k, rows_pad);
  planes[off] = (_Float16)v;
  planes[ps + off] = (_Float16)(-0.5f * v);
}

// max(., 0) on the live rows of Y | Y2 (bf16x6: gemm_x6 has no ReLU of its own)
__global__ void relu_rows_kernel(float* Y, int ldy, int R, int Nout, RowMask rm) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)R * Nout) return;
  const int r = (int)(i / Nout), c = (int)(i % Nout);
  if (!row_live(rm, r)) return;
  float* p = Y + (size_t)r * ldy + c;
  *p = fmaxf(*p, 0.f);
}

bool off16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

const char* args_error(const lg_linear_args_t& a) {
  if (const char* e = shape_error(a.R, a.K0, a.K, a.Nout)) return e;
  if (!a.A0 || !a.W) return "null A0 / W";
  if (a.K0 < a.K && !a.A1) return "A1 is null with K0 < K";
  if (a.precision != LG_PREC_AUTO && a.precision != LG_PREC_X6 && a.precision != LG_PREC_GEMM_F16) return "bad precision";
  if (a.lda0 < a.K0 || a.lda0 % 4 || (a.K0 < a.K && (a.lda1 < a.K - a.K0 || a.lda1 % 4))) return "bad lda";
  if (off16(a.A0) || off16(a.A1) || off16(a.W) || off16(a.bias) || off16(a.res) || off16(a.res2) || off16(a.Y) ||
      off16(a.Y2) || off16(a.yp) || off16(a.yp_rows) || off16(a.q) || off16(a.kp) || off16(a.vp) || off16(a.cosb) ||
      off16(a.sinb) || off16(a.ln_g) || off16(a.ln_b))
    return "a pointer is not 16-byte aligned";
  if (a.cnt) {
    if (a.mask_B <= 0 || a.mask_M0 < 0 || a.mask_N0 < 0 || (int64_t)a.mask_B * (a.mask_M0 + a.mask_N0) != a.R)
      return "row mask layout does not cover R rows";
  } else if (a.sel) {
    return "sel without cnt";
  }
  const bool planes = a.want_planes != 0;
  switch (a.epi) {
    case LG_LIN_STORE:
      if (!a.Y && !planes) return "no output requested";
      if (planes && !a.yp && a.precision != LG_PREC_X6) return "want_planes without yp";
      if (planes && !a.yp && !a.yp_rows) return "want_planes without yp / yp_rows";
      if ((a.res2 && !a.res) || (a.Y2 && !a.Y)) return "res2 / Y2 without res / Y";
      if (a.res && (a.ldr < a.Nout || a.ldr % 4)) return "bad ldr";
      if (a.Y && (a.ldy < a.Nout || a.ldy % 4)) return "bad ldy";
      if ((a.res2 && (a.res2_row0 < 0 || a.res2_row0 > a.R)) || (a.Y2 && (a.y2_row0 < 0 || a.y2_row0 > a.R)))
        return "bad res2_row0 / y2_row0";
      break;
    case LG_LIN_LN_GELU:
      if (a.Nout != 512) return "LN + GELU needs Nout == 512";
      if (!a.ln_g || !a.ln_b) return "null ln_g / ln_b";
      if (a.precision != LG_PREC_X6 ? !a.yp : !a.yp_rows) return "null yp / yp_rows";
      if (a.ln_route != 0 && a.ln_route != 1) return "bad ln_route";
      break;
    case LG_LIN_QKV_ROT:
    case LG_LIN_CROSS_QKV:
      if (a.Nout != (a.epi == LG_LIN_QKV_ROT ? 768 : 512)) return "QKV epilogue: Nout must be 768 (self) / 512 (cross)";
      if (a.K0 != a.K) return "QKV epilogue: one A operand";
      if (a.H * 64 != 256 || a.B <= 0 || a.M < 0 || a.N < 0 || (int64_t)a.B * (a.M + a.N) != a.R)
        return "QKV epilogue: H * 64 == 256 and B * (M + N) == R";
      if (!a.bias || !a.kp || !a.vp) return "QKV epilogue: null bias / kp / vp";
      if (a.epi == LG_LIN_QKV_ROT && !a.q) return "QKV epilogue: null q";
      if ((a.cosb == nullptr) != (a.sinb == nullptr)) return "cosb and sinb come together";
      if (a.pstride < (int64_t)a.R * 256) return "pstride below R * 256";
      break;
    default: return "bad epi";
  }
  return nullptr;
}

// max over the shards of M[slot] / E[slot] of a host copy of the range table
float tab_max(const unsigned* tab, int slot) {
  float m = 0.f;
  for (int i = 0; i < kRangeShards; ++i) {
    float v;
    memcpy(&v, tab + slot * kRangeStride + i, 4);
    m = std::max(m, v);
  }
  return m;
}
int tab_exp(const unsigned* tab, int slot) { return (int)tab[slot * kRangeStride + kRangeShards]; }

int run_x6(const lg_linear_args_t& a, const Layout& L, char* ws, const RowMask& rm, hipStream_t st) {
  const int R = a.R, Nout = a.Nout;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A0 = a.A0; g.lda0 = a.lda0; g.K0 = a.K0; g.A1 = a.K0 < a.K ? a.A1 : nullptr; g.lda1 = a.lda1;
  g.W = a.W; g.ldw = a.K; g.K = a.K; g.bias = a.bias; g.out_scale = a.out_scale; g.R = R; g.Nout = Nout; g.rm = rm;
  if (a.epi == LG_LIN_QKV_ROT || a.epi == LG_LIN_CROSS_QKV) {
    HeadLayout hl;
    hl.q = a.q ? a.q : reinterpret_cast<float*>(ws + L.qtmp);  // gemm_x6 always writes the fp32 queries
    hl.kp = a.kp; hl.vp = a.vp; hl.pstride = a.pstride; hl.B = a.B; hl.H = a.H; hl.M = a.M; hl.N = a.N;
    hl.cosb = a.cosb; hl.sinb = a.sinb; hl.qk_scale = a.qk_scale;
    if (a.epi == LG_LIN_QKV_ROT && !a.cosb) {  // no rotary: the identity rotation (x * 1 - x' * 0, exact)
      float* c1 = reinterpret_cast<float*>(ws + L.cos1);
      const size_t n = (size_t)R * 32;
      hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c1, 1.f, n);
      LG_HIP(hipGetLastError());
      LG_HIP(hipMemsetAsync(ws + L.sin0, 0, n * 4, st));
      hl.cosb = c1;
      hl.sinb = reinterpret_cast<float*>(ws + L.sin0);
    }
    g.out_scale = 1.f;
    g.hl = hl;
    LG_HIP(gemm_x6(g, a.epi == LG_LIN_QKV_ROT ? EPI_QKV_ROT : EPI_CROSS_QKV, 1, st));
    return LG_OK;
  }
  if (a.epi == LG_LIN_LN_GELU) {
    float* h1 = reinterpret_cast<float*>(ws + L.h1);
    LG_HIP(hipMemsetAsync(h1, 0, (size_t)R * 512 * 4, st));
    g.out_scale = 1.f; g.Y = h1; g.ldy = 512;
    LG_HIP(gemm_x6(g, EPI_STORE, 1, st));
    LG_HIP(layernorm_gelu_512(h1, a.ln_g, a.ln_b, R, nullptr, 0, range_none(), st));
    // the row kernel does not look at the mask: dead rows come back as LN + GELU of a zero row
    LG_HIP(hipMemcpyAsync(a.yp_rows, h1, (size_t)R * 512 * 4, hipMemcpyDeviceToDevice, st));
    return LG_OK;
  }
  // LG_LIN_STORE: one pass per fp32 destination (the rows, and the "planes" stand-in yp_rows)
  for (int pass = 0; pass < 2; ++pass) {
    float* Y = pass == 0 ? a.Y : (a.want_planes ? a.yp_rows : nullptr);
    float* Y2 = pass == 0 ? a.Y2 : nullptr;
    const int ldy = pass == 0 ? a.ldy : Nout;
    if (!Y) continue;
    const size_t rowb = (size_t)Nout * 4;
    GemmArgs p = g;
    p.Y = Y; p.ldy = ldy; p.res = a.res; p.ldr = a.ldr;
    float* ytmp = reinterpret_cast<float*>(ws + L.ytmp);
    if (a.res2) {  // res | res2 as one array
      float* rt = reinterpret_cast<float*>(ws + L.rtmp);
      if (a.res2_row0 > 0)
        LG_HIP(hipMemcpy2DAsync(rt, rowb, a.res, (size_t)a.ldr * 4, rowb, a.res2_row0, hipMemcpyDeviceToDevice, st));
      if (R - a.res2_row0 > 0)
        LG_HIP(hipMemcpy2DAsync(rt + (size_t)a.res2_row0 * Nout, rowb, a.res2, (size_t)a.ldr * 4, rowb, R - a.res2_row0,
                                hipMemcpyDeviceToDevice, st));
      p.res = rt; p.ldr = Nout;
    }
    if (Y2) {  // Y | Y2 as one array, starting from the caller's contents (dead rows keep them)
      if (a.y2_row0 > 0)
        LG_HIP(hipMemcpy2DAsync(ytmp, rowb, Y, (size_t)ldy * 4, rowb, a.y2_row0, hipMemcpyDeviceToDevice, st));
      if (R - a.y2_row0 > 0)
        LG_HIP(hipMemcpy2DAsync(ytmp + (size_t)a.y2_row0 * Nout, rowb, Y2, (size_t)ldy * 4, rowb, R - a.y2_row0,
                                hipMemcpyDeviceToDevice, st));
      p.Y = ytmp; p.ldy = Nout;
    }
    LG_HIP(gemm_x6(p, EPI_STORE, 1, st));
    if (a.relu) {
      const size_t n = (size_t)R * Nout;
      hipLaunchKernelGGL(relu_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p.Y, p.ldy, R, Nout, rm);
      LG_HIP(hipGetLastError());
    }
    if (Y2) {
      if (a.y2_row0 > 0)
        LG_HIP(hipMemcpy2DAsync(Y, (size_t)ldy * 4, ytmp, rowb, rowb, a.y2_row0, hipMemcpyDeviceToDevice, st));
      if (R - a.y2_row0 > 0)
        LG_HIP(hipMemcpy2DAsync(Y2, (size_t)ldy * 4, ytmp + (size_t)a.y2_row0 * Nout, rowb, rowb, R - a.y2_row0,
                                hipMemcpyDeviceToDevice, st));
    }
  }
  return LG_OK;
}

}  // namespace

extern "C" {

int lg_linear_workspace_bytes(int32_t R, int32_t K0, int32_t K, int32_t Nout, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (const char* e = shape_error(R, K0, K, Nout)) return fail(LG_E_INVALID, e);
  *bytes = carve(R, K0, K, Nout).bytes;
  return LG_OK;
}

int lg_linear(lg_linear_args_t* args, void* workspace, size_t workspace_bytes, void* stream) {
  if (!args) return fail(LG_E_INVALID, "null argument");
  lg_linear_args_t& a = *args;
  if (const char* e = args_error(a)) return fail(LG_E_INVALID, e);
  const Layout L = carve(a.R, a.K0, a.K, a.Nout);
  if (!workspace || workspace_bytes < L.bytes) return fail(LG_E_WORKSPACE, "workspace too small (lg_linear_workspace_bytes)");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(LG_E_INVALID, "workspace is not 256-byte aligned");
  a.exp_a0 = a.exp_a1 = a.exp_out = a.exp_out_v = 0;
  a.max_out = a.max_out_v = a.bound_out = 0.f;
  if (a.R == 0) return LG_OK;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const int R = a.R, K0 = a.K0, K = a.K, K1 = K - K0, Nout = a.Nout, RP = L.RP;
  RowMask rm{};
  if (a.cnt) rm = RowMask{a.cnt, a.sel, a.sel_eq, SegLayout{a.mask_B, a.mask_M0, a.mask_N0}};

  if (a.precision == LG_PREC_X6) {
    const int rc = run_x6(a, L, ws, rm, st);
    if (rc != LG_OK) return rc;
    LG_HIP(hipStreamSynchronize(st));
    return LG_OK;
  }

  unsigned* rtab = reinterpret_cast<unsigned*>(ws + L.rtab);
  float* stats = reinterpret_cast<float*>(ws + L.stats);
  _Float16* a0p = reinterpret_cast<_Float16*>(ws + L.a0);
  _Float16* a1p = reinterpret_cast<_Float16*>(ws + L.a1);
  _Float16* wp = reinterpret_cast<_Float16*>(ws + L.w);
  const bool qkv = a.epi == LG_LIN_QKV_ROT || a.epi == LG_LIN_CROSS_QKV;

  // ---- range table, A plane images (each half its own exponent)
  LG_HIP(hipMemsetAsync(rtab, 0, (size_t)kSlots * kRangeStride * sizeof(unsigned), st));
  LG_HIP(hipMemsetAsync(a0p, 0, (size_t)2 * RP * K0 * 2, st));
  if (K1) LG_HIP(hipMemsetAsync(a1p, 0, (size_t)2 * RP * K1 * 2, st));
  auto absmax_half = [&](const float* x, int k, int ld, int slot) {
    if (ld == k && !rm.cnt) return range_absmax(x, (size_t)R * k, rtab, slot, st);
    return range_absmax_rows(x, R, k, ld, 0, rm, rtab, slot, st);  // live rows only, as a ragged batch
  };
  LG_HIP(absmax_half(a.A0, K0, a.lda0, S_IN0));
  if (K1) LG_HIP(absmax_half(a.A1, K1, a.lda1, S_IN1));
  LG_HIP(rows_to_planes(a.A0, R, K0, a.lda0, a0p, RP, 0, RangeOut{rtab, S_IN0, -1, 1.f, 0.f, 0.f, S_A0, kRangeTrack}, st,
                        nullptr, &rm));
  if (K1)
    LG_HIP(rows_to_planes(a.A1, R, K1, a.lda1, a1p, RP, 0, RangeOut{rtab, S_IN1, -1, 1.f, 0.f, 0.f, S_A1, kRangeTrack}, st,
                          nullptr, &rm));
  if (a.poison) {
    const size_t n0 = (size_t)RP * K0, n1 = (size_t)RP * K1;
    hipLaunchKernelGGL(poison_rows_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, a0p, (long long)RP * K0, RP,
                       K0, R, rm);
    if (K1)
      hipLaunchKernelGGL(poison_rows_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, a1p, (long long)RP * K1,
                         RP, K1, R, rm);
    LG_HIP(hipGetLastError());
  }

  // ---- weight planes and range statistics as at load time (one read-back)
  // stats: [0] max|W|; [2,3] L1 / bias max of the whole matrix or the key rows; [4,5] value rows; [6] LN bound
  LG_HIP(hipMemsetAsync(stats, 0, 16 * sizeof(float), st));
  LG_HIP(absmax(a.W, (size_t)Nout * K, stats, st));
  if (qkv) {
    const size_t k0 = a.epi == LG_LIN_QKV_ROT ? 256 : 0, v0 = k0 + 256;
    LG_HIP(weight_range_stats(a.W + k0 * K, 256, K, a.bias + k0, stats + 2, st));
    LG_HIP(weight_range_stats(a.W + v0 * K, 256, K, a.bias + v0, stats + 4, st));
  } else {
    LG_HIP(weight_range_stats(a.W, Nout, K, a.bias, stats + 2, st));
  }
  if (a.epi == LG_LIN_LN_GELU) LG_HIP(layernorm_bound(a.ln_g, a.ln_b, 512, stats + 6, st));
  if (a.res) {
    const int r0 = a.res2 ? a.res2_row0 : R;
    LG_HIP(range_absmax_rows(a.res, r0, Nout, a.ldr, 0, RowMask{}, rtab, S_RES, st));
    if (a.res2) LG_HIP(range_absmax_rows(a.res2, R - r0, Nout, a.ldr, 0, RowMask{}, rtab, S_RES, st));
  }
  float hs[16];
  unsigned htab[kSlots * kRangeStride];
  LG_HIP(hipMemcpyAsync(hs, stats, sizeof(hs), hipMemcpyDeviceToHost, st));
  LG_HIP(hipMemcpyAsync(htab, rtab, sizeof(htab), hipMemcpyDeviceToHost, st));
  LG_HIP(hipStreamSynchronize(st));
  int sw = 0;
  if (hs[0] > 0.f && std::isfinite(hs[0])) {
    int E;
    (void)std::frexp(hs[0], &E);  // max = m 2^E, m in [0.5, 1)
    sw = std::min(std::max(4 - E, -100), 100);
  }
  LG_HIP(split_weight_h3(a.W, Nout, K, std::ldexp(1.f, sw), wp, st));

  GemmH3Args g;
  memset(&g, 0, sizeof(g));
  g.A0 = PlaneRef{a0p, (long long)RP * K0, RP};
  if (K1) g.A1 = PlaneRef{a1p, (long long)RP * K1, RP};
  g.K0 = K0; g.K = K;
  g.W = PlaneRef{wp, (long long)Nout * K, Nout};
  g.R = R; g.Nout = Nout;
  g.h1 = a.precision == LG_PREC_GEMM_F16;  // one fp16 MFMA per product on the high planes: no 2^11
  g.acc_scale = std::ldexp(1.f, g.h1 ? -sw : -(11 + sw));
  g.out_scale = 1.f;
  g.bias = a.bias;
  g.rtab = rtab; g.a0_slot = S_A0; g.a1_slot = K1 ? S_A1 : -1;
  g.rm = rm;
  _Float16* yp = static_cast<_Float16*>(a.yp);
  const long long yps = (long long)RP * Nout;
  const int in1 = K1 ? S_A1 : -1;

  if (a.epi == LG_LIN_STORE) {
    const float os = std::fabs(a.out_scale);
    g.out_scale = a.out_scale; g.relu = a.relu;
    g.res = a.res; g.res2 = a.res2; g.res2_row0 = a.res2_row0; g.ldr = a.ldr;
    g.Y = a.Y; g.Y2 = a.Y2; g.y2_row0 = a.y2_row0; g.ldy = a.ldy;
    if (a.want_planes) {
      g.Yp = yp; g.yps = yps; g.yrows_pad = RP;
      // |res + (A W^T + b) s| <= max|res| + |s| (|W|_1 (M[a0] + M[a1]) + max|b|)
      g.ro = RangeOut{rtab, S_A0, in1, hs[2] * os, hs[2] * os, hs[3] * os + (a.res ? tab_max(htab, S_RES) : 0.f), S_OUT,
                      kRangeTrack};
    }
    LG_HIP(gemm_h3(g, EPI_STORE, st));
  } else if (a.epi == LG_LIN_LN_GELU) {
    const RangeOut ro_h{rtab, -1, -1, 0.f, 0.f, hs[6], S_OUT, kRangeTrack};
    a.bound_out = hs[6];
    if (a.ln_route == 1) {
      float* h1 = reinterpret_cast<float*>(ws + L.h1);
      LG_HIP(hipMemsetAsync(h1, 0, (size_t)R * 512 * 4, st));
      g.Y = h1; g.ldy = 512;
      LG_HIP(gemm_h3(g, EPI_STORE, st));
      LG_HIP(layernorm_gelu_512(h1, a.ln_g, a.ln_b, R, yp, RP, ro_h, st));
    } else {
      g.Yp = yp; g.yps = yps; g.yrows_pad = RP; g.ln_g = a.ln_g; g.ln_b = a.ln_b; g.ro = ro_h;
      LG_HIP(gemm_h3(g, EPI_LN_GELU, st));
    }
  } else {
    HeadLayout hl;
    hl.q = a.q; hl.kp = a.kp; hl.vp = a.vp; hl.pstride = a.pstride; hl.B = a.B; hl.H = a.H; hl.M = a.M; hl.N = a.N;
    hl.cosb = a.cosb; hl.sinb = a.sinb; hl.qk_scale = a.qk_scale;
    g.hl = hl;
    // rotated keys: |k cos - k' sin| <= sqrt(2) max(|k|, |k'|) < 1.5 max; cross: qk * qk_scale
    const float kf = a.epi == LG_LIN_QKV_ROT ? 1.5f : std::fabs(a.qk_scale);
    g.ro = RangeOut{rtab, S_A0, -1, hs[2] * kf, 0.f, hs[3] * kf, S_OUT, kRangeTrack};
    g.ro_v = RangeOut{rtab, S_A0, -1, hs[4], 0.f, hs[5], S_OUTV, kRangeTwoSided | kRangeTrack};
    LG_HIP(gemm_h3(g, a.epi == LG_LIN_QKV_ROT ? EPI_QKV_ROT : EPI_CROSS_QKV, st));
  }
  if (!qkv && a.yp_rows && (a.want_planes || a.epi == LG_LIN_LN_GELU))
    LG_HIP(image_to_rows(yp, yps, RP, Nout, a.yp_rows, R, rtab, S_OUT, st));
  LG_HIP(hipMemcpyAsync(htab, rtab, sizeof(htab), hipMemcpyDeviceToHost, st));
  LG_HIP(hipStreamSynchronize(st));
  a.exp_a0 = tab_exp(htab, S_A0);
  a.exp_a1 = K1 ? tab_exp(htab, S_A1) : a.exp_a0;
  a.exp_out = tab_exp(htab, S_OUT);
  a.exp_out_v = tab_exp(htab, S_OUTV);
  a.max_out = tab_max(htab, S_OUT);
  a.max_out_v = tab_max(htab, S_OUTV);
  return LG_OK;
}

int lg_plane_roundtrip(const float* x, int32_t R, int32_t K, int32_t lshift, int32_t two_sided, float* out,
                       int32_t* exponent, void* stream) {
  if (!x || !out || !exponent) return fail(LG_E_INVALID, "null argument");
  if (R <= 0 || K <= 0 || K % 32 || R > (1 << 20) || K > 4096 || lshift < 0 || lshift > 15)
    return fail(LG_E_INVALID, "bad shape (R > 0, K a positive multiple of 32, lshift in [0, 15])");
  if (off16(x) || off16(out)) return fail(LG_E_INVALID, "a pointer is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int RP = (R + 255) / 256 * 256;
  const size_t tabb = align256((size_t)2 * kRangeStride * sizeof(unsigned)), imgb = (size_t)2 * RP * K * 2;
  char* buf = nullptr;
  LG_HIP(hipMallocAsync((void**)&buf, tabb + imgb, st));
  unsigned* tab = reinterpret_cast<unsigned*>(buf);
  _Float16* img = reinterpret_cast<_Float16*>(buf + tabb);
  unsigned htab[2 * kRangeStride];
  hipError_t e = hipMemsetAsync(buf, 0, tabb + imgb, st);
  if (e == hipSuccess) e = range_absmax(x, (size_t)R * K, tab, 0, st);
  if (e == hipSuccess)
    e = rows_to_planes(x, R, K, K, img, RP, 0,
                       RangeOut{tab, 0, -1, 1.f, 0.f, 0.f, 1, kRangeTrack | (two_sided ? kRangeTwoSided : 0), lshift}, st);
  if (e == hipSuccess) e = image_to_rows(img, (long long)RP * K, RP, K, out, R, tab, 1, st);
  if (e == hipSuccess) e = hipMemcpyAsync(htab, tab, sizeof(htab), hipMemcpyDeviceToHost, st);
  (void)hipFreeAsync(buf, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(LG_E_HIP, std::string("lg_plane_roundtrip: ") + hipGetErrorString(e));
  *exponent = tab_exp(htab, 1);
  return LG_OK;
}

}  // extern "C"
