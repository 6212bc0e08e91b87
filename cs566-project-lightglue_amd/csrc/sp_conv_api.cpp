// C-ABI of the kernel-level SuperPoint entries (include/lightglue_mi355x.h: sp_conv_layer,
// sp_head_scores, sp_head_normalize): one launch of sp_conv3x3 / sp_conv1a on plain fp32 tensors,
// prepared inside the caller's workspace the way sp_load_weights and sp_forward prepare them
// (superpoint_api.cpp), and the two dense-head kernels on the caller's rows.
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

constexpr int kSlots = 4;  // 0: max|x|; 1: the input image; 2: the output image
enum { S_IN = 0, S_X = 1, S_Y = 2 };

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
int rows_pad_for(long long R) { return (int)(((R + 1) + 255) / 256 * 256); }  // >= R + 1: a zero row
bool off16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

struct Layout {
  long long rin, rout;
  int rpx, rpy;
  size_t rtab, stats, xp, wrep, wp, bytes;
};
Layout carve(int B, int H, int W, int Cin, int Cout, int pool, int conv1a) {
  Layout L{};
  L.rin = (long long)B * H * W;
  L.rout = pool ? (long long)B * (H / 2) * (W / 2) : L.rin;
  L.rpx = rows_pad_for(L.rin);
  L.rpy = rows_pad_for(L.rout);
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += align256(n);
    return o;
  };
  L.rtab = take((size_t)kSlots * kRangeStride * sizeof(unsigned));
  L.stats = take(16 * sizeof(float));
  if (!conv1a) {
    L.xp = take((size_t)2 * L.rpx * Cin * 2);
    L.wrep = take((size_t)Cout * 9 * Cin * 4);
    L.wp = take((size_t)2 * Cout * 9 * Cin * 2);
  }
  L.bytes = off;
  return L;
}

// what sp_conv3x3 / sp_conv1a validate, before anything is launched
const char* shape_error(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int pool, int conv1a) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return "negative or empty size";
  if (B * H * W + 1 >= (1LL << 26)) return "B * H * W too large (< 2^26 pixels)";
  if (conv1a) {
    if (Cin != 1 && Cin != 3) return "conv1a: the image has 1 or 3 channels";
    if (Cout != 64) return "conv1a: Cout must be 64";
    if (pool) return "conv1a has no pool";
    return nullptr;
  }
  if (Cin % kKB) return "Cin must be a multiple of 32";
  if (Cout % 64) return "Cout must be a multiple of 64";
  if (Cin > 4096 || Cout > 4096) return "shape too large for the kernel-level entry";
  if (pool && (H < 2 || W < 2)) return "pool needs H >= 2 and W >= 2";
  return nullptr;
}

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

}  // namespace

extern "C" {

int sp_conv_layer_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pool, int32_t conv1a,
                                  size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (const char* e = shape_error(B, H, W, Cin, Cout, pool, conv1a)) return fail(LG_E_INVALID, e);
  *bytes = carve(B, H, W, Cin, Cout, pool, conv1a).bytes;
  return LG_OK;
}

int sp_conv_layer_rows(int32_t B, int32_t H, int32_t W, int32_t pool, int64_t* rout, int32_t* yrows_pad) {
  if (!rout || !yrows_pad) return fail(LG_E_INVALID, "null argument");
  if (B <= 0 || H <= 0 || W <= 0 || (int64_t)B * H * W + 1 >= (1LL << 26)) return fail(LG_E_INVALID, "bad size");
  *rout = pool ? (int64_t)B * (H / 2) * (W / 2) : (int64_t)B * H * W;
  *yrows_pad = rows_pad_for(*rout);
  return LG_OK;
}

int sp_conv_layer(const sp_conv_layer_args_t* args, void* workspace, size_t workspace_bytes, void* stream) {
  if (!args) return fail(LG_E_INVALID, "null argument");
  const sp_conv_layer_args_t& a = *args;
  if (const char* e = shape_error(a.B, a.H, a.W, a.Cin, a.Cout, a.pool, a.conv1a)) return fail(LG_E_INVALID, e);
  if (!a.x || !a.w || !a.bias || !a.y_planes) return fail(LG_E_INVALID, "null x / w / bias / y_planes");
  if (!a.post_scale != !a.post_shift) return fail(LG_E_INVALID, "post_scale and post_shift come together");
  if (off16(a.x) || off16(a.w) || off16(a.bias) || off16(a.post_scale) || off16(a.post_shift) || off16(a.y_rows) ||
      off16(a.y_planes))
    return fail(LG_E_INVALID, "a pointer is not 16-byte aligned");
  const Layout L = carve(a.B, a.H, a.W, a.Cin, a.Cout, a.pool, a.conv1a);
  if (!workspace || workspace_bytes < L.bytes)
    return fail(LG_E_WORKSPACE, "workspace too small (sp_conv_layer_workspace_bytes)");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(LG_E_INVALID, "workspace is not 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const int B = a.B, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
  const bool aff = a.post_scale != nullptr;
  unsigned* rtab = reinterpret_cast<unsigned*>(ws + L.rtab);
  float* stats = reinterpret_cast<float*>(ws + L.stats);
  _Float16* yp = static_cast<_Float16*>(a.y_planes);
  const long long yps = (long long)L.rpy * Cout;

  LG_HIP(hipMemsetAsync(rtab, 0, (size_t)kSlots * kRangeStride * sizeof(unsigned), st));
  LG_HIP(hipMemsetAsync(stats, 0, 16 * sizeof(float), st));
  LG_HIP(range_absmax(a.x, (size_t)L.rin * Cin, rtab, S_IN, st));
  // stats: [0] max|W| of the repacked matrix; [1, 2] its largest row L1 norm, max|bias|; [3, 4] max|s|, max|t|
  const float* wmat = a.w;  // conv1a: [64][1][3][3] is already [64][9]
  if (!a.conv1a) {
    float* wrep = reinterpret_cast<float*>(ws + L.wrep);
    LG_HIP(sp_repack_conv(a.w, Cout, Cin, 3, wrep, st));
    LG_HIP(absmax(wrep, (size_t)Cout * 9 * Cin, stats, st));
    wmat = wrep;
  }
  LG_HIP(weight_range_stats(wmat, Cout, a.conv1a ? 9 : 9 * Cin, a.bias, stats + 1, st));
  if (aff) {
    LG_HIP(absmax(a.post_scale, (size_t)Cout, stats + 3, st));
    LG_HIP(absmax(a.post_shift, (size_t)Cout, stats + 4, st));
  }
  float hs[16];
  LG_HIP(hipMemcpyAsync(hs, stats, sizeof(hs), hipMemcpyDeviceToHost, st));
  LG_HIP(hipStreamSynchronize(st));
  // |relu(conv + b)| <= g M[in] + bmax; with the affine |relu(.) s + t| <= max|s| (g M + bmax) + max|t|
  const float g = hs[1], bmax = hs[2], smax = aff ? hs[3] : 1.f, tmax = aff ? hs[4] : 0.f;
  const int in_slot = a.conv1a ? S_IN : S_X;  // gray weights sum to 1: |gray| <= max|image|
  const RangeOut ro{rtab, in_slot, -1, smax * g, 0.f, smax * bmax + tmax, S_Y, kRangeTrack};

  if (a.conv1a) {
    LG_HIP(sp_conv1a(a.x, B, Cin, H, W, a.w, a.bias, a.post_scale, a.post_shift, yp, L.rpy, ro, st));
  } else {
    _Float16* xp = reinterpret_cast<_Float16*>(ws + L.xp);
    _Float16* wp = reinterpret_cast<_Float16*>(ws + L.wp);
    // the input image: two-sided exponent from max|x| (an input of any magnitude keeps 22 bits)
    LG_HIP(rows_to_planes(a.x, (int)L.rin, Cin, Cin, xp, L.rpx, 0,
                          RangeOut{rtab, S_IN, -1, 1.f, 0.f, 0.f, S_X, kRangeTrack | kRangeTwoSided}, st));
    LG_HIP(sp_zero_rows(xp, (long long)L.rpx * Cin, L.rpx, Cin, (int)L.rin, st));
    int sw = 0;
    if (hs[0] > 0.f && std::isfinite(hs[0])) {
      int E;
      (void)std::frexp(hs[0], &E);  // max = m 2^E, m in [0.5, 1)
      sw = std::min(std::max(4 - E, -100), 100);
    }
    LG_HIP(split_weight_h3(wmat, Cout, 9 * Cin, std::ldexp(1.f, sw), wp, st));
    ConvH3Args c{};
    c.X = {xp, (long long)L.rpx * Cin, L.rpx};
    c.B = B;
    c.H = H;
    c.W = W;
    c.Cin = Cin;
    c.Cout = Cout;
    c.Wt = {wp, (long long)Cout * 9 * Cin, Cout};
    c.acc_scale = std::ldexp(1.f, -(11 + sw));
    c.bias = a.bias;
    c.Y = yp;
    c.yps = yps;
    c.yrows_pad = L.rpy;
    c.rtab = rtab;
    c.x_slot = S_X;
    c.ro = ro;
    c.pool = a.pool ? 1 : 0;
    c.post_scale = a.post_scale;
    c.post_shift = a.post_shift;
    LG_HIP(sp_conv3x3(c, st));
  }
  if (a.y_rows) LG_HIP(image_to_rows(yp, yps, L.rpy, Cout, a.y_rows, (int)L.rout, rtab, S_Y, st));
  unsigned htab[kSlots * kRangeStride];
  LG_HIP(hipMemcpyAsync(htab, rtab, sizeof(htab), hipMemcpyDeviceToHost, st));
  LG_HIP(hipStreamSynchronize(st));
  if (a.exp_in) *a.exp_in = a.conv1a ? 0 : tab_exp(htab, S_X);
  if (a.exp_out) *a.exp_out = tab_exp(htab, S_Y);
  if (a.max_out) *a.max_out = tab_max(htab, S_Y);
  return LG_OK;
}

int sp_head_scores(const float* logits, int32_t ld, int32_t B, int32_t Hc, int32_t Wc, float* scores, void* stream) {
  if (!logits || !scores) return fail(LG_E_INVALID, "null argument");
  if (B <= 0 || Hc <= 0 || Wc <= 0 || ld < 65 || (int64_t)B * Hc * Wc * 64 >= (1LL << 31))
    return fail(LG_E_INVALID, "bad shape (B, Hc, Wc > 0, ld >= 65, B * Hc * Wc * 64 < 2^31)");
  if (off16(scores)) return fail(LG_E_INVALID, "scores is not 16-byte aligned");
  LG_HIP(sp_detector_scores(logits, ld, B, Hc, Wc, scores, (hipStream_t)stream));
  return LG_OK;
}

int sp_head_normalize(const float* x, int32_t rows, float* y, void* stream) {
  if (!x || !y) return fail(LG_E_INVALID, "null argument");
  if (rows <= 0) return fail(LG_E_INVALID, "rows must be positive");
  if (off16(x) || off16(y)) return fail(LG_E_INVALID, "a pointer is not 16-byte aligned");
  LG_HIP(sp_desc_normalize(x, rows, y, (hipStream_t)stream));
  return LG_OK;
}

}  // extern "C"
