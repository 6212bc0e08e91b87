// ALIKED extractor kernels for gfx950 (reference gluefactory/models/extractors/aliked.py): the
// encoder's direct convolutions, the deformable convolution, the aggregation / score head on the
// pyramid levels (the concatenated full-resolution map is never written), DKD's refinement and the
// SDDH descriptor head's gathers.  DESIGN.md §9c.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "aliked.h"

namespace lg {
namespace {

__device__ __forceinline__ float selu_f(float x) {
  // torch.selu: scale * (max(0, x) + min(0, alpha * (exp(x) - 1)))
  constexpr float kScale = 1.0507009873554804934193349852946f;
  constexpr float kNeg = 1.0507009873554804934193349852946f * 1.6732632423543772848170429916717f;
  return x > 0.f ? kScale * x : kNeg * expm1f(x);
}
__device__ __forceinline__ float act_f(float v, int act, float clampv) {
  if (act == AK_SELU) return selu_f(v);
  if (act == AK_CLAMP) return fminf(fmaxf(v, -clampv), clampv);
  if (act == AK_SIGMOID) return 1.f / (1.f + expf(-v));
  return v;
}
__device__ __forceinline__ unsigned order_key(float v) {  // as superpoint.hip
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
unsigned blocks_for(long long n, int block) { return (unsigned)std::max<long long>(1, (n + block - 1) / block); }

// ---- weight repacking --------------------------------------------------------------------------
__global__ void ak_repack_kernel(const float* w, int Cout, int Cin, int kk, int co_stride, int ci_off, const float* scale,
                                 float* wt, int CoP) {
  const int n = Cin * kk * CoP;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int co = i % CoP, r = i / CoP;  // r = ci * kk + t
    float v = 0.f;
    if (co < Cout) {
      v = w[(size_t)co * co_stride + (size_t)ci_off * kk + r];
      if (scale) v *= scale[co];
    }
    wt[i] = v;
  }
}
__global__ void ak_pad_vec_kernel(const float* src, int n, int n_pad, float* dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pad) dst[i] = (src && i < n) ? src[i] : 0.f;
}
__global__ void ak_agg_transpose_kernel(const float* agg, int M, int dim, float* aggT) {
  const long long n = (long long)M * dim * dim;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int pc = (int)(i % ((long long)M * dim)), d = (int)(i / ((long long)M * dim));
    aggT[i] = agg[(size_t)pc * dim + d];
  }
}

// ---- 3x3 convolution ---------------------------------------------------------------------------
// A 32 x 8 pixel tile per workgroup, one pixel and CO_T output channels per thread.  The input
// halo tile of 8 channels at a time goes through LDS; the weights of the group are uniform over
// the workgroup (scalar loads).
constexpr int kTX = 32, kTY = 8, kCI = 8;
template <int CO_T>
__global__ __launch_bounds__(256) void ak_conv3x3_kernel(AkConvArgs a, int CoP, int ngroups) {
  __shared__ float tile[kCI][kTY + 2][kTX + 2];
  const int b = blockIdx.z / ngroups, co0 = (blockIdx.z % ngroups) * CO_T;
  const int tx = threadIdx.x % kTX, ty = threadIdx.x / kTX;
  const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
  float acc[CO_T];
#pragma unroll
  for (int j = 0; j < CO_T; ++j) acc[j] = 0.f;
  const size_t splane = (size_t)a.srcH * a.srcW;
  for (int c0 = 0; c0 < a.Cin; c0 += kCI) {
    const int nc = min(kCI, a.Cin - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < nc * (kTY + 2) * (kTX + 2); i += 256) {
      const int c = i / ((kTY + 2) * (kTX + 2)), rem = i % ((kTY + 2) * (kTX + 2));
      const int yy = rem / (kTX + 2), xx = rem % (kTX + 2);
      const int y = y0 + yy - 1, x = x0 + xx - 1;
      float v = 0.f;
      if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
        const int sy = min(max(y - a.pt, 0), a.srcH - 1), sx = min(max(x - a.pl, 0), a.srcW - 1);
        v = a.X[((size_t)b * a.Cin + c0 + c) * splane + (size_t)sy * a.srcW + sx];
      }
      tile[c][yy][xx] = v;
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      float v[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) v[t] = tile[c][ty + t / 3][tx + t % 3];
      const float* w = a.Wt + (size_t)(c0 + c) * 9 * CoP + co0;
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < CO_T; ++j) acc[j] = fmaf(v[t], w[t * CoP + j], acc[j]);
    }
  }
  const int y = y0 + ty, x = x0 + tx;
  if (y >= a.H || x >= a.W) return;
  const int oy = y - a.oy0, ox = x - a.ox0;
  if ((unsigned)oy >= (unsigned)a.outH || (unsigned)ox >= (unsigned)a.outW) return;
#pragma unroll
  for (int j = 0; j < CO_T; ++j) {
    const int co = co0 + j;
    if (co >= a.Cout) break;
    float v = acc[j] + a.bias[co];
    if (a.res) v += a.res[((size_t)b * a.Cout + co) * a.H * a.W + (size_t)y * a.W + x];
    a.Y[((size_t)b * a.Cout + co) * a.outH * a.outW + (size_t)oy * a.outW + ox] = act_f(v, a.act, a.clampv);
  }
}

// ---- 1x1 convolution ---------------------------------------------------------------------------
template <int CO_T>
__global__ __launch_bounds__(256) void ak_conv1x1_kernel(const float* X, int Cin, int Cout, long long HW, const float* Wt,
                                                         const float* bias, int act, float* Y, int CoP) {
  const int b = blockIdx.z, co0 = blockIdx.y * CO_T;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  float acc[CO_T];
#pragma unroll
  for (int j = 0; j < CO_T; ++j) acc[j] = 0.f;
  const float* xb = X + (size_t)b * Cin * HW + p;
  for (int c = 0; c < Cin; ++c) {
    const float v = xb[(size_t)c * HW];
    const float* w = Wt + (size_t)c * CoP + co0;
#pragma unroll
    for (int j = 0; j < CO_T; ++j) acc[j] = fmaf(v, w[j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < CO_T; ++j) {
    const int co = co0 + j;
    if (co >= Cout) break;
    Y[((size_t)b * Cout + co) * HW + p] = act_f(acc[j] + bias[co], act, 0.f);
  }
}

__global__ void ak_avgpool_kernel(const float* X, long long BC, int H, int W, int k, float* Y) {
  const int Ho = H / k, Wo = W / k;
  const long long n = BC * Ho * Wo;
  const float inv = 1.f / (float)(k * k);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const long long pc = i / ((long long)Wo * Ho);
    const float* src = X + (size_t)pc * H * W + (size_t)yo * k * W + (size_t)xo * k;
    float s = 0.f;
    for (int dy = 0; dy < k; ++dy)
      for (int dx = 0; dx < k; ++dx) s += src[(size_t)dy * W + dx];
    Y[i] = s * inv;
  }
}

// ---- deformable 3x3 convolution ----------------------------------------------------------------
// 64 pixels per workgroup.  The four bilinear corners of every (tap, pixel) are set up once, the
// sampled columns of 8 input channels at a time go through LDS, and wave g accumulates output
// channels g * CO_T .. for the 64 pixels (weights uniform per wave).
constexpr int kDP = 64, kDCI = 8;
template <int CO_T>
__global__ __launch_bounds__(256) void ak_deform_kernel(const float* X, const float* off, int Cin, int Cout, int H, int W,
                                                        const float* Wt, const float* bias, const float* res, int act,
                                                        float* Y, int CoP) {
  __shared__ int sidx[9 * kDP][4];
  __shared__ float swt[9 * kDP][4];
  __shared__ float col[kDCI][9][kDP];
  const int b = blockIdx.y, HW = H * W, p0 = blockIdx.x * kDP;
  for (int i = threadIdx.x; i < 9 * kDP; i += 256) {
    const int k = i / kDP, pix = p0 + i % kDP;
    int id[4] = {0, 0, 0, 0};
    float wt[4] = {0.f, 0.f, 0.f, 0.f};
    if (pix < HW) {
      const int y = pix / W, x = pix - y * W;
      const float py = (float)(y - 1 + k / 3) + off[((size_t)b * 18 + 2 * k) * HW + pix];
      const float px = (float)(x - 1 + k % 3) + off[((size_t)b * 18 + 2 * k + 1) * HW + pix];
      if (py > -1.f && py < (float)H && px > -1.f && px < (float)W) {
        const float fy = floorf(py), fx = floorf(px);
        const int yl = (int)fy, xl = (int)fx, yh = yl + 1, xh = xl + 1;
        const float ly = py - fy, lx = px - fx, hy = 1.f - ly, hx = 1.f - lx;
        const bool oyl = yl >= 0, oxl = xl >= 0, oyh = yh <= H - 1, oxh = xh <= W - 1;
        if (oyl && oxl) { id[0] = yl * W + xl; wt[0] = hy * hx; }
        if (oyl && oxh) { id[1] = yl * W + xh; wt[1] = hy * lx; }
        if (oyh && oxl) { id[2] = yh * W + xl; wt[2] = ly * hx; }
        if (oyh && oxh) { id[3] = yh * W + xh; wt[3] = ly * lx; }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sidx[i][q] = id[q];
      swt[i][q] = wt[q];
    }
  }
  const int p = threadIdx.x % kDP;
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x / kDP);
  float acc[CO_T];
#pragma unroll
  for (int j = 0; j < CO_T; ++j) acc[j] = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += kDCI) {
    const int nc = min(kDCI, Cin - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < nc * 9 * kDP; i += 256) {
      const int c = i / (9 * kDP), kp = i % (9 * kDP);
      const float* xc = X + ((size_t)b * Cin + c0 + c) * HW;
      const float v = swt[kp][0] * xc[sidx[kp][0]] + swt[kp][1] * xc[sidx[kp][1]] + swt[kp][2] * xc[sidx[kp][2]] +
                      swt[kp][3] * xc[sidx[kp][3]];
      (&col[c][0][0])[kp] = v;
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      const float* w = Wt + (size_t)(c0 + c) * 9 * CoP + g * CO_T;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float v = col[c][t][p];
#pragma unroll
        for (int j = 0; j < CO_T; ++j) acc[j] = fmaf(v, w[t * CoP + j], acc[j]);
      }
    }
  }
  const int pix = p0 + p;
  if (pix >= HW) return;
#pragma unroll
  for (int j = 0; j < CO_T; ++j) {
    const int co = g * CO_T + j;
    if (co >= Cout) break;
    const size_t o = ((size_t)b * Cout + co) * HW + pix;
    float v = acc[j] + bias[co];
    if (res) v += res[o];
    Y[o] = act_f(v, act, 0.f);
  }
}

// ---- bilinear align_corners=True upsampling: the four source taps of a full-resolution pixel ----
// (torch's upsample_bilinear2d: scale = (in - 1) / (out - 1) in fp32 -- AkPyramid::ry / rx, formed
// on the host -- and the low index by truncation)
struct Taps {
  int i00, i01, i10, i11;  // pixel indices into the level
  float ly0, ly1, lx0, lx1;
};
__device__ __forceinline__ Taps up_taps(int Y, int X, float ry, float rx, int h, int w) {
  const float sy = ry * (float)Y, sx = rx * (float)X;
  const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
  const int yp = y0 < h - 1 ? 1 : 0, xp = x0 < w - 1 ? 1 : 0;
  Taps t;
  t.ly1 = sy - (float)y0;
  t.ly0 = 1.f - t.ly1;
  t.lx1 = sx - (float)x0;
  t.lx0 = 1.f - t.lx1;
  t.i00 = y0 * w + x0;
  t.i01 = t.i00 + xp;
  t.i10 = t.i00 + yp * w;
  t.i11 = t.i10 + xp;
  return t;
}
__device__ __forceinline__ float up_value(const float* m, const Taps& t) {  // planar map
  return t.ly0 * (t.lx0 * m[t.i00] + t.lx1 * m[t.i01]) + t.ly1 * (t.lx0 * m[t.i10] + t.lx1 * m[t.i11]);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float up1(float a, float b, float c, float d, const Taps& t) {
  return t.ly0 * (t.lx0 * a + t.lx1 * b) + t.ly1 * (t.lx0 * c + t.lx1 * d);
}
// four consecutive channels of a channel-last level [hw][dq] (m points at the image's channel c)
__device__ __forceinline__ float4 up_value4(const float* m, int dq, const Taps& t) {
  const float4 a = ld4(m + (size_t)t.i00 * dq), b = ld4(m + (size_t)t.i01 * dq), c = ld4(m + (size_t)t.i10 * dq),
               d = ld4(m + (size_t)t.i11 * dq);
  return make_float4(up1(a.x, b.x, c.x, d.x, t), up1(a.y, b.y, c.y, d.y, t), up1(a.z, b.z, c.z, d.z, t),
                     up1(a.w, b.w, c.w, d.w, t));
}

// ---- aggregation: A = selu(conv1x1(X)) written channel-last, and the score head's partial products
// P = W_l A from the registers (score_head.0 is linear and bilinear upsampling is linear, so the
// 8-channel products are formed per level and upsampled, never the dim-channel concatenation)
template <int DQ>
__global__ __launch_bounds__(256) void ak_agg_kernel(const float* X, int Cin, long long HW, const float* Wt, const float* Wp,
                                                     float* A, float* P) {
  const int b = blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  float acc[DQ];
#pragma unroll
  for (int j = 0; j < DQ; ++j) acc[j] = 0.f;
  const float* xb = X + (size_t)b * Cin * HW + p;
  for (int c = 0; c < Cin; ++c) {
    const float v = xb[(size_t)c * HW];
    const float* w = Wt + (size_t)c * DQ;
#pragma unroll
    for (int j = 0; j < DQ; ++j) acc[j] = fmaf(v, w[j], acc[j]);
  }
  float pp[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) pp[q] = 0.f;
  float* ab = A + ((size_t)b * HW + p) * DQ;
#pragma unroll
  for (int j = 0; j < DQ; ++j) {
    acc[j] = selu_f(acc[j]);
#pragma unroll
    for (int q = 0; q < 8; ++q) pp[q] = fmaf(acc[j], Wp[j * kAkCoPad + q], pp[q]);
  }
#pragma unroll
  for (int j = 0; j < DQ; j += 4) *reinterpret_cast<float4*>(ab + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
#pragma unroll
  for (int q = 0; q < 8; ++q) P[((size_t)b * 8 + q) * HW + p] = pp[q];
}

__global__ __launch_bounds__(256) void ak_head_kernel(AkPyramid py, float* S8, float* inv) {
  const int b = blockIdx.y, Hp = py.h[0], Wp = py.w[0], dq = py.dq;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= Hp * Wp) return;
  const int Y = pix / Wp, X = pix - Y * Wp;
  const size_t HW = (size_t)Hp * Wp;
  float s8[8];
  float n2 = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s8[j] = py.P[0][((size_t)b * 8 + j) * HW + pix];
  const float* a0 = py.A[0] + ((size_t)b * HW + pix) * dq;
  for (int c = 0; c < dq; c += 4) {
    const float4 v = ld4(a0 + c);
    n2 = fmaf(v.x, v.x, n2);
    n2 = fmaf(v.y, v.y, n2);
    n2 = fmaf(v.z, v.z, n2);
    n2 = fmaf(v.w, v.w, n2);
  }
  for (int l = 1; l < 4; ++l) {
    const Taps t = up_taps(Y, X, py.ry[l], py.rx[l], py.h[l], py.w[l]);
    const size_t hw = (size_t)py.h[l] * py.w[l];
#pragma unroll
    for (int j = 0; j < 8; ++j) s8[j] += up_value(py.P[l] + ((size_t)b * 8 + j) * hw, t);
    const float* al = py.A[l] + (size_t)b * hw * dq;
    for (int c = 0; c < dq; c += 4) {
      const float4 v = up_value4(al + c, dq, t);
      n2 = fmaf(v.x, v.x, n2);
      n2 = fmaf(v.y, v.y, n2);
      n2 = fmaf(v.z, v.z, n2);
      n2 = fmaf(v.w, v.w, n2);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) S8[((size_t)b * 8 + j) * HW + pix] = selu_f(s8[j]);
  inv[(size_t)b * HW + pix] = 1.f / fmaxf(sqrtf(n2), 1e-12f);
}

// channels c .. c+3 (c a multiple of 4: one level) of the normalised feature map at the padded pixel (Y, X)
__device__ __forceinline__ float4 feat4_at(const AkPyramid& py, const float* inv, int b, int c, int Y, int X) {
  const int l = c / py.dq, cl = c - l * py.dq, Wp = py.w[0];
  const size_t HW = (size_t)py.h[0] * Wp, pix = (size_t)Y * Wp + X;
  const float nv = inv[(size_t)b * HW + pix];
  float4 v;
  if (l == 0) {
    v = ld4(py.A[0] + ((size_t)b * HW + pix) * py.dq + cl);
  } else {
    const Taps t = up_taps(Y, X, py.ry[l], py.rx[l], py.h[l], py.w[l]);
    v = up_value4(py.A[l] + (size_t)b * py.h[l] * py.w[l] * py.dq + cl, py.dq, t);
  }
  return make_float4(nv * v.x, nv * v.y, nv * v.z, nv * v.w);
}

// ---- DKD ---------------------------------------------------------------------------------------
__global__ void ak_border_mask_kernel(const unsigned char* mask, int H, int W, int r, const float* image_size,
                                      unsigned char* out) {
  const int b = blockIdx.y;
  int y1 = H - r, x1 = W - r;
  if (image_size) {  // image_size[i].long(): truncation
    x1 = (int)image_size[2 * b] - r;
    y1 = (int)image_size[2 * b + 1] - r;
  }
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < H * W; p += gridDim.x * blockDim.x) {
    const int y = p / W, x = p - y * W;
    const size_t o = (size_t)b * H * W + p;
    out[o] = mask[o] && y >= r && x >= r && y < y1 && x < x1;
  }
}

__global__ __launch_bounds__(1024) void ak_fill_zeros_kernel(const float* scores, const unsigned char* mask, int HW, int k,
                                                             unsigned* key, int* idx, int* cnt) {
  __shared__ int wtot[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int c = cnt[b];
  // one more than k where the map has it: sp_select sorts only when it has more than k to choose from
  const int k1 = min(k + 1, HW);
  if (c >= k1) return;  // uniform
  const size_t base = (size_t)b * HW;
  for (int p0 = 0; p0 < HW && c < k1; p0 += 1024) {
    const int p = p0 + tid;
    const bool f = p < HW && !(mask[base + p] && scores[base + p] > 0.f);
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wtot[wv] = __popcll(bal);
    __syncthreads();
    int offw = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
      if (w < wv) offw += wtot[w];
      total += wtot[w];
    }
    const int pos = c + offw + before;
    if (f && pos < k1) {
      key[base + pos] = order_key(0.f);
      idx[base + pos] = p;
    }
    c = min(k1, c + total);
  }
  __syncthreads();
  if (tid == 0) cnt[b] = c;
}

__global__ __launch_bounds__(256) void ak_mean_kernel(const float* scores, long long HW, float* mean) {
  __shared__ double part[256];
  const int b = blockIdx.x;
  double s = 0.0;
  for (long long i = threadIdx.x; i < HW; i += 256) s += (double)scores[(size_t)b * HW + i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) mean[b] = (float)(part[0] / (double)HW);
}

// grid_sample(bilinear, align_corners=True, zeros) of one channel at the normalised (gx, gy)
__device__ __forceinline__ void gs_setup(float g, int size, int& i0, float& w0, float& w1) {
  float ix = ((g + 1.f) / 2.f) * (float)(size - 1);
  ix = fminf(fmaxf(ix, -2.f), (float)size + 1.f);  // beyond: every tap is outside anyway (and NaN -> -2)
  const float f = floorf(ix);
  i0 = (int)f;
  w1 = ix - f;           // weight of i0 + 1
  w0 = (f + 1.f) - ix;   // weight of i0
}

__global__ void ak_refine_kernel(const float* scores, const int* sel_idx, const int* n, int B, int cap, int H, int W, int r,
                                 float* kn, float* kpts, float* sampled, float* disp) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * cap) return;
  const int b = (int)(t / cap), i = (int)(t - (long long)b * cap);
  if (i >= n[b]) {
    kn[2 * t] = kn[2 * t + 1] = 0.f;
    kpts[2 * t] = kpts[2 * t + 1] = 0.f;
    sampled[t] = 0.f;
    disp[t] = 0.f;
    return;
  }
  const float* s = scores + (size_t)b * H * W;
  const int p = min(max(sel_idx[t], 0), H * W - 1), y = p / W, x = p - y * W;
  constexpr float kInvT = 1.f / 0.1f;
  float mx = -INFINITY;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const int yy = y + dy, xx = x + dx;
      const float v = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? s[(size_t)yy * W + xx] : 0.f;
      mx = fmaxf(mx, v);
    }
  float s0 = 0.f, sx = 0.f, sy = 0.f;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const int yy = y + dy, xx = x + dx;
      const float v = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? s[(size_t)yy * W + xx] : 0.f;
      const float e = expf((v - mx) * kInvT);
      s0 += e;
      sx += e * (float)dx;
      sy += e * (float)dy;
    }
  const float rx = sx / s0, ry = sy / s0;
  float d = 0.f;
  const float fr = (float)r;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const int yy = y + dy, xx = x + dx;
      const float v = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? s[(size_t)yy * W + xx] : 0.f;
      const float e = expf((v - mx) * kInvT);
      const float ux = ((float)dx - rx) / fr, uy = ((float)dy - ry) / fr;
      d += e * (ux * ux + uy * uy);
    }
  const float gx = ((float)x + rx) / (float)(W - 1) * 2.f - 1.f;
  const float gy = ((float)y + ry) / (float)(H - 1) * 2.f - 1.f;
  int x0, y0;
  float wx0, wx1, wy0, wy1;
  gs_setup(gx, W, x0, wx0, wx1);
  gs_setup(gy, H, y0, wy0, wy1);
  float v = 0.f;
  const bool ox0 = (unsigned)x0 < (unsigned)W, ox1 = (unsigned)(x0 + 1) < (unsigned)W;
  const bool oy0 = (unsigned)y0 < (unsigned)H, oy1 = (unsigned)(y0 + 1) < (unsigned)H;
  if (oy0 && ox0) v += s[(size_t)y0 * W + x0] * (wx0 * wy0);
  if (oy0 && ox1) v += s[(size_t)y0 * W + x0 + 1] * (wx1 * wy0);
  if (oy1 && ox0) v += s[(size_t)(y0 + 1) * W + x0] * (wx0 * wy1);
  if (oy1 && ox1) v += s[(size_t)(y0 + 1) * W + x0 + 1] * (wx1 * wy1);
  kn[2 * t] = gx;
  kn[2 * t + 1] = gy;
  kpts[2 * t] = (float)W * (gx + 1.f) / 2.f;
  kpts[2 * t + 1] = (float)H * (gy + 1.f) / 2.f;
  sampled[t] = v;
  disp[t] = d / s0;
}

// ---- SDDH --------------------------------------------------------------------------------------
// keypoint position in pixels of the unpadded map: (k / 2 + 0.5) * (size - 1)
__device__ __forceinline__ float kpt_px(float g, int size) { return (g / 2.f + 0.5f) * (float)(size - 1); }
// get_patches' corner: (long(k) - ps / 2 + 1).long() clamped to [0, size - 1 - ps], ps = 3
__device__ __forceinline__ int patch_corner(float kpx, int size) {
  const float kc = fminf(fmaxf(kpx, -1.f), (float)size);  // keeps the conversion defined
  const int l = (int)kc;                                   // .long(): truncation
  const int c = (int)((float)l - 0.5f);                    // truncation again
  return min(max(c, 0), size - 4);
}

constexpr int kSdKP = 8;  // keypoints per workgroup
__global__ __launch_bounds__(256) void ak_sddh_offsets_kernel(AkSddh s, const float* W0t, const float* b0, const float* W1t,
                                                              const float* b1, float* offs) {
  __shared__ float patch[kSdKP][128 * 9];
  __shared__ float hid[kSdKP][64];
  const int b = blockIdx.y, n0 = blockIdx.x * kSdKP, C2 = 2 * s.M, K9 = s.dim * 9;
  const int D4 = s.dim / 4;
  for (int i = threadIdx.x; i < kSdKP * 9 * D4; i += 256) {  // channels fastest: the levels are channel-last
    const int kp = i / (9 * D4), rem = i - kp * 9 * D4, t = rem / D4, c = 4 * (rem - t * D4);
    const int n = n0 + kp;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < s.cap) {
      const float* k = s.kn + ((size_t)b * s.cap + n) * 2;
      const int cx = patch_corner(kpt_px(k[0], s.W), s.W), cy = patch_corner(kpt_px(k[1], s.H), s.H);
      v = feat4_at(s.py, s.inv, b, c, s.pt + cy + t / 3, s.pl + cx + t % 3);
    }
    patch[kp][c * 9 + t] = v.x;
    patch[kp][(c + 1) * 9 + t] = v.y;
    patch[kp][(c + 2) * 9 + t] = v.z;
    patch[kp][(c + 3) * 9 + t] = v.w;
  }
  __syncthreads();
  const int j = threadIdx.x % C2, g = threadIdx.x / C2, G = 256 / C2;  // G = 8 (M 16) or 4 (M 32)
  float acc[2] = {0.f, 0.f};
  for (int r = 0; r < K9; ++r) {
    const float w = W0t[(size_t)r * C2 + j];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int kp = g + q * G;
      if (kp < kSdKP) acc[q] = fmaf(w, patch[kp][r], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int kp = g + q * G;
    if (kp < kSdKP) hid[kp][j] = selu_f(acc[q] + b0[j]);
  }
  __syncthreads();
  const float mo = (float)max(s.H, s.W) / 4.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int kp = g + q * G, n = n0 + kp;
    if (kp >= kSdKP || n >= s.cap) continue;
    float o = b1[j];
    for (int i = 0; i < C2; ++i) o = fmaf(W1t[(size_t)i * C2 + j], hid[kp][i], o);
    offs[((size_t)b * s.cap + n) * C2 + j] = fminf(fmaxf(o, -mo), mo);
  }
}

__device__ __forceinline__ void axpy4(float4& a, float w, const float4& v) {
  a.x = fmaf(w, v.x, a.x);
  a.y = fmaf(w, v.y, a.y);
  a.z = fmaf(w, v.z, a.z);
  a.w = fmaf(w, v.w, a.w);
}
// four channels per thread: dim / 4 threads per row
__global__ __launch_bounds__(256) void ak_sddh_sample_kernel(AkSddh s, const float* offs, float* F) {
  const int tpr = s.dim / 4, rpb = 256 / tpr;
  const long long rows = (long long)s.B * s.cap * s.M;
  const long long row = (long long)blockIdx.x * rpb + threadIdx.x / tpr;
  const int c = 4 * (threadIdx.x % tpr);
  if (row >= rows) return;
  const int p = (int)(row % s.M);
  const long long bn = row / s.M;
  const int b = (int)(bn / s.cap);
  const float* k = s.kn + (size_t)bn * 2;
  const float* o = offs + (size_t)bn * 2 * s.M;
  // pos = kpt + offset (channel p: x, M + p: y), 2 pos / (size - 1) - 1, then grid_sample's own mapping
  const float px = kpt_px(k[0], s.W) + o[p], py = kpt_px(k[1], s.H) + o[s.M + p];
  const float gx = 2.f * px / (float)(s.W - 1) - 1.f, gy = 2.f * py / (float)(s.H - 1) - 1.f;
  int x0, y0;
  float wx0, wx1, wy0, wy1;
  gs_setup(gx, s.W, x0, wx0, wx1);
  gs_setup(gy, s.H, y0, wy0, wy1);
  const bool ox0 = (unsigned)x0 < (unsigned)s.W, ox1 = (unsigned)(x0 + 1) < (unsigned)s.W;
  const bool oy0 = (unsigned)y0 < (unsigned)s.H, oy1 = (unsigned)(y0 + 1) < (unsigned)s.H;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (oy0 && ox0) axpy4(v, wx0 * wy0, feat4_at(s.py, s.inv, b, c, s.pt + y0, s.pl + x0));
  if (oy0 && ox1) axpy4(v, wx1 * wy0, feat4_at(s.py, s.inv, b, c, s.pt + y0, s.pl + x0 + 1));
  if (oy1 && ox0) axpy4(v, wx0 * wy1, feat4_at(s.py, s.inv, b, c, s.pt + y0 + 1, s.pl + x0));
  if (oy1 && ox1) axpy4(v, wx1 * wy1, feat4_at(s.py, s.inv, b, c, s.pt + y0 + 1, s.pl + x0 + 1));
  *reinterpret_cast<float4*>(F + (size_t)row * s.dim + c) = v;
}

__global__ void ak_selu_kernel(float* x, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    x[i] = selu_f(x[i]);
}

// one wave per row
__global__ __launch_bounds__(256) void ak_l2norm_kernel(const float* x, long long rows, int dim, float* y) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float s = 0.f;
  for (int c = lane; c < dim; c += 64) {
    const float v = x[(size_t)row * dim + c];
    s = fmaf(v, v, s);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float inv = 1.f / fmaxf(sqrtf(s), 1e-12f);
  for (int c = lane; c < dim; c += 64) y[(size_t)row * dim + c] = x[(size_t)row * dim + c] * inv;
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------
hipError_t ak_repack(const float* w, int Cout, int Cin, int kk, int co_stride, int ci_off, const float* scale, float* wt,
                     hipStream_t st) {
  const int CoP = ak_copad(Cout);
  hipLaunchKernelGGL(ak_repack_kernel, dim3(std::min(1024u, blocks_for((long long)Cin * kk * CoP, 256))), dim3(256), 0, st, w,
                     Cout, Cin, kk, co_stride, ci_off, scale, wt, CoP);
  return hipGetLastError();
}
hipError_t ak_pad_vec(const float* src, int n, int n_pad, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(ak_pad_vec_kernel, dim3(blocks_for(n_pad, 256)), dim3(256), 0, st, src, n, n_pad, dst);
  return hipGetLastError();
}
hipError_t ak_agg_transpose(const float* agg, int M, int dim, float* aggT, hipStream_t st) {
  hipLaunchKernelGGL(ak_agg_transpose_kernel, dim3(std::min(2048u, blocks_for((long long)M * dim * dim, 256))), dim3(256), 0,
                     st, agg, M, dim, aggT);
  return hipGetLastError();
}

hipError_t ak_conv3x3(const AkConvArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const int CoP = ak_copad(a.Cout);
  const int cot = a.Cout % 16 == 0 ? 16 : (a.Cout > 4 ? 8 : 4);
  const int ng = (a.Cout + cot - 1) / cot;
  if ((long long)a.B * ng > 65535) return hipErrorInvalidValue;
  const dim3 grid((a.W + kTX - 1) / kTX, (a.H + kTY - 1) / kTY, a.B * ng);
  if (cot == 16)
    hipLaunchKernelGGL(ak_conv3x3_kernel<16>, grid, dim3(256), 0, st, a, CoP, ng);
  else if (cot == 8)
    hipLaunchKernelGGL(ak_conv3x3_kernel<8>, grid, dim3(256), 0, st, a, CoP, ng);
  else
    hipLaunchKernelGGL(ak_conv3x3_kernel<4>, grid, dim3(256), 0, st, a, CoP, ng);
  return hipGetLastError();
}

hipError_t ak_conv1x1(const float* X, int B, int Cin, int Cout, long long HW, const float* Wt, const float* bias, int act,
                      float* Y, hipStream_t st) {
  if (B <= 0 || HW <= 0) return hipSuccess;
  const int CoP = ak_copad(Cout);
  if (B > 65535) return hipErrorInvalidValue;
  if (Cout % 16 == 0) {
    const dim3 grid(blocks_for(HW, 256), Cout / 16, B);
    hipLaunchKernelGGL(ak_conv1x1_kernel<16>, grid, dim3(256), 0, st, X, Cin, Cout, HW, Wt, bias, act, Y, CoP);
  } else {
    const dim3 grid(blocks_for(HW, 256), (Cout + 7) / 8, B);
    hipLaunchKernelGGL(ak_conv1x1_kernel<8>, grid, dim3(256), 0, st, X, Cin, Cout, HW, Wt, bias, act, Y, CoP);
  }
  return hipGetLastError();
}

hipError_t ak_avgpool(const float* X, long long BC, int H, int W, int k, float* Y, hipStream_t st) {
  const long long n = BC * (H / k) * (W / k);
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ak_avgpool_kernel, dim3(std::min(65535u, blocks_for(n, 256))), dim3(256), 0, st, X, BC, H, W, k, Y);
  return hipGetLastError();
}

hipError_t ak_deform_conv(const float* X, const float* off, int B, int Cin, int Cout, int H, int W, const float* Wt,
                          const float* bias, const float* res, int act, float* Y, hipStream_t st) {
  if (B <= 0 || H <= 0 || W <= 0) return hipSuccess;
  if (B > 65535 || (long long)H * W > (1ll << 30)) return hipErrorInvalidValue;
  const int CoP = ak_copad(Cout);
  const dim3 grid((H * W + kDP - 1) / kDP, B);
#define AK_DEFORM(T) \
  hipLaunchKernelGGL(ak_deform_kernel<T>, grid, dim3(256), 0, st, X, off, Cin, Cout, H, W, Wt, bias, res, act, Y, CoP)
  switch (Cout) {
    case 32: AK_DEFORM(8); break;
    case 64: AK_DEFORM(16); break;
    case 128: AK_DEFORM(32); break;
    default: return hipErrorInvalidValue;
  }
#undef AK_DEFORM
  return hipGetLastError();
}

hipError_t ak_agg(const float* X, int B, int Cin, int dq, long long HW, const float* Wt, const float* Wp, float* A, float* P,
                  hipStream_t st) {
  if (B <= 0 || HW <= 0) return hipSuccess;
  if (B > 65535) return hipErrorInvalidValue;
  const dim3 grid(blocks_for(HW, 256), B);
  if (dq == 32)
    hipLaunchKernelGGL(ak_agg_kernel<32>, grid, dim3(256), 0, st, X, Cin, HW, Wt, Wp, A, P);
  else if (dq == 16)
    hipLaunchKernelGGL(ak_agg_kernel<16>, grid, dim3(256), 0, st, X, Cin, HW, Wt, Wp, A, P);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t ak_head(const AkPyramid& py, int B, float* S8, float* inv, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const dim3 grid(blocks_for((long long)py.h[0] * py.w[0], 256), B);
  hipLaunchKernelGGL(ak_head_kernel, grid, dim3(256), 0, st, py, S8, inv);
  return hipGetLastError();
}

hipError_t ak_border_mask(const unsigned char* mask, int B, int H, int W, int radius, const float* image_size,
                          unsigned char* out, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const dim3 grid(std::min(1024u, blocks_for((long long)H * W, 256)), B);
  hipLaunchKernelGGL(ak_border_mask_kernel, grid, dim3(256), 0, st, mask, H, W, radius, image_size, out);
  return hipGetLastError();
}
hipError_t ak_fill_zeros(const float* scores, const unsigned char* mask, int B, int H, int W, int k, unsigned* key, int* idx,
                         int* cnt, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (k > H * W) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ak_fill_zeros_kernel, dim3(B), dim3(1024), 0, st, scores, mask, H * W, k, key, idx, cnt);
  return hipGetLastError();
}
hipError_t ak_mean(const float* scores, int B, long long HW, float* mean, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(ak_mean_kernel, dim3(B), dim3(256), 0, st, scores, HW, mean);
  return hipGetLastError();
}
hipError_t ak_refine(const float* scores, const int* sel_idx, const int* n, int B, int cap, int H, int W, int radius,
                     float* kn, float* kpts, float* sampled, float* disp, hipStream_t st) {
  if (B <= 0 || cap <= 0) return hipSuccess;
  hipLaunchKernelGGL(ak_refine_kernel, dim3(blocks_for((long long)B * cap, 128)), dim3(128), 0, st, scores, sel_idx, n, B, cap,
                     H, W, radius, kn, kpts, sampled, disp);
  return hipGetLastError();
}

hipError_t ak_sddh_offsets(const AkSddh& s, const float* W0t, const float* b0, const float* W1t, const float* b1, float* offs,
                           hipStream_t st) {
  if (s.B <= 0 || s.cap <= 0) return hipSuccess;
  if (s.dim > 128 || 2 * s.M > 64 || 256 % (2 * s.M) != 0 || 256 / (2 * s.M) * 2 < kSdKP || s.B > 65535)
    return hipErrorInvalidValue;
  const dim3 grid((s.cap + kSdKP - 1) / kSdKP, s.B);
  hipLaunchKernelGGL(ak_sddh_offsets_kernel, grid, dim3(256), 0, st, s, W0t, b0, W1t, b1, offs);
  return hipGetLastError();
}
hipError_t ak_sddh_sample(const AkSddh& s, const float* offs, float* F, hipStream_t st) {
  if (s.B <= 0 || s.cap <= 0) return hipSuccess;
  if (s.dim > 256 || s.dim % 16 != 0 || 256 % (s.dim / 4) != 0 || s.py.dq % 4 != 0) return hipErrorInvalidValue;
  const long long rows = (long long)s.B * s.cap * s.M;
  const int rpb = 256 / (s.dim / 4);
  const long long blocks = (rows + rpb - 1) / rpb;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ak_sddh_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, st, s, offs, F);
  return hipGetLastError();
}
hipError_t ak_selu(float* x, long long n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ak_selu_kernel, dim3(std::min(65535u, blocks_for(n, 256))), dim3(256), 0, st, x, n);
  return hipGetLastError();
}
hipError_t ak_l2norm(const float* x, long long rows, int dim, float* y, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(ak_l2norm_kernel, dim3(blocks_for(rows, 4)), dim3(256), 0, st, x, rows, dim, y);
  return hipGetLastError();
}

}  // namespace lg
