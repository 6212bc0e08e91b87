// ALIKED extractor kernels (aliked.hip), reference gluefactory/models/extractors/aliked.py.
// Feature maps are planar fp32 [B][C][H][W]; the four aggregated pyramid levels are channel-last.
// Convolution weights are repacked to [Cin * k * k][CoP]
// (output channel fastest, CoP = Cout rounded up to 16, zero filled), BatchNorm folded in, so that a
// workgroup reads the weights of its output-channel group through the scalar cache.
#pragma once
#include <hip/hip_runtime.h>

namespace lg {

constexpr int kAkCoPad = 16;
inline int ak_copad(int cout) { return (cout + kAkCoPad - 1) / kAkCoPad * kAkCoPad; }

enum AkAct { AK_NONE = 0, AK_SELU = 1, AK_CLAMP = 2, AK_SIGMOID = 3 };

// w [Cout][co_stride] (element (co, ci, t) at co * co_stride + (ci_off + ci) * kk + t), scale
// [Cout] or null -> wt [Cin * kk][CoP]
hipError_t ak_repack(const float* w, int Cout, int Cin, int kk, int co_stride, int ci_off, const float* scale, float* wt,
                     hipStream_t st);
// dst [n_pad] = src [n] (or 0 when src is null), zero filled
hipError_t ak_pad_vec(const float* src, int n, int n_pad, float* dst, hipStream_t st);
// agg [M][dim][dim] (p, c, d) -> aggT [dim d][M * dim (p, c)]
hipError_t ak_agg_transpose(const float* agg, int M, int dim, float* aggT, hipStream_t st);

struct AkConvArgs {
  const float* X;      // [B][Cin][srcH][srcW]
  int B, Cin, Cout;
  int H, W;            // the convolution's (zero-padded) domain
  int srcH, srcW;      // domain pixel (y, x) reads X at (clamp(y - pt, 0, srcH-1), clamp(x - pl, 0, srcW-1)):
  int pt, pl;          // the replicate padding of the image; srcH = H, pt = 0 elsewhere
  const float* Wt;     // [Cin * 9][CoP]
  const float* bias;   // [CoP]
  const float* res;    // [B][Cout][H][W] or null, added before the activation
  float* Y;            // [B][Cout][outH][outW]: domain pixel (y, x) goes to (y - oy0, x - ox0) when inside
  int outH, outW, oy0, ox0;
  int act;
  float clampv;
};
hipError_t ak_conv3x3(const AkConvArgs& a, hipStream_t st);

// Y [B][Cout][HW] = act(Wt^T X + bias); X [B][Cin][HW]
hipError_t ak_conv1x1(const float* X, int B, int Cin, int Cout, long long HW, const float* Wt, const float* bias, int act,
                      float* Y, hipStream_t st);
// AvgPool2d(k, k): X [BC][H][W] -> Y [BC][H/k][W/k]
hipError_t ak_avgpool(const float* X, long long BC, int H, int W, int k, float* Y, hipStream_t st);

// torchvision.ops.deform_conv2d (3x3, stride 1, padding 1, no mask): X [B][Cin][H][W],
// off [B][18][H][W], Wt [Cin * 9][CoP], bias [CoP], res nullable -> Y [B][Cout][H][W]
hipError_t ak_deform_conv(const float* X, const float* off, int B, int Cin, int Cout, int H, int W, const float* Wt,
                          const float* bias, const float* res, int act, float* Y, hipStream_t st);

// The four aggregated pyramid levels (dq = dim / 4 channels each) and, for the score head, the
// eight-channel partial products of score_head.0 per level
struct AkPyramid {
  const float* A[4];   // [B][h_l][w_l][dq]: channel-last, the sparse readers take all channels of a pixel
  const float* P[4];   // [B][8][h_l][w_l]
  int h[4], w[4];      // h[0] = Hp, w[0] = Wp (the padded size)
  float ry[4], rx[4];  // align_corners source steps (h_l - 1) / (Hp - 1), (w_l - 1) / (Wp - 1); 0 when Hp (Wp) is 1
  int dq;
};
// one level: A = selu(Wt^T X) channel-last and P = Wp^T A; X [B][Cin][HW] planar, Wt [Cin][dq]
// (dq 16 or 32), Wp [dq][16] (8 used)
hipError_t ak_agg(const float* X, int B, int Cin, int dq, long long HW, const float* Wt, const float* Wp, float* A, float* P,
                  hipStream_t st);
// per padded pixel: S8 = selu(P1 + up(P2) + up(P3) + up(P4)) [B][8][Hp][Wp] and
// inv = 1 / max(|x1234|, 1e-12) [B][Hp][Wp], x1234 the concatenation of the upsampled levels
hipError_t ak_head(const AkPyramid& py, int B, float* S8, float* inv, hipStream_t st);

// NMS mask without the borders of `radius` pixels (far borders at image_size (w, h) when given)
hipError_t ak_border_mask(const unsigned char* mask, int B, int H, int W, int radius, const float* image_size,
                          unsigned char* out, hipStream_t st);
// top-k mode: images with fewer than k positive candidates take zero-score pixels, lowest pixel
// index first, up to k
hipError_t ak_fill_zeros(const float* scores, const unsigned char* mask, int B, int H, int W, int k, unsigned* key,
                         int* idx, int* cnt, hipStream_t st);
// per image mean of the score map (threshold mode with no threshold), double accumulation
hipError_t ak_mean(const float* scores, int B, long long HW, float* mean, hipStream_t st);
// DKD's soft-argmax refinement, dispersity and score sampling (aliked.py:167-216) for the selected
// pixels: kn [B][cap][2] in [-1, 1], kpts = (W, H) * (kn + 1) / 2; slots >= n[b] are zero filled
hipError_t ak_refine(const float* scores, const int* sel_idx, const int* n, int B, int cap, int H, int W, int radius,
                     float* kn, float* kpts, float* sampled, float* disp, hipStream_t st);

struct AkSddh {
  AkPyramid py;
  const float* inv;    // [B][Hp][Wp]
  int pt, pl, H, W;    // the unpadded map is rows pt .. pt+H-1, columns pl .. pl+W-1 of the padded one
  int B, cap, dim, M;
  const float* kn;     // [B][cap][2]
};
// offsets [B][cap][2M]: conv3x3 on the 3x3 patch + SELU + 1x1, clamped (aliked.py:525-542)
hipError_t ak_sddh_offsets(const AkSddh& s, const float* W0t, const float* b0, const float* W1t, const float* b1,
                           float* offs, hipStream_t st);
// F [B * cap * M][dim]: the normalised map sampled at kpt + offset (aliked.py:556-566)
hipError_t ak_sddh_sample(const AkSddh& s, const float* offs, float* F, hipStream_t st);
hipError_t ak_selu(float* x, long long n, hipStream_t st);
// rows of dim -> x / max(|x|, 1e-12)
hipError_t ak_l2norm(const float* x, long long rows, int dim, float* y, hipStream_t st);

}  // namespace lg
