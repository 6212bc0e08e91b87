// The AttentionalGNN trunk SuperGlue and GlueStick share (superglue_api.cpp owns the code): the
// packed weights of one AttentionalPropagation layer, their load-time folds, and the layer's four
// launches (QKV GEMM, attention, mlp.0 with merge and BatchNorm folded, mlp.3 + residual).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <vector>

#include "kernels.h"

namespace lg {

struct SgMat {
  size_t off, boff;   // floats into the packed fp32 buffer
  int rows, K;
  size_t poff;        // halfs into the plane buffer
  float unscale;
  float g, bmax;      // row-L1 max, |bias| max
};
struct SgLayer {
  int type;           // 0 self, 1 cross
  SgMat qkv, w1, w2;  // qkv: 768 x 256 (stats: keys / values rows below)
  float gK, bK, gV, bV;
  size_t bn1;         // raw BatchNorm of mlp.1 (folded into w1)
};

// the row buffers a layer works on (rows: image 0 of every pair, then image 1)
struct SgTrunkWork {
  float *X, *Q, *ctx;
  void *KP, *VP;
  _Float16 *Xp, *Cp, *Hp;
  unsigned* rtab;
  int rows_pad;
};

constexpr int kSgTmpFloats = 3 * 256 * 256 + 3 * 256 + 512 * 256 + 512 + 256 * 256;

// perm: qkv_perm [768] | merge_perm [256] (device); 4 * 256 ints
std::vector<int> sg_layer_perm();
// packed offsets of one layer, taken from `take` (floats, 64-aligned)
void sg_layer_layout(SgLayer& ly, int type, const std::function<size_t(size_t)>& take);
// q / k / v stacked and gathered head-major, merge folded into mlp.0, then the eval BatchNorm;
// p = the AttentionalPropagation module's name ("gnn.layers.3", "gnn.layers.3.update"),
// tmp = kSgTmpFloats floats
hipError_t sg_pack_layer(const std::function<float*(const std::string&)>& raw, const std::string& p, SgLayer& ly,
                         float* buf, float* tmp, const int* perm, hipStream_t st);
// fp16x3 plane images (per-matrix power-of-two scale) and range statistics of `mats` (the layers'
// matrices must be among them) and the layers' key / value statistics; `scalars` (device floats)
// are read back in the same transfer.  (Re)allocates *planes.  Synchronises the stream.
hipError_t sg_finish_mats(float* buf, const std::vector<SgMat*>& mats, std::vector<SgLayer>& layers,
                          const std::vector<const float*>& scalars, std::vector<float>& scalars_out, _Float16** planes,
                          hipStream_t st);
// one layer over both images; slots: s_x (in), s_k, s_v, s_h (scratch), s_xn (out)
hipError_t sg_gnn_layer(const SgLayer& ly, const float* W, const _Float16* planes, const SgTrunkWork& w, int B, int M,
                        int N, const RowMask& live, const int* c0, const int* c1, int s_x, int s_k, int s_v, int s_h,
                        int s_xn, hipStream_t st);

}  // namespace lg
