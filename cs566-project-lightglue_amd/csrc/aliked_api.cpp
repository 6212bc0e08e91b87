// C-ABI of the ALIKED extractor (include/aliked_mi355x.h): handle, weight repacking with the
// BatchNorm folded in, and the eval forward orchestration (reference
// gluefactory/models/extractors/aliked.py:732-783).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/aliked_mi355x.h"
#include "../../include/lightglue_mi355x.h"
#include "aliked.h"
#include "api_common.h"
#include "kernels.h"

namespace {

constexpr float kBnEps = 1e-5f;      // nn.BatchNorm2d default
constexpr int kNLimitMax = 20000;    // aliked.py:603

// how a convolution's weights reach the kernels
enum Kind { K_BN3, K_BIAS3, K_BIAS1, K_PLAIN1, K_PLAIN3, K_SLICE1 };
struct Layer {
  std::string conv;  // module name of the convolution
  std::string bn;    // module name of its BatchNorm (K_BN3)
  Kind kind;
  int cin, cout;
  int slice;         // K_SLICE1: input-channel offset into the [cout][4 cin] weight
  size_t w = 0, b = 0;  // floats into gbuf
};
enum {
  L_B1C1, L_B1C2, L_B2C1, L_B2C2, L_B2D,
  L_B3O1, L_B3R1, L_B3O2, L_B3R2, L_B3D,
  L_B4O1, L_B4R1, L_B4O2, L_B4R2, L_B4D,
  L_AG1, L_AG2, L_AG3, L_AG4, L_SP1, L_SP2, L_SP3, L_SP4, L_S2, L_S4, L_S6, L_COUNT
};

size_t a64(size_t n) { return (n + 63) & ~size_t(63); }  // floats: 256-byte steps

}  // namespace

struct sp_aliked_handle {
  sp_aliked_config_t cfg;
  int device;
  lg::WeightSchema schema;
  std::vector<Layer> layers;
  float* gbuf = nullptr;
  size_t gfloats = 0;
  size_t w0t = 0, b0 = 0, w1t = 0, b1 = 0, sf = 0, aggT = 0, tmp_s = 0, tmp_t = 0;
  bool loaded = false;
  bool profile = false;        // sp_aliked_set_profile: stage boundaries of the last forward as events
  hipEvent_t ev[6] = {};
  bool ev_valid = false;
};

namespace {

void build(sp_aliked_handle* h) {
  const auto& c = h->cfg;
  const int dq = c.dim / 4, C2 = 2 * c.M;
  auto& L = h->layers;
  L.resize(L_COUNT);
  L[L_B1C1] = {"block1.conv1", "block1.bn1", K_BN3, 3, c.c1, 0};
  L[L_B1C2] = {"block1.conv2", "block1.bn2", K_BN3, c.c1, c.c1, 0};
  L[L_B2C1] = {"block2.conv1", "block2.bn1", K_BN3, c.c1, c.c2, 0};
  L[L_B2C2] = {"block2.conv2", "block2.bn2", K_BN3, c.c2, c.c2, 0};
  L[L_B2D] = {"block2.downsample", "", K_BIAS1, c.c1, c.c2, 0};
  L[L_B3O1] = {"block3.conv1.offset_conv", "", K_BIAS3, c.c2, 18, 0};
  L[L_B3R1] = {"block3.conv1.regular_conv", "block3.bn1", K_BN3, c.c2, c.c3, 0};
  L[L_B3O2] = {"block3.conv2.offset_conv", "", K_BIAS3, c.c3, 18, 0};
  L[L_B3R2] = {"block3.conv2.regular_conv", "block3.bn2", K_BN3, c.c3, c.c3, 0};
  L[L_B3D] = {"block3.downsample", "", K_BIAS1, c.c2, c.c3, 0};
  L[L_B4O1] = {"block4.conv1.offset_conv", "", K_BIAS3, c.c3, 18, 0};
  L[L_B4R1] = {"block4.conv1.regular_conv", "block4.bn1", K_BN3, c.c3, c.c4, 0};
  L[L_B4O2] = {"block4.conv2.offset_conv", "", K_BIAS3, c.c4, 18, 0};
  L[L_B4R2] = {"block4.conv2.regular_conv", "block4.bn2", K_BN3, c.c4, c.c4, 0};
  L[L_B4D] = {"block4.downsample", "", K_BIAS1, c.c3, c.c4, 0};
  L[L_AG1] = {"conv1", "", K_PLAIN1, c.c1, dq, 0};
  L[L_AG2] = {"conv2", "", K_PLAIN1, c.c2, dq, 0};
  L[L_AG3] = {"conv3", "", K_PLAIN1, c.c3, dq, 0};
  L[L_AG4] = {"conv4", "", K_PLAIN1, c.dim, dq, 0};
  for (int l = 0; l < 4; ++l) L[L_SP1 + l] = {"score_head.0", "", K_SLICE1, dq, 8, l * dq};
  L[L_S2] = {"score_head.2", "", K_PLAIN3, 8, 4, 0};
  L[L_S4] = {"score_head.4", "", K_PLAIN3, 4, 4, 0};
  L[L_S6] = {"score_head.6", "", K_PLAIN3, 4, 1, 0};

  // the reference's state_dict order (a module's own parameters before its children's)
  auto& S = h->schema;
  auto bn = [&](const std::string& n, int ch) {
    for (const char* t : {"weight", "bias", "running_mean", "running_var"}) S.add(n + "." + t, ch);
  };
  auto block = [&](const std::string& n, int ci, int co, bool dcn, bool down) {
    int cin = ci;
    for (int i = 1; i <= 2; ++i) {
      const std::string cv = n + ".conv" + std::to_string(i);
      if (dcn) {
        S.add(cv + ".offset_conv.weight", (int64_t)18 * cin * 9);
        S.add(cv + ".offset_conv.bias", 18);
        S.add(cv + ".regular_conv.weight", (int64_t)co * cin * 9);
      } else {
        S.add(cv + ".weight", (int64_t)co * cin * 9);
      }
      bn(n + ".bn" + std::to_string(i), co);
      cin = co;
    }
    if (down) {
      S.add(n + ".downsample.weight", (int64_t)co * ci);
      S.add(n + ".downsample.bias", co);
    }
  };
  block("block1", 3, c.c1, false, false);
  block("block2", c.c1, c.c2, false, true);
  block("block3", c.c2, c.c3, true, true);
  block("block4", c.c3, c.c4, true, true);
  S.add("conv1.weight", (int64_t)dq * c.c1);
  S.add("conv2.weight", (int64_t)dq * c.c2);
  S.add("conv3.weight", (int64_t)dq * c.c3);
  S.add("conv4.weight", (int64_t)dq * c.dim);
  S.add("score_head.0.weight", (int64_t)8 * c.dim);
  S.add("score_head.2.weight", 4 * 8 * 9);
  S.add("score_head.4.weight", 4 * 4 * 9);
  S.add("score_head.6.weight", 1 * 4 * 9);
  S.add("desc_head.agg_weights", (int64_t)c.M * c.dim * c.dim);
  S.add("desc_head.offset_conv.0.weight", (int64_t)C2 * c.dim * 9);
  S.add("desc_head.offset_conv.0.bias", C2);
  S.add("desc_head.offset_conv.2.weight", (int64_t)C2 * C2);
  S.add("desc_head.offset_conv.2.bias", C2);
  S.add("desc_head.sf_conv.weight", (int64_t)c.dim * c.dim);

  size_t o = 0;
  auto take = [&](size_t n) {
    const size_t r = o;
    o += a64(n);
    return r;
  };
  for (auto& l : L) {
    const int kk = (l.kind == K_BN3 || l.kind == K_BIAS3 || l.kind == K_PLAIN3) ? 9 : 1;
    l.w = take((size_t)l.cin * kk * lg::ak_copad(l.cout));
    l.b = take(lg::ak_copad(l.cout));
  }
  h->w0t = take((size_t)c.dim * 9 * C2);
  h->b0 = take(C2);
  h->w1t = take((size_t)C2 * C2);
  h->b1 = take(C2);
  h->sf = take((size_t)c.dim * c.dim);
  h->aggT = take((size_t)c.M * c.dim * c.dim);
  h->tmp_s = take(256);
  h->tmp_t = take(256);
  h->gfloats = o;
}

struct Geo {
  int B, H, W, Hp, Wp, pt, pl, cap;
  int h[4], w[4];
  size_t hw[4];
};
Geo make_geo(int B, int H, int W, int cap) {
  Geo g{};
  g.B = B;
  g.H = H;
  g.W = W;
  g.cap = cap;
  const int ph = (32 - H % 32) % 32, pw = (32 - W % 32) % 32;  // InputPadder, aliked.py:246-256
  g.pt = ph / 2;
  g.pl = pw / 2;
  g.Hp = H + ph;
  g.Wp = W + pw;
  const int div[4] = {1, 2, 8, 32};
  for (int l = 0; l < 4; ++l) {
    g.h[l] = g.Hp / div[l];
    g.w[l] = g.Wp / div[l];
    g.hw[l] = (size_t)g.h[l] * g.w[l];
  }
  return g;
}

struct Work {
  float *t1a, *x1, *p2, *d2, *t2, *x2, *p3, *off, *d3, *t3, *x3, *p4, *d4, *t4, *x4;
  float *A[4], *P[4], *S8, *inv, *s4a, *s4b;
  unsigned char *mask, *sup, *mask2;
  float *ss, *sel_score, *kn, *mean, *offs, *F, *Y1, *D;
  unsigned* key;
  int *idx, *blk, *cnt, *nsel, *sel_idx;
  size_t bytes;
};
Work carve(char* base, const sp_aliked_config_t& c, const Geo& g) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += (bytes + 255) & ~size_t(255);
    return p;
  };
  auto fl = [&](size_t n) { return reinterpret_cast<float*>(take(n * sizeof(float))); };
  const size_t B = g.B;
  const int dq = c.dim / 4;
  Work w{};
  w.t1a = fl(B * std::max(c.c1, 8) * g.hw[0]);
  w.x1 = fl(B * c.c1 * g.hw[0]);
  w.p2 = fl(B * c.c1 * g.hw[1]);
  w.d2 = fl(B * c.c2 * g.hw[1]);
  w.t2 = fl(B * c.c2 * g.hw[1]);
  w.x2 = fl(B * c.c2 * g.hw[1]);
  w.p3 = fl(B * c.c2 * g.hw[2]);
  w.off = fl(B * 18 * g.hw[2]);
  w.d3 = fl(B * c.c3 * g.hw[2]);
  w.t3 = fl(B * c.c3 * g.hw[2]);
  w.x3 = fl(B * c.c3 * g.hw[2]);
  w.p4 = fl(B * c.c3 * g.hw[3]);
  w.d4 = fl(B * c.c4 * g.hw[3]);
  w.t4 = fl(B * c.c4 * g.hw[3]);
  w.x4 = fl(B * c.c4 * g.hw[3]);
  for (int l = 0; l < 4; ++l) w.A[l] = fl(B * dq * g.hw[l]);
  w.P[0] = w.t1a;  // block1's first map is dead once x1 exists
  for (int l = 1; l < 4; ++l) w.P[l] = fl(B * 8 * g.hw[l]);
  w.S8 = fl(B * 8 * g.hw[0]);
  w.inv = fl(B * g.hw[0]);
  w.s4a = fl(B * 4 * g.hw[0]);
  w.s4b = fl(B * 4 * g.hw[0]);
  const size_t HW = (size_t)g.H * g.W;
  w.mask = reinterpret_cast<unsigned char*>(take(B * HW));
  w.sup = reinterpret_cast<unsigned char*>(take(B * HW));
  w.mask2 = reinterpret_cast<unsigned char*>(take(B * HW));
  w.ss = fl(B * HW);
  w.key = reinterpret_cast<unsigned*>(take(B * HW * 4));
  w.idx = reinterpret_cast<int*>(take(B * HW * 4));
  w.blk = reinterpret_cast<int*>(take(B * (size_t)lg::sp_cand_blocks(g.H) * 4));
  w.cnt = reinterpret_cast<int*>(take(B * 4));
  w.nsel = reinterpret_cast<int*>(take(B * 4));
  w.mean = fl(B);
  w.sel_idx = reinterpret_cast<int*>(take(B * (size_t)g.cap * 4));
  w.sel_score = fl(B * g.cap);
  w.kn = fl(B * g.cap * 2);
  w.offs = fl(B * g.cap * 2 * c.M);
  w.F = fl(B * g.cap * c.M * c.dim);
  w.Y1 = fl(B * g.cap * c.M * c.dim);
  w.D = fl(B * g.cap * c.dim);
  w.bytes = o;
  return w;
}

bool topk_mode(const sp_aliked_config_t& c) { return c.detection_threshold <= 0.f && c.max_num_keypoints > 0; }
int n_limit(const sp_aliked_config_t& c) { return c.max_num_keypoints > 0 ? c.max_num_keypoints : kNLimitMax; }

int check_shape(const sp_aliked_handle* h, int B, int H, int W, int cap) {
  if (B < 0 || H < 8 || W < 8) return fail(LG_E_INVALID, "sp_aliked: the image must be at least 8 x 8");
  if ((long long)B * (H + 31) * (W + 31) * 8 > 0x7fffffffll * 4)
    return fail(LG_E_INVALID, "sp_aliked: batch too large for one call");
  const long long HW = (long long)H * W;
  if (topk_mode(h->cfg)) {
    if (h->cfg.max_num_keypoints > lg::kSpSelectMax || h->cfg.max_num_keypoints > HW)
      return fail(LG_E_INVALID, "sp_aliked: max_num_keypoints must be at most 16384 and at most H * W");
    if (cap < h->cfg.max_num_keypoints) return fail(LG_E_INVALID, "sp_aliked: capacity below max_num_keypoints");
  } else if (cap < std::min<long long>(n_limit(h->cfg), HW)) {
    return fail(LG_E_INVALID, "sp_aliked: capacity below min(n_limit, H * W)");
  }
  if ((long long)B * cap * h->cfg.M > 0x7fffffffll) return fail(LG_E_INVALID, "sp_aliked: too many keypoints for one call");
  return LG_OK;
}

}  // namespace

extern "C" {

int sp_aliked_create(const sp_aliked_config_t* cfg, int device, sp_aliked_handle_t** out) {
  if (!cfg || !out) return fail(LG_E_INVALID, "sp_aliked_create: null argument");
  const auto& c = *cfg;
  for (int ch : {c.c1, c.c2, c.c3, c.c4})
    if (ch < 8 || ch > 128 || ch % 8 != 0) return fail(LG_E_INVALID, "sp_aliked_create: widths must be multiples of 8 in 8..128");
  if ((c.c3 != 32 && c.c3 != 64 && c.c3 != 128) || (c.c4 != 32 && c.c4 != 64 && c.c4 != 128))
    return fail(LG_E_INVALID, "sp_aliked_create: the deformable blocks take c3, c4 in {32, 64, 128}");
  if (c.dim != c.c4 || (c.dim != 64 && c.dim != 128)) return fail(LG_E_INVALID, "sp_aliked_create: dim must equal c4: 64 or 128");
  if (c.M != 16 && c.M != 32) return fail(LG_E_INVALID, "sp_aliked_create: M must be 16 or 32");
  if (c.nms_radius < 1 || c.nms_radius > 8) return fail(LG_E_INVALID, "sp_aliked_create: nms_radius must be in 1..8");
  LG_HIP(hipSetDevice(device));
  auto* h = new sp_aliked_handle();
  h->cfg = c;
  h->device = device;
  build(h);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->gbuf), h->gfloats * sizeof(float));
  if (e != hipSuccess) {
    delete h;
    return fail(LG_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  *out = h;
  return LG_OK;
}

int sp_aliked_destroy(sp_aliked_handle_t* h) {
  if (!h) return LG_OK;
  if (h->gbuf) (void)hipFree(h->gbuf);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  delete h;
  return LG_OK;
}

int sp_aliked_weight_count(const sp_aliked_handle_t* h) { return h ? lg::weight_count(h->schema) : 0; }
const char* sp_aliked_weight_name(const sp_aliked_handle_t* h, int i) { return h ? lg::weight_name(h->schema, i) : nullptr; }
int64_t sp_aliked_weight_numel(const sp_aliked_handle_t* h, int i) { return h ? lg::weight_numel(h->schema, i) : -1; }

int sp_aliked_load_weights(sp_aliked_handle_t* h, int n, const char* const* names, const float* const* tensors,
                           const int64_t* numels, void* stream) {
  if (!h || !names || !tensors || !numels) return fail(LG_E_INVALID, "sp_aliked_load_weights: null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  LG_HIP(hipSetDevice(h->device));
  std::vector<int> src;
  std::string err;
  if (!h->schema.match(n, names, tensors, numels, src, err)) return fail(LG_E_WEIGHTS, err);
  auto got = [&](const std::string& name) { return tensors[src[h->schema.find(name)]]; };
  h->loaded = false;
  float* G = h->gbuf;
  for (const auto& l : h->layers) {
    const int kk = (l.kind == K_BN3 || l.kind == K_BIAS3 || l.kind == K_PLAIN3) ? 9 : 1;
    const int CoP = lg::ak_copad(l.cout);
    const float* w = got(l.conv + ".weight");
    if (l.kind == K_BN3) {
      LG_HIP(lg::sp_bn_fold(got(l.bn + ".weight"), got(l.bn + ".bias"), got(l.bn + ".running_mean"),
                            got(l.bn + ".running_var"), l.cout, kBnEps, G + h->tmp_s, G + h->tmp_t, nullptr, st));
      LG_HIP(lg::ak_repack(w, l.cout, l.cin, kk, l.cin * kk, 0, G + h->tmp_s, G + l.w, st));
      LG_HIP(lg::ak_pad_vec(G + h->tmp_t, l.cout, CoP, G + l.b, st));
    } else if (l.kind == K_SLICE1) {
      LG_HIP(lg::ak_repack(w, l.cout, l.cin, 1, 4 * l.cin, l.slice, nullptr, G + l.w, st));
      LG_HIP(lg::ak_pad_vec(nullptr, 0, CoP, G + l.b, st));
    } else {
      LG_HIP(lg::ak_repack(w, l.cout, l.cin, kk, l.cin * kk, 0, nullptr, G + l.w, st));
      const bool has_bias = l.kind == K_BIAS3 || l.kind == K_BIAS1;
      LG_HIP(lg::ak_pad_vec(has_bias ? got(l.conv + ".bias") : nullptr, l.cout, CoP, G + l.b, st));
    }
  }
  const auto& c = h->cfg;
  const int C2 = 2 * c.M;
  LG_HIP(lg::ak_repack(got("desc_head.offset_conv.0.weight"), C2, c.dim, 9, c.dim * 9, 0, nullptr, G + h->w0t, st));
  LG_HIP(lg::ak_pad_vec(got("desc_head.offset_conv.0.bias"), C2, C2, G + h->b0, st));
  LG_HIP(lg::ak_repack(got("desc_head.offset_conv.2.weight"), C2, C2, 1, C2, 0, nullptr, G + h->w1t, st));
  LG_HIP(lg::ak_pad_vec(got("desc_head.offset_conv.2.bias"), C2, C2, G + h->b1, st));
  LG_HIP(hipMemcpyAsync(G + h->sf, got("desc_head.sf_conv.weight"), (size_t)c.dim * c.dim * sizeof(float),
                        hipMemcpyDeviceToDevice, st));
  LG_HIP(lg::ak_agg_transpose(got("desc_head.agg_weights"), c.M, c.dim, G + h->aggT, st));
  h->loaded = true;
  return LG_OK;
}

int sp_aliked_workspace_bytes(const sp_aliked_handle_t* h, int32_t B, int32_t H, int32_t W, int32_t capacity, size_t* bytes) {
  if (!h || !bytes) return fail(LG_E_INVALID, "sp_aliked_workspace_bytes: null argument");
  if (int rc = check_shape(h, B, H, W, capacity)) return rc;
  *bytes = carve(nullptr, h->cfg, make_geo(B, H, W, capacity)).bytes;
  return LG_OK;
}

int sp_aliked_forward(sp_aliked_handle_t* h, const sp_aliked_inputs_t* in, sp_aliked_outputs_t* out, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (!h || !in || !out) return fail(LG_E_INVALID, "sp_aliked_forward: null argument");
  if (!h->loaded) return fail(LG_E_WEIGHTS, "sp_aliked_forward: no weights loaded");
  if (int rc = check_shape(h, in->B, in->H, in->W, out->capacity)) return rc;
  if (in->B == 0) return LG_OK;
  if (!in->image || !out->score_map || !out->keypoints || !out->descriptors || !out->sampled_scores || !out->dispersity ||
      !out->counts || !workspace)
    return fail(LG_E_INVALID, "sp_aliked_forward: null buffer");
  const auto& c = h->cfg;
  const Geo g = make_geo(in->B, in->H, in->W, out->capacity);
  const Work w = carve(static_cast<char*>(workspace), c, g);
  if (workspace_bytes < w.bytes) return fail(LG_E_WORKSPACE, "sp_aliked_forward: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  LG_HIP(hipSetDevice(h->device));
  const float* G = h->gbuf;
  const auto& L = h->layers;
  const int B = g.B;
  h->ev_valid = false;
  auto mark = [&](int i) -> hipError_t {
    if (!h->profile) return hipSuccess;
    if (!h->ev[i]) {
      hipError_t e = hipEventCreate(&h->ev[i]);
      if (e != hipSuccess) return e;
    }
    return hipEventRecord(h->ev[i], st);
  };
  LG_HIP(mark(0));

  auto conv3 = [&](int li, const float* X, int lvl, const float* res, int act, float* Y) {
    lg::AkConvArgs a{};
    a.X = X;
    a.B = B;
    a.Cin = L[li].cin;
    a.Cout = L[li].cout;
    a.H = a.srcH = a.outH = g.h[lvl];
    a.W = a.srcW = a.outW = g.w[lvl];
    a.Wt = G + L[li].w;
    a.bias = G + L[li].b;
    a.res = res;
    a.Y = Y;
    a.act = act;
    a.clampv = (float)std::max(g.h[lvl], g.w[lvl]) / 4.f;
    return a;
  };
  auto conv1 = [&](int li, const float* X, int lvl, int act, float* Y) {
    return lg::ak_conv1x1(X, B, L[li].cin, L[li].cout, (long long)g.hw[lvl], G + L[li].w, G + L[li].b, act, Y, st);
  };
  auto deform = [&](int li, const float* X, int lvl, const float* res, float* Y) {
    return lg::ak_deform_conv(X, w.off, B, L[li].cin, L[li].cout, g.h[lvl], g.w[lvl], G + L[li].w, G + L[li].b, res,
                              lg::AK_SELU, Y, st);
  };

  // ---- encoder (aliked.py:738-745)
  {
    lg::AkConvArgs a = conv3(L_B1C1, in->image, 0, nullptr, lg::AK_SELU, w.t1a);
    a.srcH = g.H;
    a.srcW = g.W;
    a.pt = g.pt;
    a.pl = g.pl;
    LG_HIP(lg::ak_conv3x3(a, st));
  }
  LG_HIP(lg::ak_conv3x3(conv3(L_B1C2, w.t1a, 0, nullptr, lg::AK_SELU, w.x1), st));
  LG_HIP(lg::ak_avgpool(w.x1, (long long)B * c.c1, g.h[0], g.w[0], 2, w.p2, st));
  LG_HIP(conv1(L_B2D, w.p2, 1, lg::AK_NONE, w.d2));
  LG_HIP(lg::ak_conv3x3(conv3(L_B2C1, w.p2, 1, nullptr, lg::AK_SELU, w.t2), st));
  LG_HIP(lg::ak_conv3x3(conv3(L_B2C2, w.t2, 1, w.d2, lg::AK_SELU, w.x2), st));
  LG_HIP(lg::ak_avgpool(w.x2, (long long)B * c.c2, g.h[1], g.w[1], 4, w.p3, st));
  LG_HIP(mark(1));
  LG_HIP(conv1(L_B3D, w.p3, 2, lg::AK_NONE, w.d3));
  LG_HIP(lg::ak_conv3x3(conv3(L_B3O1, w.p3, 2, nullptr, lg::AK_CLAMP, w.off), st));
  LG_HIP(deform(L_B3R1, w.p3, 2, nullptr, w.t3));
  LG_HIP(lg::ak_conv3x3(conv3(L_B3O2, w.t3, 2, nullptr, lg::AK_CLAMP, w.off), st));
  LG_HIP(deform(L_B3R2, w.t3, 2, w.d3, w.x3));
  LG_HIP(lg::ak_avgpool(w.x3, (long long)B * c.c3, g.h[2], g.w[2], 4, w.p4, st));
  LG_HIP(conv1(L_B4D, w.p4, 3, lg::AK_NONE, w.d4));
  LG_HIP(lg::ak_conv3x3(conv3(L_B4O1, w.p4, 3, nullptr, lg::AK_CLAMP, w.off), st));
  LG_HIP(deform(L_B4R1, w.p4, 3, nullptr, w.t4));
  LG_HIP(lg::ak_conv3x3(conv3(L_B4O2, w.t4, 3, nullptr, lg::AK_CLAMP, w.off), st));
  LG_HIP(deform(L_B4R2, w.t4, 3, w.d4, w.x4));

  LG_HIP(mark(2));
  // ---- aggregation and score head on the pyramid levels (aliked.py:747-757)
  const float* xs[4] = {w.x1, w.x2, w.x3, w.x4};
  lg::AkPyramid py{};
  py.dq = c.dim / 4;
  for (int l = 0; l < 4; ++l) {
    LG_HIP(lg::ak_agg(xs[l], B, L[L_AG1 + l].cin, py.dq, (long long)g.hw[l], G + L[L_AG1 + l].w, G + L[L_SP1 + l].w, w.A[l],
                      w.P[l], st));
    py.A[l] = w.A[l];
    py.P[l] = w.P[l];
    py.h[l] = g.h[l];
    py.w[l] = g.w[l];
    py.ry[l] = g.Hp > 1 ? (float)(g.h[l] - 1) / (float)(g.Hp - 1) : 0.f;
    py.rx[l] = g.Wp > 1 ? (float)(g.w[l] - 1) / (float)(g.Wp - 1) : 0.f;
  }
  LG_HIP(lg::ak_head(py, B, w.S8, w.inv, st));
  LG_HIP(lg::ak_conv3x3(conv3(L_S2, w.S8, 0, nullptr, lg::AK_SELU, w.s4a), st));
  LG_HIP(lg::ak_conv3x3(conv3(L_S4, w.s4a, 0, nullptr, lg::AK_SELU, w.s4b), st));
  {
    lg::AkConvArgs a = conv3(L_S6, w.s4b, 0, nullptr, lg::AK_SIGMOID, out->score_map);  // unpadded
    a.outH = g.H;
    a.outW = g.W;
    a.oy0 = g.pt;
    a.ox0 = g.pl;
    LG_HIP(lg::ak_conv3x3(a, st));
  }

  LG_HIP(mark(3));
  // ---- DKD (aliked.py:118-216)
  const int H = g.H, W = g.W, cap = g.cap, r = c.nms_radius;
  const size_t HW = (size_t)H * W;
  const float* scores = out->score_map;
  LG_HIP(lg::sp_nms(scores, B, H, W, r, w.mask, w.sup, w.ss, st));
  LG_HIP(lg::ak_border_mask(w.mask, B, H, W, r, in->image_size, w.mask2, st));
  std::vector<int> hc(B, 0);
  if (topk_mode(c)) {
    const int k = c.max_num_keypoints;
    LG_HIP(lg::sp_candidates(scores, w.mask2, B, H, W, 0, nullptr, 0.f, w.key, w.idx, w.blk, w.cnt, st));
    LG_HIP(lg::ak_fill_zeros(scores, w.mask2, B, H, W, k, w.key, w.idx, w.cnt, st));
    LG_HIP(lg::sp_select(w.key, w.idx, w.cnt, B, (int)HW, k, w.sel_idx, w.sel_score, cap, w.nsel, st));
  } else {
    bool use_mean = !(c.detection_threshold > 0.f);
    if (!use_mean) {
      LG_HIP(lg::sp_candidates(scores, w.mask2, B, H, W, 0, nullptr, c.detection_threshold, w.key, w.idx, w.blk, w.cnt, st));
      LG_HIP(hipMemcpyAsync(hc.data(), w.cnt, B * sizeof(int), hipMemcpyDeviceToHost, st));
      LG_HIP(hipStreamSynchronize(st));
      long long total = 0;
      for (int v : hc) total += v;
      use_mean = total == 0;  // aliked.py:141-143: nothing passes in the whole batch
    }
    if (use_mean) {
      std::vector<float> hm(B);
      LG_HIP(lg::ak_mean(scores, B, (long long)HW, w.mean, st));
      LG_HIP(hipMemcpyAsync(hm.data(), w.mean, B * sizeof(float), hipMemcpyDeviceToHost, st));
      LG_HIP(hipStreamSynchronize(st));
      const int nb = lg::sp_cand_blocks(H);
      for (int b = 0; b < B; ++b)
        LG_HIP(lg::sp_candidates(scores + b * HW, w.mask2 + b * HW, 1, H, W, 0, nullptr, hm[b], w.key + b * HW, w.idx + b * HW,
                                 w.blk + (size_t)b * nb, w.cnt + b, st));
      LG_HIP(hipMemcpyAsync(hc.data(), w.cnt, B * sizeof(int), hipMemcpyDeviceToHost, st));
      LG_HIP(hipStreamSynchronize(st));
    }
    const int nl = n_limit(c);
    const int mx = *std::max_element(hc.begin(), hc.end());
    int k = 0;
    if (mx > nl) {
      if (nl > lg::kSpSelectMax) return fail(LG_E_INVALID, "sp_aliked_forward: more than 16384 keypoints pass the threshold");
      k = nl;
    }
    if (std::min(mx, nl) > cap) return fail(LG_E_INVALID, "sp_aliked_forward: capacity below the keypoint count");
    LG_HIP(lg::sp_select(w.key, w.idx, w.cnt, B, (int)HW, k, w.sel_idx, w.sel_score, cap, w.nsel, st));
    for (int b = 0; b < B; ++b) hc[b] = std::min(hc[b], nl);
  }
  LG_HIP(lg::ak_refine(scores, w.sel_idx, w.nsel, B, cap, H, W, r, w.kn, out->keypoints, out->sampled_scores, out->dispersity,
                       st));
  LG_HIP(hipMemcpyAsync(out->counts, w.nsel, B * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (out->host_counts) {
    if (topk_mode(c))
      for (int b = 0; b < B; ++b) out->host_counts[b] = c.max_num_keypoints;
    else
      for (int b = 0; b < B; ++b) out->host_counts[b] = hc[b];
  }

  LG_HIP(mark(4));
  // ---- SDDH (aliked.py:513-588)
  lg::AkSddh s{};
  s.py = py;
  s.inv = w.inv;
  s.pt = g.pt;
  s.pl = g.pl;
  s.H = H;
  s.W = W;
  s.B = B;
  s.cap = cap;
  s.dim = c.dim;
  s.M = c.M;
  s.kn = w.kn;
  LG_HIP(lg::ak_sddh_offsets(s, G + h->w0t, G + h->b0, G + h->w1t, G + h->b1, w.offs, st));
  LG_HIP(lg::ak_sddh_sample(s, w.offs, w.F, st));
  const long long rows = (long long)B * cap * c.M;
  {  // sf_conv: [N M, dim] x [dim, dim] on the matrix cores (bf16x6: fp32-accurate products)
    lg::GemmArgs a{};
    a.A0 = w.F;
    a.lda0 = c.dim;
    a.K0 = a.K = c.dim;
    a.W = G + h->sf;
    a.ldw = c.dim;
    a.Y = w.Y1;
    a.ldy = c.dim;
    a.out_scale = 1.f;
    a.R = (int)rows;
    a.Nout = c.dim;
    LG_HIP(lg::gemm_x6(a, lg::EPI_STORE, 1, st));
  }
  LG_HIP(lg::ak_selu(w.Y1, rows * c.dim, st));
  {  // einsum("ncp,pcd->nd"): [N, M dim] x [M dim, dim]
    lg::GemmArgs a{};
    a.A0 = w.Y1;
    a.lda0 = c.M * c.dim;
    a.K0 = a.K = c.M * c.dim;
    a.W = G + h->aggT;
    a.ldw = c.M * c.dim;
    a.Y = w.D;
    a.ldy = c.dim;
    a.out_scale = 1.f;
    a.R = B * cap;
    a.Nout = c.dim;
    LG_HIP(lg::gemm_x6(a, lg::EPI_STORE, 1, st));
  }
  LG_HIP(lg::ak_l2norm(w.D, (long long)B * cap, c.dim, out->descriptors, st));
  LG_HIP(mark(5));
  h->ev_valid = h->profile;
  return LG_OK;
}

int sp_aliked_set_profile(sp_aliked_handle_t* h, int32_t on) {
  if (!h) return fail(LG_E_INVALID, "sp_aliked_set_profile: null handle");
  h->profile = on != 0;
  h->ev_valid = false;
  return LG_OK;
}

int sp_aliked_stage_ms(sp_aliked_handle_t* h, float* ms) {
  if (!h || !ms) return fail(LG_E_INVALID, "sp_aliked_stage_ms: null argument");
  if (!h->ev_valid) return fail(LG_E_INVALID, "sp_aliked_stage_ms: no profiled forward (sp_aliked_set_profile)");
  LG_HIP(hipEventSynchronize(h->ev[5]));
  for (int i = 0; i < 5; ++i) LG_HIP(hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
  return LG_OK;
}

int sp_aliked_deform_conv(const float* x, const float* offset, const float* weight, const float* bias, int32_t B, int32_t Cin,
                          int32_t Cout, int32_t H, int32_t W, float* y, float* scratch, size_t scratch_bytes, void* stream) {
  if (B == 0 || H == 0 || W == 0) return LG_OK;
  if (!x || !offset || !weight || !y || !scratch) return fail(LG_E_INVALID, "sp_aliked_deform_conv: null argument");
  if (B < 0 || H < 0 || W < 0 || Cin <= 0 || (Cout != 32 && Cout != 64 && Cout != 128))
    return fail(LG_E_INVALID, "sp_aliked_deform_conv: Cout must be 32, 64 or 128");
  const size_t need = ((size_t)9 * Cin + 1) * Cout * sizeof(float);
  if (scratch_bytes < need) return fail(LG_E_WORKSPACE, "sp_aliked_deform_conv: scratch too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* wt = scratch;
  float* bp = scratch + (size_t)9 * Cin * Cout;
  LG_HIP(lg::ak_repack(weight, Cout, Cin, 9, Cin * 9, 0, nullptr, wt, st));
  LG_HIP(lg::ak_pad_vec(bias, Cout, Cout, bp, st));
  LG_HIP(lg::ak_deform_conv(x, offset, B, Cin, Cout, H, W, wt, bp, nullptr, lg::AK_NONE, y, st));
  return LG_OK;
}

}  // extern "C"
