// C-ABI of the GlueStick matcher (include/gluestick_mi355x.h): schema, load-time folds and the eval
// forward (reference gluefactory/models/matchers/gluestick.py:136-312):
//   keypoint encoder + descriptors -> residual stream x; endpoint encoder -> line_enc (once)
//   junction -> endpoint lists (count, scan, stable fill; once: the indices do not change)
//   per GNN layer: the SuperGlue layer (sg_trunk.h: QKV GEMM, attention, mlp.0, mlp.3 + residual);
//   after every "self" layer, num_line_iterations times the line layer:
//     G = [x[j(e)] | x[j(e ^ 1)] | line_enc[e]]      gather, fp32 rows -> plane image (K = 768)
//     h = relu(BN(W1 G)), u = W2 h + b2              two fp16x3 GEMMs, BatchNorm folded into W1
//     x[j] += mean over the junction's endpoints      one wave per junction, list order; then x's
//                                                     plane image and range slot are rewritten
//   [md | mdl] = [final_proj; final_line_proj](x)     one fp16x3 GEMM, Nout = 512
//   points: md0 md1^T / 16 (bf16x6), log_double_softmax with bin_score, mutual filter
//   lines:  rows of mdl at the endpoints' junctions, one 2 L0 x 2 L1 product / 16, the better of
//           the two orientations per line pair, log_double_softmax with line_bin_score, filter
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gluestick_mi355x.h"
#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "common.h"
#include "kernels.h"
#include "sg_trunk.h"

namespace {

constexpr int D = 256;
// range slots per forward: 2 for the encoder, 4 per GNN layer, 5 per line layer application
constexpr int kSlotsMax = 8 + SG_MAX_LAYERS * (4 + 5 * SG_GLUESTICK_MAX_LINE_ITERS);

void add_mlp(lg::WeightSchema& s, const std::string& p, const std::vector<int>& ch) {
  int idx = 0;
  for (size_t i = 1; i < ch.size(); ++i) {
    s.add(p + "." + std::to_string(idx) + ".weight", (int64_t)ch[i] * ch[i - 1]);
    s.add(p + "." + std::to_string(idx) + ".bias", ch[i]);
    ++idx;
    if (i < ch.size() - 1) {
      for (const char* f : {"weight", "bias", "running_mean", "running_var"})
        s.add(p + "." + std::to_string(idx) + "." + f, ch[i]);
      idx += 2;
    }
  }
}

std::vector<int> enc_channels(const sg_gluestick_config_t& c, int cin) {
  std::vector<int> ch = {cin};
  for (int i = 0; i < c.n_kenc; ++i) ch.push_back(c.keypoint_encoder[i]);
  ch.push_back(D);
  return ch;
}

// the module's own parameters lead its state dict, then the children in registration order
lg::WeightSchema make_schema(const sg_gluestick_config_t& c) {
  lg::WeightSchema s;
  s.add("bin_score", 1);
  s.add("line_bin_score", 1);
  add_mlp(s, "kenc.encoder", enc_channels(c, 3));
  add_mlp(s, "lenc.encoder", enc_channels(c, 5));
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = "gnn.layers." + std::to_string(i) + ".update";
    s.add(p + ".attn.merge.weight", (int64_t)D * D);
    s.add(p + ".attn.merge.bias", D);
    for (int j = 0; j < 3; ++j) {
      s.add(p + ".attn.proj." + std::to_string(j) + ".weight", (int64_t)D * D);
      s.add(p + ".attn.proj." + std::to_string(j) + ".bias", D);
    }
    add_mlp(s, p + ".mlp", {2 * D, 2 * D, D});
  }
  for (int i = 0; i < c.n_layers / 2; ++i) add_mlp(s, "gnn.line_layers." + std::to_string(i) + ".mlp", {3 * D, 2 * D, D});
  s.add("final_proj.weight", (int64_t)D * D);
  s.add("final_proj.bias", D);
  s.add("final_line_proj.weight", (int64_t)D * D);
  s.add("final_line_proj.bias", D);
  return s;
}

size_t a256(size_t n) { return (n + 255) & ~size_t(255); }
int pad256(size_t n) { return (int)((n + 255) / 256 * 256); }

// what one line layer application needs beside x
struct LineWork {
  float *enc, *G, *U;
  _Float16 *Gp, *LHp;
  int *idx32, *deg, *start, *cursor, *list;
  int EP;
  size_t bytes;
};
LineWork carve_lines(char* base, size_t R, size_t E) {
  size_t o = 0;
  auto take = [&](size_t n) {
    char* p = base ? base + o : nullptr;
    o += a256(n);
    return p;
  };
  LineWork w{};
  w.EP = pad256(E);
  w.enc = (float*)take(E * D * 4);
  w.G = (float*)take(E * 3 * D * 4);
  w.U = (float*)take(E * D * 4);
  w.Gp = (_Float16*)take(2 * (size_t)w.EP * 3 * D * 2);
  w.LHp = (_Float16*)take(2 * (size_t)w.EP * 2 * D * 2);
  w.idx32 = (int*)take(E * 4);
  w.deg = (int*)take(R * 4);
  w.start = (int*)take(R * 4);
  w.cursor = (int*)take(R * 4);
  w.list = (int*)take(E * 4);
  w.bytes = o;
  return w;
}

struct Work {
  float *X, *Q, *ctx, *md, *cost, *Z, *fws, *dws;
  void *KP, *VP;
  _Float16 *Xp, *Cp, *Hp;
  unsigned* rtab;
  int rows_pad;
  LineWork lw;
  float *gl, *S, *raw, *LZ, *lfws, *ldws;  // line head
  size_t bytes;
};
Work carve(char* base, int B, int M, int N, int L0, int L1) {
  const size_t R = (size_t)B * (M + N);
  const size_t RP = (R + 255) / 256 * 256;
  const bool lines = L0 > 0 && L1 > 0;
  const size_t E = lines ? 2 * (size_t)B * (L0 + L1) : 0;
  size_t o = 0;
  auto take = [&](size_t n) {
    char* p = base ? base + o : nullptr;
    o += a256(n);
    return p;
  };
  Work w{};
  w.rows_pad = (int)RP;
  w.X = (float*)take(R * D * 4);
  w.Q = (float*)take(R * D * 4);
  w.ctx = (float*)take(R * D * 4);
  w.md = (float*)take(R * 2 * D * 4);
  w.KP = take(2 * R * D * 2);
  w.VP = take(2 * R * D * 2);
  w.Xp = (_Float16*)take(2 * RP * D * 2);
  w.Cp = (_Float16*)take(2 * RP * D * 2);
  w.Hp = (_Float16*)take(2 * RP * 2 * D * 2);
  w.cost = (float*)take((size_t)B * M * N * 4);
  w.Z = (float*)take((size_t)B * (M + 1) * (N + 1) * 4);
  w.fws = (float*)take(lg::filter_workspace_floats(B, M, N) * 4);
  w.dws = (float*)take(2 * R * 4);
  w.rtab = (unsigned*)take((size_t)kSlotsMax * lg::kRangeStride * sizeof(unsigned));
  if (lines) {
    w.lw = carve_lines(base ? base + o : nullptr, R, E);
    o += w.lw.bytes;
    w.gl = (float*)take(E * D * 4);
    w.S = (float*)take(4 * (size_t)B * L0 * L1 * 4);
    w.raw = (float*)take((size_t)B * L0 * L1 * 4);
    w.LZ = (float*)take((size_t)B * (L0 + 1) * (L1 + 1) * 4);
    w.lfws = (float*)take(lg::filter_workspace_floats(B, L0, L1) * 4);
    w.ldws = (float*)take(2 * (size_t)B * (L0 + L1) * 4);
  }
  w.bytes = o;
  return w;
}

}  // namespace

struct sg_gluestick_handle {
  sg_gluestick_config_t cfg;
  int device;
  lg::WeightSchema schema;
  std::vector<float*> raw;   // device copies of the loaded tensors (schema order)
  float* buf = nullptr;      // packed / folded fp32 weights
  int* perm = nullptr;       // sg_layer_perm
  _Float16* planes = nullptr;
  std::vector<lg::SgLayer> layers;
  struct Line {
    lg::SgMat w1, w2;        // 512 x 768 (BatchNorm folded), 256 x 512
  };
  std::vector<Line> lines;
  lg::SgMat fin;             // [final_proj; final_line_proj]: 512 x 256
  struct Enc {
    size_t wt, b;            // transposed weight [Cin][Cout], bias
    int bn;                  // schema index of the BatchNorm weight (-1: last layer)
  };
  std::vector<Enc> kenc, lenc;
  std::vector<int> kch, lch;
  float bin_score = 1.f, line_bin_score = 1.f;
  bool loaded = false;
};

namespace {

using Handle = sg_gluestick_handle;

// one encoder MLP over the rows of one image set (VALU, fp32): out = (desc +) MLP(inputs)
hipError_t run_encoder(const Handle* h, bool endpoints, const float* pts, const float* scores, const float* size, int fw,
                       int fh, int n, int rows, const float* desc, float* out, hipStream_t st) {
  const std::vector<Handle::Enc>& enc = endpoints ? h->lenc : h->kenc;
  const std::vector<int>& ch = endpoints ? h->lch : h->kch;
  lg::SgEncArgs e;
  memset(&e, 0, sizeof(e));
  e.kpts = pts;
  e.scores = scores;
  e.size = size;
  e.fw = (float)fw;
  e.fh = (float)fh;
  e.n = n;
  e.rows = rows;
  e.desc = desc;
  e.out = out;
  e.ldo = D;
  e.endpoints = endpoints ? 1 : 0;
  e.nl = (int)enc.size();
  for (int l = 0; l <= e.nl; ++l) e.ch[l] = ch[l];
  for (int l = 0; l < e.nl; ++l) {
    e.layer[l].Wt = h->buf + enc[l].wt;
    e.layer[l].b = h->buf + enc[l].b;
    if (enc[l].bn >= 0) {
      e.layer[l].bn_w = h->raw[enc[l].bn];
      e.layer[l].bn_b = h->raw[enc[l].bn + 1];
      e.layer[l].bn_mean = h->raw[enc[l].bn + 2];
      e.layer[l].bn_var = h->raw[enc[l].bn + 3];
    }
  }
  return lg::sg_keypoint_encoder(e, st);
}

// One line layer application on x [R][256] (gluestick.py:592-604, 634-684 with line_attention
// False).  Slots s[0..4] are fresh; with Xp the plane image of x is rewritten at slot s[4] and its
// maximum recorded there.
int line_layer(const Handle* h, int li, float* X, _Float16* Xp, int R, int RP, const lg::GsLayout& gl, const LineWork& lw,
               unsigned* rt, const int* s, hipStream_t st) {
  using namespace lg;
  const Handle::Line& ln = h->lines[li];
  const int E = gl.B * (gl.E0 + gl.E1), EP = lw.EP;
  auto ro = [&](int in0, float g0, float add, int o) { return RangeOut{rt, in0, -1, g0, 0.f, add, o, 1, 0}; };
  auto wplanes = [&](GemmH3Args& g, const SgMat& m) {
    g.W = {h->planes + m.poff, (long long)m.rows * m.K, m.rows};
    g.acc_scale = m.unscale;
    g.bias = h->buf + m.boff;
  };
  LG_HIP(gs_gather_endpoints(X, lw.enc, lw.idx32, gl, lw.G, st));
  LG_HIP(range_absmax(lw.G, (size_t)E * 3 * D, rt, s[0], st));
  LG_HIP(rows_to_planes(lw.G, E, 3 * D, 3 * D, lw.Gp, EP, 0, ro(s[0], 1.f, 0.f, s[1]), st));
  {
    GemmH3Args g;
    memset(&g, 0, sizeof(g));
    g.out_scale = 1.f;
    g.A0 = {lw.Gp, (long long)EP * 3 * D, EP}; g.K0 = 3 * D; g.K = 3 * D; wplanes(g, ln.w1);
    g.rtab = rt; g.a0_slot = s[1]; g.a1_slot = -1;
    g.R = E; g.Nout = 2 * D; g.relu = 1;
    g.Yp = lw.LHp; g.yps = (long long)EP * 2 * D; g.yrows_pad = EP;
    g.ro = ro(s[1], ln.w1.g, ln.w1.bmax, s[2]);
    LG_HIP(gemm_h3(g, EPI_STORE, st));
  }
  {
    GemmH3Args g;
    memset(&g, 0, sizeof(g));
    g.out_scale = 1.f;
    g.A0 = {lw.LHp, (long long)EP * 2 * D, EP}; g.K0 = 2 * D; g.K = 2 * D; wplanes(g, ln.w2);
    g.rtab = rt; g.a0_slot = s[2]; g.a1_slot = -1;
    g.R = E; g.Nout = D; g.Y = lw.U; g.ldy = D;
    LG_HIP(gemm_h3(g, EPI_STORE, st));
  }
  LG_HIP(gs_scatter_mean(X, R, lw.U, lw.deg, lw.start, lw.list, st));
  if (Xp) {  // the next QKV GEMM reads the planes at this slot's exponent
    LG_HIP(range_absmax(X, (size_t)R * D, rt, s[3], st));
    LG_HIP(rows_to_planes(X, R, D, D, Xp, RP, 0, ro(s[3], 1.f, 0.f, s[4]), st));
  }
  return LG_OK;
}


// Raw line scores (gluestick.py:335-357) from projected rows: the endpoints' junction rows of
// p0 [B][n0] / p1 [B][n1] (256 floats at row stride ld) gathered into g0 [B][E0][256] / g1
// [B][E1][256], S [B][E0][E1] = g0 g1^T / 16, raw [B][L0][L1] = the better orientation, halved.
int line_head_scores(const float* p0, const float* p1, int ld, int n0, int n1, const int64_t* idx0, const int64_t* idx1,
                     int B, int L0, int L1, float* g0, float* g1, float* S, float* raw, hipStream_t st) {
  using namespace lg;
  const int E0 = 2 * L0, E1 = 2 * L1;
  LG_HIP(gs_gather_rows256(p0, ld, n0, idx0, B, E0, g0, st));
  LG_HIP(gs_gather_rows256(p1, ld, n1, idx1, B, E1, g1, st));
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A0 = g0; g.lda0 = D; g.K0 = D; g.K = D; g.sA = (long long)E0 * D;
  g.W = g1; g.ldw = D; g.sW = (long long)E1 * D;
  g.R = E0; g.Nout = E1; g.Y = S; g.ldy = E1; g.sY = (long long)E0 * E1;
  g.out_scale = 1.f / 16.f;
  LG_HIP(gemm_x6(g, EPI_STORE, B, st));
  LG_HIP(gs_line_combine(S, B, L0, L1, raw, st));
  return LG_OK;
}

}  // namespace

extern "C" {

int sg_gluestick_create(const sg_gluestick_config_t* cfg, int device, sg_gluestick_handle_t** out) {
  if (!cfg || !out) return fail(LG_E_INVALID, "null argument");
  if (cfg->descriptor_dim != D) return fail(LG_E_INVALID, "descriptor_dim must be 256 (kernels are specialised)");
  if (cfg->n_layers < 0 || cfg->n_layers > SG_MAX_LAYERS) return fail(LG_E_INVALID, "n_layers out of range");
  if (cfg->n_kenc < 0 || cfg->n_kenc > SG_MAX_KENC) return fail(LG_E_INVALID, "keypoint_encoder too long");
  for (int i = 0; i < cfg->n_kenc; ++i)
    if (cfg->keypoint_encoder[i] <= 0 || cfg->keypoint_encoder[i] > 256 || cfg->keypoint_encoder[i] % 4)
      return fail(LG_E_INVALID, "keypoint_encoder widths must be multiples of 4 in [4, 256]");
  for (int i = 0; i < cfg->n_layers; ++i)
    if (cfg->layer_types[i] != 0 && cfg->layer_types[i] != 1) return fail(LG_E_INVALID, "GNN layer must be self or cross");
  if (cfg->num_line_iterations < 0 || cfg->num_line_iterations > SG_GLUESTICK_MAX_LINE_ITERS)
    return fail(LG_E_INVALID, "num_line_iterations out of range");
  // no device call here: the schema and the workspace size are host arithmetic, and a host
  // without a GPU can ask for them; load_weights and forward select the device
  sg_gluestick_handle* h = new sg_gluestick_handle();
  h->cfg = *cfg;
  h->device = device;
  h->schema = make_schema(*cfg);
  h->kch = enc_channels(*cfg, 3);
  h->lch = enc_channels(*cfg, 5);
  *out = h;
  return LG_OK;
}

int sg_gluestick_destroy(sg_gluestick_handle_t* h) {
  if (!h) return LG_OK;
  if (!h->raw.empty() || h->buf || h->perm || h->planes) (void)hipSetDevice(h->device);
  for (float* p : h->raw) (void)hipFree(p);
  if (h->buf) (void)hipFree(h->buf);
  if (h->perm) (void)hipFree(h->perm);
  if (h->planes) (void)hipFree(h->planes);
  delete h;
  return LG_OK;
}

int sg_gluestick_weight_count(const sg_gluestick_handle_t* h) { return h ? lg::weight_count(h->schema) : 0; }
const char* sg_gluestick_weight_name(const sg_gluestick_handle_t* h, int i) {
  return h ? lg::weight_name(h->schema, i) : nullptr;
}
int64_t sg_gluestick_weight_numel(const sg_gluestick_handle_t* h, int i) { return h ? lg::weight_numel(h->schema, i) : -1; }

int sg_gluestick_load_weights(sg_gluestick_handle_t* h, int n, const char* const* names, const float* const* tensors,
                              const int64_t* numels, void* stream) {
  if (!h || n < 0 || (n && (!names || !tensors || !numels))) return fail(LG_E_INVALID, "null argument");
  LG_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  std::vector<int> src;
  std::string err;
  if (!h->schema.match(n, names, tensors, numels, src, err)) return fail(LG_E_WEIGHTS, err);
  h->loaded = false;
  for (float* p : h->raw) (void)hipFree(p);
  h->raw.assign(h->schema.size(), nullptr);
  for (int k = 0; k < h->schema.size(); ++k) {
    LG_HIP(hipMalloc((void**)&h->raw[k], h->schema.numel(k) * sizeof(float)));
    LG_HIP(hipMemcpyAsync(h->raw[k], tensors[src[k]], h->schema.numel(k) * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  auto raw = [&](const std::string& name) { return h->raw[h->schema.find(name)]; };

  const int L = h->cfg.n_layers, NL = L / 2;
  size_t off = 0;
  auto take = [&](size_t nf) {
    const size_t o = off;
    off += (nf + 63) & ~size_t(63);
    return o;
  };
  auto enc_layout = [&](std::vector<Handle::Enc>& enc, const std::vector<int>& ch, const std::string& p) {
    enc.clear();
    for (size_t l = 0; l + 1 < ch.size(); ++l) {
      Handle::Enc e;
      e.wt = take((size_t)ch[l] * ch[l + 1]);
      e.b = take(ch[l + 1]);
      e.bn = l + 2 < ch.size() ? h->schema.find(p + "." + std::to_string(3 * l + 1) + ".weight") : -1;
      enc.push_back(e);
    }
  };
  enc_layout(h->kenc, h->kch, "kenc.encoder");
  enc_layout(h->lenc, h->lch, "lenc.encoder");
  h->layers.assign(L, {});
  for (int i = 0; i < L; ++i) lg::sg_layer_layout(h->layers[i], h->cfg.layer_types[i], take);
  h->lines.assign(NL, {});
  for (int i = 0; i < NL; ++i) {
    h->lines[i].w1 = {take(2 * D * 3 * D), take(2 * D), 2 * D, 3 * D, 0, 0.f, 0.f, 0.f};
    h->lines[i].w2 = {take(D * 2 * D), take(D), D, 2 * D, 0, 0.f, 0.f, 0.f};
  }
  h->fin = {take(2 * D * D), take(2 * D), 2 * D, D, 0, 0.f, 0.f, 0.f};
  if (h->buf) (void)hipFree(h->buf);
  h->buf = nullptr;
  LG_HIP(hipMalloc((void**)&h->buf, off * sizeof(float)));
  if (!h->perm) {
    LG_HIP(hipMalloc((void**)&h->perm, 4 * D * sizeof(int)));
    const std::vector<int> p = lg::sg_layer_perm();
    LG_HIP(hipMemcpy(h->perm, p.data(), p.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  float* tmp = nullptr;
  LG_HIP(hipMallocAsync((void**)&tmp, lg::kSgTmpFloats * sizeof(float), st));
  float* B = h->buf;
  auto copy = [&](size_t dst, const std::string& name, size_t nf) {
    return hipMemcpyAsync(B + dst, raw(name), nf * sizeof(float), hipMemcpyDeviceToDevice, st);
  };
  auto enc_pack = [&](const std::vector<Handle::Enc>& enc, const std::vector<int>& ch, const std::string& p) -> int {
    for (size_t l = 0; l < enc.size(); ++l) {
      const std::string q = p + "." + std::to_string(3 * l);
      LG_HIP(lg::sg_transpose(raw(q + ".weight"), ch[l + 1], ch[l], B + enc[l].wt, st));
      LG_HIP(copy(enc[l].b, q + ".bias", ch[l + 1]));
    }
    return LG_OK;
  };
  if (int rc = enc_pack(h->kenc, h->kch, "kenc.encoder")) return rc;
  if (int rc = enc_pack(h->lenc, h->lch, "lenc.encoder")) return rc;
  for (int i = 0; i < L; ++i)
    LG_HIP(lg::sg_pack_layer(raw, "gnn.layers." + std::to_string(i) + ".update", h->layers[i], B, tmp, h->perm, st));
  for (int i = 0; i < NL; ++i) {
    const std::string p = "gnn.line_layers." + std::to_string(i) + ".mlp";
    Handle::Line& ln = h->lines[i];
    LG_HIP(copy(ln.w1.off, p + ".0.weight", 2 * D * 3 * D));
    LG_HIP(copy(ln.w1.boff, p + ".0.bias", 2 * D));
    LG_HIP(lg::sg_bn_fold(B + ln.w1.off, B + ln.w1.boff, raw(p + ".1.weight"), raw(p + ".1.bias"),
                          raw(p + ".1.running_mean"), raw(p + ".1.running_var"), 2 * D, 3 * D, st));
    LG_HIP(copy(ln.w2.off, p + ".3.weight", D * 2 * D));
    LG_HIP(copy(ln.w2.boff, p + ".3.bias", D));
  }
  LG_HIP(copy(h->fin.off, "final_proj.weight", D * D));
  LG_HIP(copy(h->fin.off + D * D, "final_line_proj.weight", D * D));
  LG_HIP(copy(h->fin.boff, "final_proj.bias", D));
  LG_HIP(copy(h->fin.boff + D, "final_line_proj.bias", D));
  LG_HIP(hipFreeAsync(tmp, st));

  std::vector<lg::SgMat*> mats;
  for (auto& ly : h->layers) {
    mats.push_back(&ly.qkv);
    mats.push_back(&ly.w1);
    mats.push_back(&ly.w2);
  }
  for (auto& ln : h->lines) {
    mats.push_back(&ln.w1);
    mats.push_back(&ln.w2);
  }
  mats.push_back(&h->fin);
  std::vector<float> scal;
  LG_HIP(lg::sg_finish_mats(B, mats, h->layers, {raw("bin_score"), raw("line_bin_score")}, scal, &h->planes, st));
  h->bin_score = scal[0];
  h->line_bin_score = scal[1];
  LG_HIP(hipStreamSynchronize(st));
  h->loaded = true;
  return LG_OK;
}

int sg_gluestick_workspace_bytes(const sg_gluestick_handle_t* h, int32_t B, int32_t M, int32_t N, int32_t L0, int32_t L1,
                                 size_t* bytes) {
  if (!h || !bytes || B < 0 || M < 0 || N < 0 || L0 < 0 || L1 < 0) return fail(LG_E_INVALID, "bad argument");
  *bytes = carve(nullptr, B, M, N, L0, L1).bytes;
  return LG_OK;
}

int sg_gluestick_forward(sg_gluestick_handle_t* h, const sg_gluestick_inputs_t* in, sg_gluestick_outputs_t* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
  using namespace lg;
  if (!h || !in || !out) return fail(LG_E_INVALID, "null argument");
  if (!h->loaded) return fail(LG_E_WEIGHTS, "weights not loaded");
  const int B = in->B, M = in->M, N = in->N, L0 = in->L0, L1 = in->L1;
  if (B <= 0 || M <= 0 || N <= 0) return fail(LG_E_INVALID, "B, M and N must be >= 1 (empty views: gluestick.py:156)");
  if (L0 < 0 || L1 < 0) return fail(LG_E_INVALID, "negative line count");
  if (!in->keypoints0 || !in->keypoints1 || !in->descriptors0 || !in->descriptors1 || !in->scores0 || !in->scores1)
    return fail(LG_E_INVALID, "missing input tensor");
  if ((!in->image_size0 && (in->image_w0 <= 0 || in->image_h0 <= 0)) || (!in->image_size1 && (in->image_w1 <= 0 || in->image_h1 <= 0)))
    return fail(LG_E_INVALID, "image_size or the image shape is required (gluestick.py:139-148)");
  if (!out->matches0 || !out->matches1 || !out->matching_scores0 || !out->matching_scores1)
    return fail(LG_E_INVALID, "missing output tensor");
  const bool lines = L0 > 0 && L1 > 0;  // the reference skips the line layers when either image has none (:723-727)
  if (lines) {
    if (!in->lines0 || !in->lines1 || !in->lines_junc_idx0 || !in->lines_junc_idx1 || !in->line_scores0 || !in->line_scores1)
      return fail(LG_E_INVALID, "missing line input tensor");
    if (!out->line_log_assignment || !out->line_matches0 || !out->line_matches1 || !out->line_matching_scores0 ||
        !out->line_matching_scores1 || !out->raw_line_scores)
      return fail(LG_E_INVALID, "missing line output tensor");
    for (int i = 0; i < h->cfg.n_layers; ++i)
      if (h->cfg.layer_types[i] == 0 && h->cfg.num_line_iterations > 0 && i / 2 >= (int)h->lines.size())
        return fail(LG_E_INVALID, "self layer " + std::to_string(i) + " has no line layer (gnn.line_layers holds len(GNN_layers) // 2)");
  }
  const Work need = carve(nullptr, B, M, N, L0, L1);
  if (!workspace || workspace_bytes < need.bytes) return fail(LG_E_WORKSPACE, "workspace too small: need " + std::to_string(need.bytes));
  LG_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  Work w = carve((char*)workspace, B, M, N, L0, L1);
  const int R = B * (M + N), RP = w.rows_pad;
  const int E0 = 2 * L0, E1 = 2 * L1;
  const float* W = h->buf;
  unsigned* rt = w.rtab;
  int nslot = 0;
  auto slot = [&]() { return nslot < kSlotsMax ? nslot++ : kSlotsMax - 1; };
  const int slots_used = std::min(kSlotsMax, 2 + h->cfg.n_layers * (4 + 5 * h->cfg.num_line_iterations));
  LG_HIP(hipMemsetAsync(rt, 0, (size_t)slots_used * kRangeStride * sizeof(unsigned), st));

  // ---- keypoint encoder + descriptors -> x (gluestick.py:200-204), then its plane image
  LG_HIP(run_encoder(h, false, in->keypoints0, in->scores0, in->image_size0, in->image_w0, in->image_h0, M, B * M,
                     in->descriptors0, w.X, st));
  LG_HIP(run_encoder(h, false, in->keypoints1, in->scores1, in->image_size1, in->image_w1, in->image_h1, N, B * N,
                     in->descriptors1, w.X + (size_t)B * M * D, st));
  const int s_in = slot();
  int s_x = slot();
  LG_HIP(range_absmax(w.X, (size_t)R * D, rt, s_in, st));
  LG_HIP(rows_to_planes(w.X, R, D, D, w.Xp, RP, 0, RangeOut{rt, s_in, -1, 1.f, 0.f, 0.f, s_x, 1, 0}, st));

  // ---- endpoint encoder (:206-215) and the junction -> endpoint lists, once per forward
  const GsLayout gl{B, M, N, E0, E1};
  if (lines) {
    LG_HIP(run_encoder(h, true, in->lines0, in->line_scores0, in->image_size0, in->image_w0, in->image_h0, E0, B * E0,
                       nullptr, w.lw.enc, st));
    LG_HIP(run_encoder(h, true, in->lines1, in->line_scores1, in->image_size1, in->image_w1, in->image_h1, E1, B * E1,
                       nullptr, w.lw.enc + (size_t)B * E0 * D, st));
    LG_HIP(gs_clamp_idx(in->lines_junc_idx0, (size_t)B * E0, M, w.lw.idx32, st));
    LG_HIP(gs_clamp_idx(in->lines_junc_idx1, (size_t)B * E1, N, w.lw.idx32 + (size_t)B * E0, st));
    LG_HIP(gs_build_csr(w.lw.idx32, gl, w.lw.deg, w.lw.start, w.lw.cursor, w.lw.list, st));
  }

  // ---- AttentionalGNN (:713-758)
  const SgTrunkWork tw{w.X, w.Q, w.ctx, w.KP, w.VP, w.Xp, w.Cp, w.Hp, rt, RP};
  const RowMask live{};
  for (int i = 0; i < h->cfg.n_layers; ++i) {
    const int s_k = slot(), s_v = slot(), s_h = slot(), s_xn = slot();
    LG_HIP(sg_gnn_layer(h->layers[i], W, h->planes, tw, B, M, N, live, nullptr, nullptr, s_x, s_k, s_v, s_h, s_xn, st));
    s_x = s_xn;
    if (h->cfg.layer_types[i] == 0 && lines) {
      for (int it = 0; it < h->cfg.num_line_iterations; ++it) {
        int s[5];
        for (int& v : s) v = slot();
        if (int rc = line_layer(h, i / 2, w.X, w.Xp, R, RP, gl, w.lw, rt, s, st)) return rc;
        s_x = s[4];
      }
    }
  }
  if (out->descriptors0)
    LG_HIP(hipMemcpyAsync(out->descriptors0, w.X, sizeof(float) * B * M * D, hipMemcpyDeviceToDevice, st));
  if (out->descriptors1)
    LG_HIP(hipMemcpyAsync(out->descriptors1, w.X + (size_t)B * M * D, sizeof(float) * B * N * D, hipMemcpyDeviceToDevice, st));

  // ---- [final_proj; final_line_proj] in one GEMM: md rows [R][512] = [md | mdl]
  {
    GemmH3Args g;
    memset(&g, 0, sizeof(g));
    g.out_scale = 1.f;
    g.A0 = {w.Xp, (long long)RP * D, RP}; g.K0 = D; g.K = D;
    g.W = {h->planes + h->fin.poff, (long long)h->fin.rows * h->fin.K, h->fin.rows};
    g.acc_scale = h->fin.unscale;
    g.bias = W + h->fin.boff;
    g.rtab = rt; g.a0_slot = s_x; g.a1_slot = -1;
    g.R = R; g.Nout = 2 * D; g.Y = w.md; g.ldy = 2 * D;
    LG_HIP(gemm_h3(g, EPI_STORE, st));
  }
  // ---- points: scores = md0 . md1 / sqrt(256), log_double_softmax, mutual filter (:237-247)
  {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A0 = w.md; g.lda0 = 2 * D; g.K0 = D; g.K = D; g.sA = (long long)M * 2 * D;
    g.W = w.md + (size_t)B * M * 2 * D; g.ldw = 2 * D; g.sW = (long long)N * 2 * D;
    g.R = M; g.Nout = N; g.Y = w.cost; g.ldy = N; g.sY = (long long)M * N;
    g.out_scale = 1.f / 16.f;
    LG_HIP(gemm_x6(g, EPI_STORE, B, st));
  }
  float* Z = out->log_assignment ? out->log_assignment : w.Z;
  LG_HIP(gs_double_softmax(w.cost, h->bin_score, B, M, N, Z, w.dws, st));
  LG_HIP(filter_from_scores(Z, B, M, N, h->cfg.filter_threshold, w.fws, out->matches0, out->matches1,
                            out->matching_scores0, out->matching_scores1, st));
  if (!lines) return LG_OK;

  // ---- lines (:329-369): the endpoints' rows of mdl, one 2 L0 x 2 L1 product, the better orientation
  if (int rc = line_head_scores(w.md + D, w.md + (size_t)B * M * 2 * D + D, 2 * D, M, N, in->lines_junc_idx0,
                                in->lines_junc_idx1, B, L0, L1, w.gl, w.gl + (size_t)B * E0 * D, w.S, out->raw_line_scores, st))
    return rc;
  LG_HIP(gs_double_softmax(out->raw_line_scores, h->line_bin_score, B, L0, L1, out->line_log_assignment, w.ldws, st));
  LG_HIP(filter_from_scores(out->line_log_assignment, B, L0, L1, h->cfg.filter_threshold, w.lfws, out->line_matches0,
                            out->line_matches1, out->line_matching_scores0, out->line_matching_scores1, st));
  return LG_OK;
}

int sg_gluestick_line_update(sg_gluestick_handle_t* h, int32_t layer, const float* X, const float* line_enc,
                             const int64_t* idx, int32_t B, int32_t n, int32_t L, float* out, void* stream) {
  using namespace lg;
  if (!h || !X || !line_enc || !idx || !out) return fail(LG_E_INVALID, "null argument");
  if (!h->loaded) return fail(LG_E_WEIGHTS, "weights not loaded");
  if (layer < 0 || layer >= (int)h->lines.size()) return fail(LG_E_INVALID, "no such line layer");
  if (B <= 0 || n <= 0 || L <= 0) return fail(LG_E_INVALID, "B, n and L must be >= 1");
  LG_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t R = (size_t)B * n, E = 2 * (size_t)B * L;
  const LineWork need = carve_lines(nullptr, R, E);
  const size_t rt_bytes = a256(8 * kRangeStride * sizeof(unsigned));
  char* ws = nullptr;
  LG_HIP(hipMallocAsync((void**)&ws, need.bytes + rt_bytes, st));
  LineWork lw = carve_lines(ws + rt_bytes, R, E);
  unsigned* rt = (unsigned*)ws;
  const GsLayout gl{B, n, 0, 2 * L, 0};
  const int s[5] = {0, 1, 2, 3, 4};
  int rc = LG_OK;
  auto run = [&]() -> int {
    LG_HIP(hipMemsetAsync(rt, 0, 8 * kRangeStride * sizeof(unsigned), st));
    LG_HIP(hipMemcpyAsync(out, X, R * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    LG_HIP(hipMemcpyAsync(lw.enc, line_enc, E * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    LG_HIP(gs_clamp_idx(idx, E, n, lw.idx32, st));
    LG_HIP(gs_build_csr(lw.idx32, gl, lw.deg, lw.start, lw.cursor, lw.list, st));
    return line_layer(h, layer, out, nullptr, (int)R, 0, gl, lw, rt, s, st);
  };
  rc = run();
  const hipError_t f = hipFreeAsync(ws, st);
  if (rc == LG_OK && f != hipSuccess) return fail(LG_E_HIP, hipGetErrorString(f));
  return rc;
}

int sg_gluestick_double_softmax(const float* scores, float bin, int32_t B, int32_t M, int32_t N, float* out, void* stream) {
  if (!scores || !out || B <= 0 || M <= 0 || N <= 0) return fail(LG_E_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  float* ws = nullptr;
  LG_HIP(hipMallocAsync((void**)&ws, 2 * (size_t)B * (M + N) * sizeof(float), st));
  const hipError_t e = lg::gs_double_softmax(scores, bin, B, M, N, out, ws, st);
  const hipError_t f = hipFreeAsync(ws, st);
  LG_HIP(e);
  LG_HIP(f);
  return LG_OK;
}

int sg_gluestick_line_scores(const float* md0, const float* md1, const int64_t* idx0, const int64_t* idx1, int32_t B,
                             int32_t n0, int32_t n1, int32_t L0, int32_t L1, float* out, void* stream) {
  using namespace lg;
  if (!md0 || !md1 || !idx0 || !idx1 || !out || B <= 0 || n0 <= 0 || n1 <= 0 || L0 <= 0 || L1 <= 0)
    return fail(LG_E_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int E0 = 2 * L0, E1 = 2 * L1;
  const size_t g0f = a256((size_t)B * E0 * D * 4) / 4, g1f = a256((size_t)B * E1 * D * 4) / 4;
  float* ws = nullptr;
  LG_HIP(hipMallocAsync((void**)&ws, (g0f + g1f + (size_t)B * E0 * E1) * sizeof(float), st));
  float *g0 = ws, *g1 = ws + g0f, *S = ws + g0f + g1f;
  const int rc = line_head_scores(md0, md1, D, n0, n1, idx0, idx1, B, L0, L1, g0, g1, S, out, st);
  const hipError_t f = hipFreeAsync(ws, st);
  if (rc == LG_OK && f != hipSuccess) return fail(LG_E_HIP, hipGetErrorString(f));
  return rc;
}

}  // extern "C"
