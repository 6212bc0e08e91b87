// C-ABI of the LightGlue training path (include/lightglue_mi355x.h, "Training"): the
// activation-saving training forward, its backward, and the assignment-head backward -- what
// torch autograd computes in the reference (gluefactory/train.py:436-450 over
// gluefactory/models/matchers/lightglue.py:444-579 and :614-663).  Kernels: train.hip.
//
// Row space: R = B (M + N) rows of 256 -- image-0 rows (pair-major, R0 = B M of them) then image-1
// rows -- as in the eval forward.  Every activation is row-major fp32; head h of a projection is
// columns [64h, 64h + 64).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"
#include "train.h"

namespace lg {
const lg_config_t* handle_config(const lg_handle* h);
int handle_device(const lg_handle* h);
void handle_grad_ready(const lg_handle* h, int layer, void* stream);  // lg_set_grad_ready_hook
const WeightSchema& handle_schema(const lg_handle* h);
}  // namespace lg

namespace {

using namespace lg;

constexpr int D = 256;

struct Dims {
  int B, M, N, R, R0, din, L, H, m_in;
  bool proj;
};

Dims dims_of(const lg_handle_t* h, int B, int M, int N) {
  const lg_config_t& c = *handle_config(h);
  Dims d;
  d.B = B;
  d.M = M;
  d.N = N;
  d.R0 = B * M;
  d.R = B * (M + N);
  d.din = c.input_dim;
  d.L = c.n_layers;
  d.H = c.num_heads;
  d.m_in = c.add_scale_ori ? 4 : 2;
  d.proj = c.input_dim != c.descriptor_dim;
  return d;
}

struct Carver {
  char* base;
  size_t off = 0;
  float* f(size_t n) {
    char* p = base ? base + off : nullptr;
    off += (n * sizeof(float) + 255) & ~size_t(255);
    return reinterpret_cast<float*>(p);
  }
};

struct Blk {
  float *Q, *K, *V, *LSE, *O, *CAT, *H1, *ST, *G, *Y;
};
struct Saved {
  float *X0, *Din, *PEX, *COS, *SIN, *SZ, *QKV;
  std::vector<Blk> self, cross;
  size_t bytes;
};

// `ckpt` (LG_FWD_CHECKPOINTED, the reference's `checkpointed`, lightglue.py:515-518): one set of
// block activations shared by every layer (the backward recomputes layer l's into it before
// differentiating it) and only each layer's output kept per layer -- the next layer's input.
Saved carve_saved(char* base, const Dims& d, bool ckpt) {
  Carver c{base};
  Saved s;
  const size_t R = d.R;
  s.X0 = c.f(R * D);
  s.Din = d.proj ? c.f(R * d.din) : nullptr;
  s.PEX = c.f(R * 4);
  s.COS = c.f(R * 32);
  s.SIN = c.f(R * 32);
  s.SZ = c.f(4 * (size_t)d.B);
  s.QKV = c.f(R * 3 * D);  // forward temporary
  const size_t nl = (size_t)d.B * d.H * (d.M + d.N);
  for (int l = 0; l < d.L; ++l) {
    if (ckpt && l > 0) {  // layer 0's buffers serve every layer; the output is per layer
      s.self.push_back(s.self[0]);
      s.cross.push_back(s.cross[0]);
      s.cross[l].Y = c.f(R * D);
      continue;
    }
    Blk b{};
    b.Q = c.f(R * D);
    b.K = c.f(R * D);
    b.V = c.f(R * D);
    b.LSE = c.f(nl);
    b.O = c.f(R * D);
    b.CAT = c.f(R * 2 * D);
    b.H1 = c.f(R * 2 * D);
    b.ST = c.f(R * 2);
    b.G = c.f(R * 2 * D);
    b.Y = c.f(R * D);
    s.self.push_back(b);
    Blk x{};
    x.Q = c.f(R * D);  // qk
    x.V = c.f(R * D);
    x.LSE = c.f(nl);
    x.O = c.f(R * D);
    x.CAT = c.f(R * 2 * D);
    x.H1 = c.f(R * 2 * D);
    x.ST = c.f(R * 2);
    x.G = c.f(R * 2 * D);
    x.Y = c.f(R * D);  // the layer's output
    s.cross.push_back(x);
  }
  s.bytes = c.off;
  return s;
}

struct Scratch {
  float *GX, *GY, *GG, *GH, *GC, *GO, *GQ, *GK, *GV, *GQKV, *DELTA, *GCOS, *GSIN, *WS, *PART;
  size_t ws_floats, part_floats, bytes;
};

size_t gemm_ws_need(const Dims& d) {
  size_t w = 0;
  auto upd = [&](int M, int N, int K) { w = std::max(w, tgemm_ws_floats(M, N, K, 1)); };
  upd(3 * D, D, d.R);
  upd(D, D, d.R);
  upd(2 * D, 2 * D, d.R);
  upd(D, 2 * D, d.R);
  if (d.proj) upd(D, d.din, d.R);
  // room for a transposed weight (the bf16x6 route of the input-gradient products) at every
  // size, so small problems take the same routes as the full-size step
  w = std::max(w, (size_t)4 * D * D + 4);
  if (d.proj) w = std::max(w, (size_t)D * d.din + 4);
  return w;
}

size_t part_need(const Dims& d) {
  size_t p = colsum_part_floats(d.R, 3 * D);
  p = std::max(p, lngelu_bwd_part_floats(d.R));
  p = std::max(p, pe_bwd_part_floats(d.R));
  return p;
}

Scratch carve_scratch(char* base, const Dims& d) {
  Carver c{base};
  Scratch s;
  const size_t R = d.R;
  s.GX = c.f(R * D);
  s.GY = c.f(R * D);
  s.GG = c.f(R * 2 * D);
  s.GH = c.f(R * 2 * D);
  s.GC = c.f(R * 2 * D);
  s.GO = c.f(R * D);
  s.GQ = c.f(R * D);
  s.GK = c.f(R * D);
  s.GV = c.f(R * D);
  s.GQKV = c.f(R * 3 * D);
  s.DELTA = c.f((size_t)d.B * d.H * (d.M + d.N));
  s.GCOS = c.f(R * 32);
  s.GSIN = c.f(R * 32);
  s.ws_floats = gemm_ws_need(d);
  s.WS = c.f(s.ws_floats + 64);
  s.part_floats = part_need(d);
  s.PART = c.f(s.part_floats + 64);
  s.bytes = c.off;
  return s;
}

// Parameter lookup by reference name.
struct Params {
  const lg_handle_t* h;
  const float* const* p;
  float* const* g;
  const float* w(const std::string& n) const { return p[handle_schema(h).find(n)]; }
  float* gr(const std::string& n) const { return g ? g[handle_schema(h).find(n)] : nullptr; }
};

struct Ctx {
  hipStream_t st;
  float* ws;
  size_t ws_floats;
  float* part;
};

// y[M,N] = alpha (x[M,K] W[N,K]^T + b) + beta y
hipError_t linear(const Ctx& c, const float* x, long long ldx, int rows, int K, const float* W, const float* b, int N,
                  float* y, long long ldy, float beta = 0.f, float alpha = 1.f) {
  TGemm g{x, W, y, ldx, K, ldy, 0, 0, 0, rows, N, K, 1, alpha, beta, b};
  return tgemm(g, false, true, c.ws, c.ws_floats, c.st);
}
// y[M,N] = res[M,N] + x[M,K] W[N,K]^T + b (the residual read in the epilogue, not copied into y first)
hipError_t linear_res(const Ctx& c, const float* x, long long ldx, int rows, int K, const float* W, const float* b, int N,
                      float* y, long long ldy, const float* res, long long ldres) {
  TGemm g{x, W, y, ldx, K, ldy, 0, 0, 0, rows, N, K, 1, 1.f, 1.f, b};
  g.R = res;
  g.ldr = ldres;
  return tgemm(g, false, true, c.ws, c.ws_floats, c.st);
}
// dx[M,K] (+)= dy[M,N] W[N,K]
hipError_t linear_dgrad(const Ctx& c, const float* dy, long long lddy, int rows, int N, const float* W, int K, float* dx,
                        long long lddx, float beta = 0.f) {
  TGemm g{dy, W, dx, lddy, K, lddx, 0, 0, 0, rows, K, N, 1, 1.f, beta, nullptr};
  return tgemm(g, false, false, c.ws, c.ws_floats, c.st);
}
// dW[N,K] = dy[rows,N]^T x[rows,K]; db[N] = colsum(dy)
hipError_t linear_wgrad(const Ctx& c, const float* dy, long long lddy, const float* x, long long ldx, int rows, int N,
                        int K, float* dW, float* db) {
  if (dW) {
    TGemm g{dy, x, dW, lddy, ldx, K, 0, 0, 0, N, K, rows, 1, 1.f, 0.f, nullptr};
    g.colsumA = db;  // the bias gradient from the weight gradient's own read of dy
    return tgemm(g, true, false, c.ws, c.ws_floats, c.st);
  }
  if (db) return colsum(dy, lddy, rows, N, nullptr, c.part, db, c.st);
  return hipSuccess;
}

TAttn attn_args(const float* Q, const float* K, const float* V, float* O, float* lse, int B, int H, int Nq, int Nk,
                float scale) {
  TAttn a{};
  a.Q = Q;
  a.K = K;
  a.V = V;
  a.O = O;
  a.lse = lse;
  a.ldq = a.ldk = a.ldv = a.ldo = D;
  a.B = B;
  a.H = H;
  a.Nq = Nq;
  a.Nk = Nk;
  a.scale = scale;
  return a;
}

// FFN + residual of a block (lightglue.py:171-176,191,246-248): CAT[:, 256:] holds the message.
// ffn.0's input [X | message] is read from its two halves (X where it lies, the message in
// CAT[:, 256:]) by the bf16x6 products of the forward and of the weight gradient, so X is never
// copied into CAT[:, :256]
hipError_t ffn_forward(const Ctx& c, const Params& P, const std::string& pre, const float* X, Blk& b, int R) {
  hipError_t e;
  TGemm g{X, P.w(pre + ".ffn.0.weight"), b.H1, D, 2 * D, 2 * D, 0, 0, 0, R, 2 * D, 2 * D, 1, 1.f, 0.f,
          P.w(pre + ".ffn.0.bias")};
  g.A1 = b.CAT + D;
  g.lda1 = 2 * D;
  g.K0 = D;
  if ((e = tgemm(g, false, true, c.ws, c.ws_floats, c.st)) != hipSuccess) return e;
  if ((e = lngelu_fwd(b.H1, P.w(pre + ".ffn.1.weight"), P.w(pre + ".ffn.1.bias"), R, b.G, b.ST, c.st)) != hipSuccess) return e;
  return linear_res(c, b.G, 2 * D, R, 2 * D, P.w(pre + ".ffn.3.weight"), P.w(pre + ".ffn.3.bias"), D, b.Y, D, X, D);
}

// FFN backward: Gout = d/d(block output); writes gX = Gout + d/d(x through the ffn input) and
// leaves d/d(message) in GC[:, 256:]; X = the block input (ffn.0's first input half)
hipError_t ffn_backward(const Ctx& c, const Params& P, const std::string& pre, const Blk& b, const float* X,
                        const float* Gout, float* gX, Scratch& s, int R) {
  hipError_t e;
  if ((e = linear_wgrad(c, Gout, D, b.G, 2 * D, R, D, 2 * D, P.gr(pre + ".ffn.3.weight"), P.gr(pre + ".ffn.3.bias"))) !=
      hipSuccess)
    return e;
  if ((e = linear_dgrad(c, Gout, D, R, D, P.w(pre + ".ffn.3.weight"), 2 * D, s.GG, 2 * D)) != hipSuccess) return e;
  if ((e = lngelu_bwd(s.GG, b.H1, b.ST, P.w(pre + ".ffn.1.weight"), P.w(pre + ".ffn.1.bias"), R, s.GH, s.PART,
                      P.gr(pre + ".ffn.1.weight"), P.gr(pre + ".ffn.1.bias"), c.st)) != hipSuccess)
    return e;
  float* dW = P.gr(pre + ".ffn.0.weight");
  float* db = P.gr(pre + ".ffn.0.bias");
  if (dW) {  // dW = GH^T [X | message]: columns < 256 from X, the rest from CAT[:, 256:]
    TGemm g{s.GH, X, dW, 2 * D, D, 2 * D, 0, 0, 0, 2 * D, 2 * D, R, 1, 1.f, 0.f, nullptr};
    g.B1 = b.CAT + D;
    g.ldb1 = 2 * D;
    g.N0 = D;
    g.colsumA = db;
    if ((e = tgemm(g, true, false, c.ws, c.ws_floats, c.st)) != hipSuccess) return e;
  } else if (db && (e = colsum(s.GH, 2 * D, R, 2 * D, nullptr, c.part, db, c.st)) != hipSuccess) {
    return e;
  }
  if ((e = linear_dgrad(c, s.GH, 2 * D, R, 2 * D, P.w(pre + ".ffn.0.weight"), 2 * D, s.GC, 2 * D)) != hipSuccess) return e;
  return add_rows256(Gout, D, s.GC, 2 * D, gX, D, R, c.st);
}

// TransformerLayer l (lightglue.py:252-272): SelfBlock then CrossBlock, activations into s.self[l] /
// s.cross[l], the output into s.cross[l].Y
hipError_t layer_forward(const Ctx& c, const Params& P, Saved& s, const Dims& d, int l) {
  const int B = d.B, M = d.M, N = d.N, R = d.R, R0 = d.R0, H = d.H;
  const float scale = 0.125f;  // head_dim ** -0.5 (:146-149; cross: (s^0.5)^2, :235-236)
  const size_t lse1 = (size_t)B * H * M;
  const std::string sp = "transformers." + std::to_string(l) + ".self_attn";
  const std::string cp = "transformers." + std::to_string(l) + ".cross_attn";
  const float* X = l == 0 ? s.X0 : s.cross[l - 1].Y;
  hipError_t e;
  // SelfBlock (:178-191) on both images (shared weights, :270-271)
  Blk& sb = s.self[l];
  if ((e = linear(c, X, D, R, D, P.w(sp + ".Wqkv.weight"), P.w(sp + ".Wqkv.bias"), 3 * D, s.QKV, 3 * D)) != hipSuccess)
    return e;
  if ((e = rotary_split(s.QKV, s.COS, s.SIN, R, H, sb.Q, sb.K, sb.V, c.st)) != hipSuccess) return e;
  if ((e = tattn_forward(attn_args(sb.Q, sb.K, sb.V, sb.O, sb.LSE, B, H, M, M, scale), c.st)) != hipSuccess) return e;
  if ((e = tattn_forward(attn_args(sb.Q + (size_t)R0 * D, sb.K + (size_t)R0 * D, sb.V + (size_t)R0 * D,
                                   sb.O + (size_t)R0 * D, sb.LSE + lse1, B, H, N, N, scale),
                         c.st)) != hipSuccess)
    return e;
  if ((e = linear(c, sb.O, D, R, D, P.w(sp + ".out_proj.weight"), P.w(sp + ".out_proj.bias"), D, sb.CAT + D, 2 * D)) !=
      hipSuccess)
    return e;
  if ((e = ffn_forward(c, P, sp, X, sb, R)) != hipSuccess) return e;
  // CrossBlock (:220-249)
  Blk& cb = s.cross[l];
  if ((e = linear(c, sb.Y, D, R, D, P.w(cp + ".to_qk.weight"), P.w(cp + ".to_qk.bias"), D, cb.Q, D)) != hipSuccess) return e;
  if ((e = linear(c, sb.Y, D, R, D, P.w(cp + ".to_v.weight"), P.w(cp + ".to_v.bias"), D, cb.V, D)) != hipSuccess) return e;
  // m0 = softmax_j(sim) v1 (image-0 queries), m1 = softmax_i(sim)^T v0 (image-1 queries)
  if ((e = tattn_forward(attn_args(cb.Q, cb.Q + (size_t)R0 * D, cb.V + (size_t)R0 * D, cb.O, cb.LSE, B, H, M, N, scale),
                         c.st)) != hipSuccess)
    return e;
  if ((e = tattn_forward(attn_args(cb.Q + (size_t)R0 * D, cb.Q, cb.V, cb.O + (size_t)R0 * D, cb.LSE + lse1, B, H, N, M, scale),
                         c.st)) != hipSuccess)
    return e;
  if ((e = linear(c, cb.O, D, R, D, P.w(cp + ".to_out.weight"), P.w(cp + ".to_out.bias"), D, cb.CAT + D, 2 * D)) !=
      hipSuccess)
    return e;
  return ffn_forward(c, P, cp, sb.Y, cb, R);
}

int check_shape(const lg_handle_t* h, int B, int M, int N) {
  if (!h) return fail(LG_E_INVALID, "null handle");
  if (B <= 0) return fail(LG_E_INVALID, "batch must be >= 1");
  if (M <= 0 || N <= 0) return fail(LG_E_INVALID, "empty keypoint set");
  if ((long long)B * (M + N) > (1ll << 30) / 1024) return fail(LG_E_INVALID, "row count too large");
  return LG_OK;
}

}  // namespace

extern "C" {

int lg_train_saved_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes) {
  if (int e = check_shape(h, B, M, N)) return e;
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  *bytes = carve_saved(nullptr, dims_of(h, B, M, N), false).bytes;
  return LG_OK;
}

int lg_train_saved_bytes_ex(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, int32_t flags, size_t* bytes) {
  if (int e = check_shape(h, B, M, N)) return e;
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  *bytes = carve_saved(nullptr, dims_of(h, B, M, N), (flags & LG_FWD_CHECKPOINTED) != 0).bytes;
  return LG_OK;
}

int lg_train_scratch_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes) {
  if (int e = check_shape(h, B, M, N)) return e;
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  *bytes = carve_scratch(nullptr, dims_of(h, B, M, N)).bytes;
  return LG_OK;
}

int lg_train_forward(lg_handle_t* h, const float* const* params, const lg_inputs_t* in, float* layer_descriptors0,
                     float* layer_descriptors1, void* saved, size_t saved_bytes, void* stream) {
  if (!in || !params || !saved) return fail(LG_E_INVALID, "null argument");
  if (int e = check_shape(h, in->B, in->M, in->N)) return e;
  if (!in->keypoints0 || !in->keypoints1 || !in->descriptors0 || !in->descriptors1)
    return fail(LG_E_INVALID, "null input tensor");
  if (in->num_keypoints0 || in->num_keypoints1)
    return fail(LG_E_INVALID, "num_keypoints0/1 (ragged batches) are not supported by the training kernels");
  const Dims d = dims_of(h, in->B, in->M, in->N);
  if (d.m_in == 4 && (!in->scales0 || !in->oris0 || !in->scales1 || !in->oris1))
    return fail(LG_E_INVALID, "add_scale_ori needs scales0/1 and oris0/1");
  const bool ckpt = (in->flags & LG_FWD_CHECKPOINTED) != 0;
  Saved s = carve_saved((char*)saved, d, ckpt);
  if (saved_bytes < s.bytes) return fail(LG_E_WORKSPACE, "saved buffer too small: need " + std::to_string(s.bytes));
  LG_HIP(hipSetDevice(handle_device(h)));
  const Ctx c{(hipStream_t)stream, nullptr, 0, nullptr};
  const Params P{h, params, nullptr};
  const int B = d.B, M = d.M, N = d.N, R = d.R, R0 = d.R0;
  // positional encoding (lightglue.py:452-456,490-494); no image_size: min/max extent (:25-26)
  if (in->image_size0) LG_HIP(hipMemcpyAsync(s.SZ, in->image_size0, 2 * B * sizeof(float), hipMemcpyDeviceToDevice, c.st));
  else LG_HIP(kpt_extent(in->keypoints0, B, M, s.SZ, c.st));
  if (in->image_size1)
    LG_HIP(hipMemcpyAsync(s.SZ + 2 * B, in->image_size1, 2 * B * sizeof(float), hipMemcpyDeviceToDevice, c.st));
  else LG_HIP(kpt_extent(in->keypoints1, B, N, s.SZ + 2 * B, c.st));
  for (int img = 0; img < 2; ++img) {
    TPE p{};
    p.kpts = img ? in->keypoints1 : in->keypoints0;
    p.size = s.SZ + 2 * B * img;
    p.scales = img ? in->scales1 : in->scales0;
    p.oris = img ? in->oris1 : in->oris0;
    p.Wr = P.w("posenc.Wr.weight");
    p.Wc = P.w("posenc.condition_modulation.weight");
    p.bc = P.w("posenc.condition_modulation.bias");
    p.B = B;
    p.n = img ? N : M;
    p.m_in = d.m_in;
    const size_t r0 = img ? R0 : 0;
    p.x = s.PEX + r0 * 4;
    p.cosb = s.COS + r0 * 32;
    p.sinb = s.SIN + r0 * 32;
    LG_HIP(pe_train(p, c.st));
  }
  // input descriptors (input_proj, :370-373,486-487)
  if (d.proj) {
    LG_HIP(hipMemcpyAsync(s.Din, in->descriptors0, (size_t)R0 * d.din * 4, hipMemcpyDeviceToDevice, c.st));
    LG_HIP(hipMemcpyAsync(s.Din + (size_t)R0 * d.din, in->descriptors1, (size_t)(R - R0) * d.din * 4,
                          hipMemcpyDeviceToDevice, c.st));
    LG_HIP(linear(c, s.Din, d.din, R, d.din, P.w("input_proj.weight"), P.w("input_proj.bias"), D, s.X0, D));
  } else {
    LG_HIP(hipMemcpyAsync(s.X0, in->descriptors0, (size_t)R0 * D * 4, hipMemcpyDeviceToDevice, c.st));
    LG_HIP(hipMemcpyAsync(s.X0 + (size_t)R0 * D, in->descriptors1, (size_t)(R - R0) * D * 4, hipMemcpyDeviceToDevice, c.st));
  }
  for (int l = 0; l < d.L; ++l) {
    LG_HIP(layer_forward(c, P, s, d, l));
    const Blk& cb = s.cross[l];
    // ref_descriptors*[:, l] (:521-524,572)
    if (layer_descriptors0)
      LG_HIP(hipMemcpy2DAsync(layer_descriptors0 + (size_t)l * M * D, (size_t)d.L * M * D * 4, cb.Y, (size_t)M * D * 4,
                              (size_t)M * D * 4, B, hipMemcpyDeviceToDevice, c.st));
    if (layer_descriptors1)
      LG_HIP(hipMemcpy2DAsync(layer_descriptors1 + (size_t)l * N * D, (size_t)d.L * N * D * 4, cb.Y + (size_t)R0 * D,
                              (size_t)N * D * 4, (size_t)N * D * 4, B, hipMemcpyDeviceToDevice, c.st));
  }
  return LG_OK;
}

int lg_train_backward(lg_handle_t* h, const float* const* params, const lg_inputs_t* in, const void* saved,
                      size_t saved_bytes, const float* grad_layer_descriptors0, const float* grad_layer_descriptors1,
                      float* const* grads, float* grad_desc0, float* grad_desc1, void* scratch, size_t scratch_bytes,
                      void* stream) {
  if (!in || !params || !saved || !scratch) return fail(LG_E_INVALID, "null argument");
  if (int e = check_shape(h, in->B, in->M, in->N)) return e;
  const Dims d = dims_of(h, in->B, in->M, in->N);
  const bool ckpt = (in->flags & LG_FWD_CHECKPOINTED) != 0;
  Saved s = carve_saved((char*)saved, d, ckpt);
  if (saved_bytes < s.bytes) return fail(LG_E_WORKSPACE, "saved buffer too small");
  Scratch w = carve_scratch((char*)scratch, d);
  if (scratch_bytes < w.bytes) return fail(LG_E_WORKSPACE, "scratch too small: need " + std::to_string(w.bytes));
  LG_HIP(hipSetDevice(handle_device(h)));
  const Ctx c{(hipStream_t)stream, w.WS, w.ws_floats, w.PART};
  const Params P{h, params, grads};
  const int B = d.B, M = d.M, N = d.N, R = d.R, R0 = d.R0, H = d.H;
  const float scale = 0.125f;
  const size_t lse1 = (size_t)B * H * M;
  const size_t o1 = (size_t)R0 * D;
  LG_HIP(hipMemsetAsync(w.GX, 0, (size_t)R * D * 4, c.st));
  LG_HIP(hipMemsetAsync(w.GCOS, 0, (size_t)R * 32 * 4, c.st));
  LG_HIP(hipMemsetAsync(w.GSIN, 0, (size_t)R * 32 * 4, c.st));
  for (int l = d.L - 1; l >= 0; --l) {
    const std::string sp = "transformers." + std::to_string(l) + ".self_attn";
    const std::string cp = "transformers." + std::to_string(l) + ".cross_attn";
    const Blk& sb = s.self[l];
    const Blk& cb = s.cross[l];
    const float* X = l == 0 ? s.X0 : s.cross[l - 1].Y;
    // checkpointed: recompute layer l's activations from its saved input (torch.utils.checkpoint's
    // recomputation, lightglue.py:515-518); the forward kernels are deterministic, so they are the
    // forward pass's values exactly
    if (ckpt) LG_HIP(layer_forward(Ctx{c.st, nullptr, 0, nullptr}, P, s, d, l));  // the forward's Ctx: same GEMM splits
    // d/d(layer output) += the heads' gradient of ref_descriptors*[:, l]
    LG_HIP(add_layer_rows(w.GX, grad_layer_descriptors0, grad_layer_descriptors1, B, M, N, d.L, l, c.st));
    // ---- CrossBlock backward: GX -> GY (d/d self-block output sb.Y)
    LG_HIP(ffn_backward(c, P, cp, cb, sb.Y, w.GX, w.GY, w, R));
    const float* gmsg = w.GC + D;
    LG_HIP(linear_wgrad(c, gmsg, 2 * D, cb.O, D, R, D, D, P.gr(cp + ".to_out.weight"), P.gr(cp + ".to_out.bias")));
    LG_HIP(linear_dgrad(c, gmsg, 2 * D, R, D, P.w(cp + ".to_out.weight"), D, w.GO, D));
    LG_HIP(attn_delta(cb.O, w.GO, D, B, H, M, w.DELTA, c.st));
    LG_HIP(attn_delta(cb.O + o1, w.GO + o1, D, B, H, N, w.DELTA + lse1, c.st));
    LG_HIP(hipMemsetAsync(w.GQ + o1, 0, (size_t)(R - R0) * D * 4, c.st));
    {  // path 1 (image-1 queries over image-0 keys): dQ -> gqk1 (atomics), dK -> gqk0, dV -> gv0
      TAttn a = attn_args(cb.Q + o1, cb.Q, cb.V, cb.O + o1, cb.LSE + lse1, B, H, N, M, scale);
      a.dO = w.GO + o1;
      a.delta = w.DELTA + lse1;
      a.dQ = w.GQ + o1;
      a.dK = w.GQ;
      a.dV = w.GV;
      a.accum_kv = 0;
      LG_HIP(tattn_backward(a, c.st));
    }
    {  // path 0 (image-0 queries over image-1 keys): dQ -> gqk0 (+= onto path 1's dK), dK += gqk1
      TAttn a = attn_args(cb.Q, cb.Q + o1, cb.V + o1, cb.O, cb.LSE, B, H, M, N, scale);
      a.dO = w.GO;
      a.delta = w.DELTA;
      a.dQ = w.GQ;
      a.dK = w.GQ + o1;
      a.dV = w.GV + o1;
      a.accum_kv = 1;
      LG_HIP(hipMemsetAsync(w.GV + o1, 0, (size_t)(R - R0) * D * 4, c.st));
      LG_HIP(tattn_backward(a, c.st));
    }
    LG_HIP(linear_wgrad(c, w.GQ, D, sb.Y, D, R, D, D, P.gr(cp + ".to_qk.weight"), P.gr(cp + ".to_qk.bias")));
    LG_HIP(linear_wgrad(c, w.GV, D, sb.Y, D, R, D, D, P.gr(cp + ".to_v.weight"), P.gr(cp + ".to_v.bias")));
    LG_HIP(linear_dgrad(c, w.GQ, D, R, D, P.w(cp + ".to_qk.weight"), D, w.GY, D, 1.f));
    LG_HIP(linear_dgrad(c, w.GV, D, R, D, P.w(cp + ".to_v.weight"), D, w.GY, D, 1.f));
    // ---- SelfBlock backward: GY -> GX (d/d layer input X)
    LG_HIP(ffn_backward(c, P, sp, sb, X, w.GY, w.GX, w, R));
    LG_HIP(linear_wgrad(c, gmsg, 2 * D, sb.O, D, R, D, D, P.gr(sp + ".out_proj.weight"), P.gr(sp + ".out_proj.bias")));
    LG_HIP(linear_dgrad(c, gmsg, 2 * D, R, D, P.w(sp + ".out_proj.weight"), D, w.GO, D));
    LG_HIP(attn_delta(sb.O, w.GO, D, B, H, M, w.DELTA, c.st));
    LG_HIP(attn_delta(sb.O + o1, w.GO + o1, D, B, H, N, w.DELTA + lse1, c.st));
    LG_HIP(hipMemsetAsync(w.GQ, 0, (size_t)R * D * 4, c.st));
    for (int img = 0; img < 2; ++img) {
      const size_t off = img ? o1 : 0;
      const int n = img ? N : M;
      TAttn a = attn_args(sb.Q + off, sb.K + off, sb.V + off, sb.O + off, sb.LSE + (img ? lse1 : 0), B, H, n, n, scale);
      a.dO = w.GO + off;
      a.delta = w.DELTA + (img ? lse1 : 0);
      a.dQ = w.GQ + off;
      a.dK = w.GK + off;
      a.dV = w.GV + off;
      LG_HIP(tattn_backward(a, c.st));
    }
    LG_HIP(rotary_split_bwd(w.GQ, w.GK, w.GV, sb.Q, sb.K, s.COS, s.SIN, R, H, w.GQKV, w.GCOS, w.GSIN, c.st));
    LG_HIP(linear_wgrad(c, w.GQKV, 3 * D, X, D, R, 3 * D, D, P.gr(sp + ".Wqkv.weight"), P.gr(sp + ".Wqkv.bias")));
    // transformers.<l>.* are final: a data-parallel caller starts this bucket's all-reduce now,
    // under the remaining layers' backward (DDP's overlap, train.py:309)
    handle_grad_ready(h, l, stream);
    LG_HIP(linear_dgrad(c, w.GQKV, 3 * D, R, 3 * D, P.w(sp + ".Wqkv.weight"), D, w.GX, D, 1.f));
  }
  // GX = d/d(X0): input_proj (:486-487) and the input descriptors
  if (d.proj) {
    LG_HIP(linear_wgrad(c, w.GX, D, s.Din, d.din, R, D, d.din, P.gr("input_proj.weight"), P.gr("input_proj.bias")));
    if (grad_desc0) LG_HIP(linear_dgrad(c, w.GX, D, R0, D, P.w("input_proj.weight"), d.din, grad_desc0, d.din));
    if (grad_desc1) LG_HIP(linear_dgrad(c, w.GX + o1, D, R - R0, D, P.w("input_proj.weight"), d.din, grad_desc1, d.din));
  } else {
    if (grad_desc0) LG_HIP(hipMemcpyAsync(grad_desc0, w.GX, o1 * 4, hipMemcpyDeviceToDevice, c.st));
    if (grad_desc1) LG_HIP(hipMemcpyAsync(grad_desc1, w.GX + o1, (size_t)(R - R0) * D * 4, hipMemcpyDeviceToDevice, c.st));
  }
  // posenc (:63-77): d/d(Wr, condition_modulation) from the rotary's cos / sin gradients
  float* gWr = P.gr("posenc.Wr.weight");
  float* gWc = P.gr("posenc.condition_modulation.weight");
  float* gbc = P.gr("posenc.condition_modulation.bias");
  // any requested subset (a frozen parameter's gradient pointer is null)
  if (gWr || gWc || gbc)
    LG_HIP(pe_backward(s.PEX, s.COS, s.SIN, w.GCOS, w.GSIN, R, R0, (float)M, (float)N, d.m_in, w.PART, gWr, gWc, gbc, c.st));
  handle_grad_ready(h, -1, stream);  // input_proj.*, posenc.*
  return LG_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ assignment head backward
namespace {
struct HeadScratch {
  float *X, *MD, *GMD, *SIM, *Z, *GZ, *LSER, *LSEC, *RS, *GD, *GT, *WS, *PART, *NLLP;
  size_t ws_floats, bytes;
};
HeadScratch carve_head_scratch(char* base, int B, int M, int N) {
  Carver c{base};
  HeadScratch s;
  const size_t R = (size_t)B * (M + N);
  s.X = c.f(R * D);
  s.MD = c.f(R * D);
  s.GMD = c.f(R * D);
  s.SIM = c.f((size_t)B * M * N);
  s.Z = c.f(R);
  s.GZ = c.f(R);
  s.LSER = c.f((size_t)B * M);
  s.LSEC = c.f((size_t)B * N);
  s.RS = c.f(R);  // row sums (image-0 rows) then column sums (image-1 rows)
  s.GD = c.f(R);  // dustbin-column entries then dustbin-row entries
  s.GT = c.f(R);
  s.ws_floats = std::max({tgemm_ws_floats(D, D, (int)R, 1), tgemm_ws_floats(M, D, N, B), tgemm_ws_floats(N, D, M, B)});
  s.WS = c.f(s.ws_floats + 64);
  s.PART = c.f(std::max({colsum_part_floats((int)R, D), sim_lse_part_floats(B, M, N), la_grad_sums_part_floats(B, M, N),
                                la_grad_gt_part_floats(B, M, N), head_vec_grads_part_floats((int)R)}) + 64);
  s.NLLP = c.f(la_nll_part_floats(B, M, N));
  s.bytes = c.off;
  return s;
}
}  // namespace

extern "C" {

int lg_head_scratch_bytes(const lg_handle_t* h, int32_t B, int32_t M, int32_t N, size_t* bytes) {
  if (int e = check_shape(h, B, M, N)) return e;
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  *bytes = carve_head_scratch(nullptr, B, M, N).bytes;
  return LG_OK;
}

}  // extern "C"

namespace {
// the NLL weights as the ground truth itself (lg_head_nll_backward)
struct GtWeights {
  const uint8_t* gta;
  const int64_t* gt0;
  const int64_t* gt1;
};
// `from_forward`: scratch still holds md, z, sim and its LSEs from lg_head_forward (same layer,
// inputs and shape, similarity == NULL there), so they are not recomputed
int head_backward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0, const float* desc1,
                  int32_t B, int32_t M, int32_t N, const float* la_grad, const float* s_in, const float* s_dust,
                  const float* grad_similarity, const float* grad_token0, const float* grad_token1, float* const* grads,
                  float* grad_desc0, float* grad_desc1, void* scratch, size_t scratch_bytes, void* stream,
                  bool from_forward, const GtWeights* gt = nullptr) {
  if (!params || !desc0 || !desc1 || !(la_grad || gt) || !scratch) return fail(LG_E_INVALID, "null argument");
  if (gt && (!gt->gta || !gt->gt0 || !gt->gt1 || !s_in || !s_dust)) return fail(LG_E_INVALID, "null argument");
  if (gt && M != N)
    return fail(LG_E_INVALID, "the NLL weights need M == N (losses.py:62-73 writes gt_matches1 at [:, -1, :m])");
  if (int e = check_shape(h, B, M, N)) return e;
  const int L = handle_config(h)->n_layers;
  if (layer < 0) layer += L;
  if (layer < 0 || layer >= L) return fail(LG_E_INVALID, "layer index out of range");
  if ((grad_token0 || grad_token1) && layer >= L - 1)
    return fail(LG_E_INVALID, "token_confidence exists for layers 0..n_layers-2 only (lightglue.py:395-397)");
  HeadScratch s = carve_head_scratch((char*)scratch, B, M, N);
  if (scratch_bytes < s.bytes) return fail(LG_E_WORKSPACE, "scratch too small: need " + std::to_string(s.bytes));
  LG_HIP(hipSetDevice(handle_device(h)));
  const Ctx c{(hipStream_t)stream, s.WS, s.ws_floats, s.PART};
  const Params P{h, params, grads};
  const std::string a = "log_assignment." + std::to_string(layer);
  const int R0 = B * M, R = B * (M + N);
  const size_t o1 = (size_t)R0 * D;
  const float* Wf = P.w(a + ".final_proj.weight");
  const float* wm = P.w(a + ".matchability.weight");
  LG_HIP(hipMemcpyAsync(s.X, desc0, o1 * 4, hipMemcpyDeviceToDevice, c.st));
  LG_HIP(hipMemcpyAsync(s.X + o1, desc1, (size_t)(R - R0) * D * 4, hipMemcpyDeviceToDevice, c.st));
  if (!from_forward) {
    // recompute: md = final_proj(desc) / 4, z = matchability(desc), sim = md0 md1^T (:306-315)
    LG_HIP(linear(c, s.X, D, R, D, Wf, P.w(a + ".final_proj.bias"), D, s.MD, D, 0.f, 0.25f));
    LG_HIP(gemv256(s.X, R, wm, P.w(a + ".matchability.bias"), s.Z, c.st));
    TGemm g{s.MD, s.MD + o1, s.SIM, D, D, N, (long long)M * D, (long long)N * D, (long long)M * N, M, N, D, B, 1.f, 0.f, nullptr};
    LG_HIP(tgemm(g, false, true, c.ws, c.ws_floats, c.st));
    LG_HIP(sim_lse(s.SIM, B, M, N, s.LSER, s.LSEC, c.part, c.st));
  }
  // sigmoid_log_double_softmax backward (:284-296)
  if (gt) {
    LG_HIP(la_grad_gt(s.SIM, gt->gta, gt->gt0, gt->gt1, s_in, s_dust, s.LSER, s.LSEC, B, M, N, s.RS, s.RS + R0, s.GD,
                      s.GD + R0, c.part, c.st));
  } else {
    LG_HIP(la_grad_sums(la_grad, s_in, s_dust, B, M, N, s.RS, s.RS + R0, s.GD, s.GD + R0, c.part, c.st));
    LG_HIP(la_grad_sim(s.SIM, la_grad, s_in, s.LSER, s.LSEC, s.RS, s.RS + R0, grad_similarity, B, M, N, c.st));
  }
  LG_HIP(la_grad_z(s.Z, s.RS, s.GD, R, s.GZ, c.st));
  // d/d(final_proj output) = d/d(md) / 4: gmd0 = gsim md1, gmd1 = gsim^T md0
  if (N % 16 == 0) {  // gmd0 on the bf16x6 GEMM through md1^T; the f32 MFMA kernel on md1 as is otherwise
    float* md1t = s.GMD + o1;  // [B][D][N]: free until the d(md1) product below
    LG_HIP(transpose_batched(s.MD + o1, N, D, B, md1t, c.st));
    TGemm g{s.SIM, md1t, s.GMD, N, N, D, (long long)M * N, (long long)D * N, (long long)M * D, M, D, N, B, 0.25f, 0.f, nullptr};
    LG_HIP(tgemm(g, false, true, c.ws, c.ws_floats, c.st));
  } else {
    TGemm g{s.SIM, s.MD + o1, s.GMD, N, D, D, (long long)M * N, (long long)N * D, (long long)M * D, M, D, N, B, 0.25f, 0.f, nullptr};
    LG_HIP(tgemm(g, false, false, c.ws, c.ws_floats, c.st));
  }
  {
    TGemm g{s.SIM, s.MD, s.GMD + o1, N, D, D, (long long)M * N, (long long)M * D, (long long)N * D, N, D, M, B, 0.25f, 0.f, nullptr};
    LG_HIP(tgemm(g, true, false, c.ws, c.ws_floats, c.st));
  }
  LG_HIP(linear_wgrad(c, s.GMD, D, s.X, D, R, D, D, P.gr(a + ".final_proj.weight"), P.gr(a + ".final_proj.bias")));
  const bool tok = grad_token0 || grad_token1;
  if (tok) {  // TokenConfidence's logit gradient (:108-122), [R]
    if (grad_token0) LG_HIP(hipMemcpyAsync(s.GT, grad_token0, (size_t)R0 * 4, hipMemcpyDeviceToDevice, c.st));
    else LG_HIP(hipMemsetAsync(s.GT, 0, (size_t)R0 * 4, c.st));
    if (grad_token1) LG_HIP(hipMemcpyAsync(s.GT + R0, grad_token1, (size_t)(R - R0) * 4, hipMemcpyDeviceToDevice, c.st));
    else LG_HIP(hipMemsetAsync(s.GT + R0, 0, (size_t)(R - R0) * 4, c.st));
  }
  const std::string t = "token_confidence." + std::to_string(layer) + ".token.0";
  // matchability's and the token linear's gradients in one read of X (TokenConfidence, :108-122:
  // logits = token(desc.detach()) -> the token Linear only)
  LG_HIP(head_vec_grads(s.X, R, s.GZ, tok ? s.GT : nullptr, c.part, P.gr(a + ".matchability.weight"),
                        P.gr(a + ".matchability.bias"), tok ? P.gr(t + ".weight") : nullptr,
                        tok ? P.gr(t + ".bias") : nullptr, c.st));
  if (grad_desc0) {
    LG_HIP(linear_dgrad(c, s.GMD, D, R0, D, Wf, D, grad_desc0, D));
    LG_HIP(rank1_add256(grad_desc0, R0, s.GZ, wm, c.st));
  }
  if (grad_desc1) {
    LG_HIP(linear_dgrad(c, s.GMD + o1, D, R - R0, D, Wf, D, grad_desc1, D));
    LG_HIP(rank1_add256(grad_desc1, R - R0, s.GZ + R0, wm, c.st));
  }
  return LG_OK;
}
}  // namespace

extern "C" {

int lg_head_backward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0, const float* desc1,
                     int32_t B, int32_t M, int32_t N, const float* la_grad, const float* s_in, const float* s_dust,
                     const float* grad_similarity, const float* grad_token0, const float* grad_token1,
                     float* const* grads, float* grad_desc0, float* grad_desc1, void* scratch, size_t scratch_bytes,
                     void* stream) {
  return head_backward(h, params, layer, desc0, desc1, B, M, N, la_grad, s_in, s_dust, grad_similarity, grad_token0,
                       grad_token1, grads, grad_desc0, grad_desc1, scratch, scratch_bytes, stream, false);
}

int lg_head_backward_from_forward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0,
                                  const float* desc1, int32_t B, int32_t M, int32_t N, const float* la_grad,
                                  const float* s_in, const float* s_dust, const float* grad_similarity,
                                  const float* grad_token0, const float* grad_token1, float* const* grads,
                                  float* grad_desc0, float* grad_desc1, void* scratch, size_t scratch_bytes,
                                  void* stream) {
  return head_backward(h, params, layer, desc0, desc1, B, M, N, la_grad, s_in, s_dust, grad_similarity, grad_token0,
                       grad_token1, grads, grad_desc0, grad_desc1, scratch, scratch_bytes, stream, true);
}

int lg_head_nll_backward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0,
                         const float* desc1, int32_t B, int32_t M, int32_t N, const uint8_t* gt_assignment,
                         const int64_t* gt_matches0, const int64_t* gt_matches1, const float* s_in, const float* s_dust,
                         const float* grad_token0, const float* grad_token1, float* const* grads, float* grad_desc0,
                         float* grad_desc1, int32_t from_forward, void* scratch, size_t scratch_bytes, void* stream) {
  const GtWeights gt{gt_assignment, gt_matches0, gt_matches1};
  return head_backward(h, params, layer, desc0, desc1, B, M, N, nullptr, s_in, s_dust, nullptr, grad_token0, grad_token1,
                       grads, grad_desc0, grad_desc1, scratch, scratch_bytes, stream, from_forward != 0, &gt);
}

int lg_head_nll_forward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0, const float* desc1,
                        int32_t B, int32_t M, int32_t N, const uint8_t* gt_assignment, const int64_t* gt_matches0,
                        const int64_t* gt_matches1, int32_t mode, float balancing, float* out, int64_t* argmax0,
                        int64_t* argmax1, float* token_logits0, float* token_logits1, void* scratch, size_t scratch_bytes,
                        void* stream) {
  if (!params || !desc0 || !desc1 || !gt_assignment || !gt_matches0 || !gt_matches1 || !out || !argmax0 || !argmax1 ||
      !scratch)
    return fail(LG_E_INVALID, "null argument");
  if (int e = check_shape(h, B, M, N)) return e;
  if (mode != 0 && mode != 1) return fail(LG_E_INVALID, "mode must be 0 or 1");
  if (mode == 1 && M != N)  // losses.py:66-70 writes the dustbin-row weights at [:, -1, :m]
    return fail(LG_E_INVALID, "NLLLoss weights need M == N (losses.py:66-70)");
  if (N > 4096) return fail(LG_E_INVALID, "lg_head_nll_forward handles N <= 4096");
  const int L = handle_config(h)->n_layers;
  if (layer < 0) layer += L;
  if (layer < 0 || layer >= L) return fail(LG_E_INVALID, "layer index out of range");
  if ((token_logits0 || token_logits1) && layer >= L - 1)
    return fail(LG_E_INVALID, "token_confidence exists for layers 0..n_layers-2 only (lightglue.py:395-397)");
  HeadScratch s = carve_head_scratch((char*)scratch, B, M, N);
  if (scratch_bytes < s.bytes) return fail(LG_E_WORKSPACE, "scratch too small: need " + std::to_string(s.bytes));
  LG_HIP(hipSetDevice(handle_device(h)));
  const Ctx c{(hipStream_t)stream, s.WS, s.ws_floats, s.PART};
  const Params P{h, params, nullptr};
  const std::string a = "log_assignment." + std::to_string(layer);
  const int R0 = B * M, R = B * (M + N);
  const size_t o1 = (size_t)R0 * D;
  for (int im = 0; im < 2; ++im) {  // md, z, sim, its LSEs: as lg_head_forward
    const float* dsc = im ? desc1 : desc0;
    const int rows = im ? R - R0 : R0;
    const size_t o = im ? o1 : 0;
    LG_HIP(linear(c, dsc, D, rows, D, P.w(a + ".final_proj.weight"), P.w(a + ".final_proj.bias"), D, s.MD + o, D, 0.f,
                  0.25f));
    LG_HIP(gemv256(dsc, rows, P.w(a + ".matchability.weight"), P.w(a + ".matchability.bias"), s.Z + (im ? R0 : 0), c.st));
  }
  {
    TGemm g{s.MD, s.MD + o1, s.SIM, D, D, N, (long long)M * D, (long long)N * D, (long long)M * N, M, N, D, B, 1.f, 0.f, nullptr};
    LG_HIP(tgemm(g, false, true, c.ws, c.ws_floats, c.st));
  }
  LG_HIP(sim_lse(s.SIM, B, M, N, s.LSER, s.LSEC, c.part, c.st));
  LG_HIP(la_nll(s.SIM, s.LSER, s.LSEC, s.Z, s.Z + R0, B, M, N, gt_assignment, gt_matches0, gt_matches1, mode, balancing, out,
                argmax0, argmax1, s.NLLP, c.st));
  if (token_logits0 || token_logits1) {
    const std::string t = "token_confidence." + std::to_string(layer) + ".token.0";
    if (token_logits0) LG_HIP(gemv256(desc0, R0, P.w(t + ".weight"), P.w(t + ".bias"), token_logits0, c.st));
    if (token_logits1) LG_HIP(gemv256(desc1, R - R0, P.w(t + ".weight"), P.w(t + ".bias"), token_logits1, c.st));
  }
  return LG_OK;
}

int lg_head_forward(lg_handle_t* h, const float* const* params, int32_t layer, const float* desc0, const float* desc1,
                    int32_t B, int32_t M, int32_t N, float* log_assignment, float* similarity, float* token_logits0,
                    float* token_logits1, void* scratch, size_t scratch_bytes, void* stream) {
  if (!params || !desc0 || !desc1 || !log_assignment || !scratch) return fail(LG_E_INVALID, "null argument");
  if (int e = check_shape(h, B, M, N)) return e;
  const int L = handle_config(h)->n_layers;
  if (layer < 0) layer += L;
  if (layer < 0 || layer >= L) return fail(LG_E_INVALID, "layer index out of range");
  if ((token_logits0 || token_logits1) && layer >= L - 1)
    return fail(LG_E_INVALID, "token_confidence exists for layers 0..n_layers-2 only (lightglue.py:395-397)");
  HeadScratch s = carve_head_scratch((char*)scratch, B, M, N);
  if (scratch_bytes < s.bytes) return fail(LG_E_WORKSPACE, "scratch too small: need " + std::to_string(s.bytes));
  LG_HIP(hipSetDevice(handle_device(h)));
  const Ctx c{(hipStream_t)stream, s.WS, s.ws_floats, s.PART};
  const Params P{h, params, nullptr};
  const std::string a = "log_assignment." + std::to_string(layer);
  const int R0 = B * M, R = B * (M + N);
  const size_t o1 = (size_t)R0 * D;
  float* sim = similarity ? similarity : s.SIM;
  // md = final_proj(desc) / d**0.25, z = matchability(desc), sim = md0 md1^T (:306-315)
  // per image, straight from the inputs (row-wise products: the same values as one call over both)
  for (int im = 0; im < 2; ++im) {
    const float* dsc = im ? desc1 : desc0;
    const int rows = im ? R - R0 : R0;
    const size_t o = im ? o1 : 0;
    LG_HIP(linear(c, dsc, D, rows, D, P.w(a + ".final_proj.weight"), P.w(a + ".final_proj.bias"), D, s.MD + o, D, 0.f,
                  0.25f));
    LG_HIP(gemv256(dsc, rows, P.w(a + ".matchability.weight"), P.w(a + ".matchability.bias"), s.Z + (im ? R0 : 0), c.st));
  }
  {
    TGemm g{s.MD, s.MD + o1, sim, D, D, N, (long long)M * D, (long long)N * D, (long long)M * N, M, N, D, B, 1.f, 0.f, nullptr};
    LG_HIP(tgemm(g, false, true, c.ws, c.ws_floats, c.st));
  }
  LG_HIP(sim_lse(sim, B, M, N, s.LSER, s.LSEC, c.part, c.st));
  LG_HIP(la_forward(sim, s.LSER, s.LSEC, s.Z, s.Z + R0, B, M, N, log_assignment, c.st));
  if (token_logits0 || token_logits1) {  // TokenConfidence's Linear (:109-110)
    const std::string t = "token_confidence." + std::to_string(layer) + ".token.0";
    if (token_logits0) LG_HIP(gemv256(desc0, R0, P.w(t + ".weight"), P.w(t + ".bias"), token_logits0, c.st));
    if (token_logits1) LG_HIP(gemv256(desc1, R - R0, P.w(t + ".weight"), P.w(t + ".bias"), token_logits1, c.st));
  }
  return LG_OK;
}

// ------------------------------------------------------------------ kernel-level entries (tests)
int lg_train_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t batch, size_t* bytes) {
  if (!bytes || M < 0 || N < 0 || K < 0 || batch < 0) return fail(LG_E_INVALID, "bad argument");
  // split-k partials, or the transposed B of an input-gradient product (tgemm's bf16x6 route)
  *bytes = std::max(tgemm_ws_floats(M, N, K, batch), (size_t)N * K + 4) * sizeof(float);
  return LG_OK;
}

int lg_train_gemm(const float* A, const float* Bm, float* C, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA,
                  int64_t sB, int64_t sC, int32_t M, int32_t N, int32_t K, int32_t batch, float alpha, float beta,
                  const float* bias, int32_t ta, int32_t tb, void* workspace, size_t workspace_bytes, void* stream) {
  if (!A || !Bm || !C || M < 0 || N < 0 || K < 0 || batch < 0) return fail(LG_E_INVALID, "bad argument");
  TGemm g{A, Bm, C, lda, ldb, ldc, sA, sB, sC, M, N, K, batch, alpha, beta, bias};
  LG_HIP(tgemm(g, ta != 0, tb != 0, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream));
  LG_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LG_OK;
}

int lg_train_gemm_ex(const float* A, const float* Bm, float* C, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA,
                     int64_t sB, int64_t sC, int32_t M, int32_t N, int32_t K, int32_t batch, float alpha, float beta,
                     const float* bias, int32_t ta, int32_t tb, const float* A1, int64_t lda1, int32_t K0, const float* B1,
                     int64_t ldb1, int32_t N0, const float* R, int64_t ldr, float* colsumA, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (!A || !Bm || !C || M < 0 || N < 0 || K < 0 || batch < 0) return fail(LG_E_INVALID, "bad argument");
  TGemm g{A, Bm, C, lda, ldb, ldc, sA, sB, sC, M, N, K, batch, alpha, beta, bias};
  g.A1 = A1;
  g.lda1 = lda1;
  g.K0 = K0;
  g.B1 = B1;
  g.ldb1 = ldb1;
  g.N0 = N0;
  g.R = R;
  g.ldr = ldr;
  g.colsumA = colsumA;
  const hipError_t e = tgemm(g, ta != 0, tb != 0, (float*)workspace, workspace_bytes / sizeof(float), (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(LG_E_INVALID, "no route of the training GEMM takes these operands");
  LG_HIP(e);
  LG_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LG_OK;
}

int lg_train_attention(const float* q, const float* k, const float* v, int32_t B, int32_t H, int32_t Nq, int32_t Nk,
                       float scale, float* o, float* lse, void* stream) {
  if (!q || !k || !v || !o || !lse || B < 0 || H <= 0 || H * 64 != D || Nq < 0 || Nk <= 0)
    return fail(LG_E_INVALID, "bad argument");
  LG_HIP(tattn_forward(attn_args(q, k, v, o, lse, B, H, Nq, Nk, scale), (hipStream_t)stream));
  LG_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LG_OK;
}

int lg_train_attention_backward(const float* q, const float* k, const float* v, const float* o, const float* lse,
                                const float* grad_o, int32_t B, int32_t H, int32_t Nq, int32_t Nk, float scale,
                                float* grad_q, float* grad_k, float* grad_v, float* delta_ws, void* stream) {
  if (!q || !k || !v || !o || !lse || !grad_o || !grad_q || !grad_k || !grad_v || !delta_ws || B < 0 || H <= 0 ||
      H * 64 != D || Nq < 0 || Nk <= 0)
    return fail(LG_E_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  LG_HIP(attn_delta(o, grad_o, D, B, H, Nq, delta_ws, st));
  LG_HIP(hipMemsetAsync(grad_q, 0, (size_t)B * Nq * D * 4, st));
  TAttn a = attn_args(q, k, v, (float*)o, (float*)lse, B, H, Nq, Nk, scale);
  a.dO = grad_o;
  a.delta = delta_ws;
  a.dQ = grad_q;
  a.dK = grad_k;
  a.dV = grad_v;
  LG_HIP(tattn_backward(a, st));
  LG_HIP(hipStreamSynchronize(st));
  return LG_OK;
}

}  // extern "C"
