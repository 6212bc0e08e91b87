// C-ABI of the kernel-level assignment entry (include/lightglue_mi355x.h: lg_assign): the dual-softmax
// assignment and the mutual filter alone, on plain fp32 tensors, over either route of the forward:
//   materialised  sim = md0 md1^T by the bf16x6 gemm_x6 (or the caller's sim), then assign_and_filter:
//                 what lg_assignment_head and the pruned forward run
//   recomputed    md written as the two-plane image the forward's final_proj epilogue produces
//                 (rows_to_planes2, one range slot, lshift = 11, rows_pad = B (M + N) rounded up to 256
//                 plus 256), then assign_and_filter_h3: the default eval route.  The forward chooses the
//                 image's exponent from a bound PREDICTED from the weights (|Wf|_1 M[x] + max|bf|); here
//                 the maximum is MEASURED (range_absmax2 over md0 and md1), so the exponent is the
//                 smallest one that holds these values -- never larger than the forward's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/lightglue_mi355x.h"
#include "api_common.h"
#include "kernels.h"

#include "common.h"

namespace {
using namespace lg;

constexpr int kD = 256;
constexpr int kSlots = 2;  // 0: max|md|; 1: the image's exponent

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

struct Layout {
  int rows_pad;
  size_t rtab, cnt, planes, sim, aws, bytes;
};
Layout carve(int B, int M, int N) {
  Layout L;
  const size_t R = (size_t)B * (M + N);
  L.rows_pad = (int)((R + 255) / 256 * 256 + 256);
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += align256(n);
    return o;
  };
  L.rtab = take((size_t)kSlots * kRangeStride * sizeof(unsigned));
  L.cnt = take((size_t)2 * B * sizeof(int));
  L.planes = take((size_t)2 * L.rows_pad * kD * 2);
  L.sim = take((size_t)B * M * N * 4);
  L.aws = take((assign_workspace_floats(B, M, N) + 64 + sim_h3_workspace_floats(B, M, N)) * 4);
  L.bytes = off;
  return L;
}

const char* shape_error(int64_t B, int64_t M, int64_t N) {
  if (B <= 0 || M <= 0 || N <= 0) return "B, M and N must be positive";
  if (B * (M + 1) * (N + 1) >= (int64_t(1) << 31) || B * (M + N) > (1 << 22)) return "shape too large for the kernel-level entry";
  return nullptr;
}

bool off16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

const char* args_error(const lg_assign_args_t& a) {
  if (const char* e = shape_error(a.B, a.M, a.N)) return e;
  if (a.route != LG_ASSIGN_MATERIALISED && a.route != LG_ASSIGN_RECOMPUTED) return "bad route";
  if (!a.z0 || !a.z1 || !a.m0 || !a.m1 || !a.s0 || !a.s1) return "null z0 / z1 / m0 / m1 / s0 / s1";
  if ((a.Mb == nullptr) != (a.Nb == nullptr)) return "Mb and Nb come together";
  if (a.fixed && !a.Mb) return "fixed without counts";
  if (a.raw_counts && (!a.Mb || a.route != LG_ASSIGN_MATERIALISED)) return "raw_counts: the counted materialised route only";
  if (a.route == LG_ASSIGN_RECOMPUTED) {
    if (a.sim) return "the recomputed route takes no sim";
    if (!a.md0 || !a.md1) return "null md0 / md1";
    if (a.M % 16 || a.N % 16) return "the recomputed route needs M % 16 == 0 and N % 16 == 0";
    if (a.Mb && !a.fixed) return "the recomputed route takes counts only in the fixed layout";
  } else if (!a.sim && (!a.md0 || !a.md1)) {
    return "null md0 / md1 without sim";
  }
  if (off16(a.md0) || off16(a.md1) || off16(a.sim)) return "a pointer is not 16-byte aligned";
  return nullptr;
}

// the forward's contract (elementwise.hip prune_init_counts_kernel): counts clamped to the capacities,
// an empty side empties the pair.  raw: clamped only -- what width pruning can leave behind
__global__ void assign_counts_kernel(const int* Mb, const int* Nb, int B, int M, int N, int raw, int* cnt) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B) return;
  int a = min(max(Mb[t], 0), M), b = min(max(Nb[t], 0), N);
  if (!raw && (a == 0 || b == 0)) a = b = 0;
  cnt[t] = a;
  cnt[B + t] = b;
}

// fp16 bit patterns no arithmetic survives: quiet NaNs and infinities of both signs
__device__ __forceinline__ unsigned short poison_bits(size_t i) {
  const unsigned short p[4] = {0x7E00, 0x7C00, 0xFE00, 0xFC00};
  return p[(i * 2654435761u >> 13) & 3];
}

// rows of the md plane image that hold no live keypoint: the padding rows [R, rows_pad) and, with
// counts, rows >= cnt of every (image, pair) slot; both planes
__global__ void assign_poison_rows_kernel(unsigned short* planes, long long ps, int rows_pad, int B, int M, int N,
                                          const int* cnt) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows_pad * kD) return;
  const int r = (int)(i / kD), k = (int)(i % kD);
  if (r < B * (M + N)) {
    if (!cnt) return;
    int local;
    const int s = seg_of_row(SegLayout{B, M, N}, r, local);
    if (local < cnt[s]) return;
  }
  const size_t off = plane_off(r, k, rows_pad);
  planes[off] = poison_bits(i);
  planes[ps + off] = poison_bits(i + 977);
}

// entries of a materialised similarity outside pair b's [Mb][Nb] block
__global__ void assign_poison_sim_kernel(float* sim, int B, int M, int N, const int* cnt) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * M * N) return;
  const int b = (int)(i / ((size_t)M * N));
  const int rem = (int)(i - (size_t)b * M * N);
  if (rem / N < cnt[b] && rem % N < cnt[B + b]) return;
  sim[i] = (i & 1) ? NAN : ((i & 2) ? INFINITY : -INFINITY);
}

__global__ void assign_fill_f32_kernel(float* p, float v, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

hipError_t fill_f32(float* p, float v, size_t n, hipStream_t st) {
  if (!p || n == 0) return hipSuccess;
  hipLaunchKernelGGL(assign_fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, v, n);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int lg_assign_workspace_bytes(int32_t B, int32_t M, int32_t N, size_t* bytes) {
  if (!bytes) return fail(LG_E_INVALID, "null argument");
  if (const char* e = shape_error(B, M, N)) return fail(LG_E_INVALID, e);
  *bytes = carve(B, M, N).bytes;
  return LG_OK;
}

int lg_assign(lg_assign_args_t* args, void* workspace, size_t workspace_bytes, void* stream) {
  if (!args) return fail(LG_E_INVALID, "null argument");
  lg_assign_args_t& a = *args;
  if (const char* e = args_error(a)) return fail(LG_E_INVALID, e);
  const int B = a.B, M = a.M, N = a.N;
  const Layout L = carve(B, M, N);
  if (!workspace || workspace_bytes < L.bytes) return fail(LG_E_WORKSPACE, "workspace too small (lg_assign_workspace_bytes)");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(LG_E_INVALID, "workspace is not 256-byte aligned");
  a.exp_md = 0;
  a.max_md = 0.f;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned* rtab = reinterpret_cast<unsigned*>(ws + L.rtab);
  int* cnt = reinterpret_cast<int*>(ws + L.cnt);
  _Float16* planes = reinterpret_cast<_Float16*>(ws + L.planes);
  float* simbuf = reinterpret_cast<float*>(ws + L.sim);
  const long long ps = (long long)L.rows_pad * kD;

  if (a.Mb) {
    hipLaunchKernelGGL(assign_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, st, a.Mb, a.Nb, B, M, N, a.raw_counts, cnt);
    LG_HIP(hipGetLastError());
  }
  if (a.poison) {
    LG_HIP(fill_f32(a.la, LG_ASSIGN_SENTINEL_F, (size_t)B * (M + 1) * (N + 1), st));
    LG_HIP(fill_f32(a.s0, LG_ASSIGN_SENTINEL_F, (size_t)B * M, st));
    LG_HIP(fill_f32(a.s1, LG_ASSIGN_SENTINEL_F, (size_t)B * N, st));
    LG_HIP(fill_i64(a.m0, LG_ASSIGN_SENTINEL_I, (size_t)B * M, st));
    LG_HIP(fill_i64(a.m1, LG_ASSIGN_SENTINEL_I, (size_t)B * N, st));
  }

  AssignArgs aa;
  memset(&aa, 0, sizeof(aa));
  aa.z0 = a.z0; aa.z1 = a.z1; aa.la = a.la; aa.ws = reinterpret_cast<float*>(ws + L.aws);
  aa.B = B; aa.M = M; aa.N = N; aa.th = a.threshold;
  aa.m0 = a.m0; aa.m1 = a.m1; aa.s0 = a.s0; aa.s1 = a.s1;
  if (a.Mb) {
    aa.Mb = cnt;
    aa.Nb = cnt + B;
    aa.fixed = a.fixed ? 1 : 0;
  }

  if (a.route == LG_ASSIGN_RECOMPUTED) {
    LG_HIP(hipMemsetAsync(rtab, 0, (size_t)kSlots * kRangeStride * sizeof(unsigned), st));
    LG_HIP(hipMemsetAsync(planes, 0, (size_t)2 * L.rows_pad * kD * 2, st));
    LG_HIP(range_absmax2(a.md0, (size_t)B * M * kD, a.md1, (size_t)B * N * kD, rtab, 0, st));
    // the final_proj epilogue's RangeOut (lightglue_api.cpp: track 0, lshift 11), its bound measured
    LG_HIP(rows_to_planes2(a.md0, B * M, a.md1, B * N, kD, kD, planes, L.rows_pad, 0,
                           RangeOut{rtab, 0, -1, 1.f, 0.f, 0.f, 1, 0, 11}, st));
    if (a.poison) {
      const size_t n = (size_t)L.rows_pad * kD;
      hipLaunchKernelGGL(assign_poison_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                         reinterpret_cast<unsigned short*>(planes), ps, L.rows_pad, B, M, N, a.Mb ? cnt : nullptr);
      LG_HIP(hipGetLastError());
    }
    const hipError_t e = assign_and_filter_h3(aa, PlaneRef{planes, ps, L.rows_pad}, rtab, 1, st);
    if (e == hipErrorInvalidValue) return fail(LG_E_INVALID, "assign_and_filter_h3 takes no such operands (LG_ASSIGN_SIM_X6 set?)");
    LG_HIP(e);
    unsigned htab[kSlots * kRangeStride];
    LG_HIP(hipMemcpyAsync(htab, rtab, sizeof(htab), hipMemcpyDeviceToHost, st));
    LG_HIP(hipStreamSynchronize(st));
    a.exp_md = (int)htab[kRangeStride + kRangeShards];
    for (int i = 0; i < kRangeShards; ++i) {
      float v;
      memcpy(&v, htab + i, 4);
      a.max_md = std::fmax(a.max_md, v);
    }
    return LG_OK;
  }

  if (a.sim) {
    aa.sim = a.sim;
  } else {
    // sim = md0 md1^T per pair over the capacities: lg_assignment_head's and the pruned forward's GEMM
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.out_scale = 1.f;
    g.A0 = a.md0; g.lda0 = kD; g.K0 = kD; g.K = kD; g.sA = (long long)M * kD;
    g.W = a.md1; g.ldw = kD; g.sW = (long long)N * kD;
    g.R = M; g.Nout = N; g.Y = simbuf; g.ldy = N; g.sY = (long long)M * N;
    LG_HIP(gemm_x6(g, EPI_STORE, B, st));
    if (a.poison && a.Mb) {
      const size_t n = (size_t)B * M * N;
      hipLaunchKernelGGL(assign_poison_sim_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, simbuf, B, M, N, cnt);
      LG_HIP(hipGetLastError());
    }
    aa.sim = simbuf;
  }
  LG_HIP(assign_and_filter(aa, st));
  LG_HIP(hipStreamSynchronize(st));
  return LG_OK;
}

}  // extern "C"
