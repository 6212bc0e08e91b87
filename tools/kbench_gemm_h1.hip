// Pipeline-shape micro-benchmark of the single-product fp16 GEMM (gemm_h3.hip H1; tools only, not shipped):
// the k-loop alone (EPI_PROBE: no epilogue, so ring depths and wave tiles the epilogues' LDS buffers and
// WN == 64 rule out can still be timed) at the configs[2] row count, next to the fp16x3 k-loop and the
// complete EPI_STORE kernels of both numerics.  Operands are random (the chip's clock under load depends
// on the data).  Every variant runs in every round, so the variants alternate within the process.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-sched-strategy=max-ilp tools/kbench_gemm_h1.hip -o tools/kbench_gemm_h1
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../cs566-project-lightglue_amd/csrc/elementwise.hip"
#include "../cs566-project-lightglue_amd/csrc/gemm_h3.hip"

using namespace lg;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

__global__ void fill_kernel(float* x, size_t n, unsigned seed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned h = (unsigned)i * 2654435761u ^ (seed * 0x9E3779B9u);
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  x[i] = (float)(h >> 8) * (1.f / 8388608.f) - 1.f;  // [-1, 1)
}

struct Shape { int R, K, N; const char* name; };

template <class F>
double timed(F launch, int iters) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  launch();
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  for (int i = 0; i < iters; ++i) launch();
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  CK(hipGetLastError());
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  return ms / iters;
}

// k-loop only: the 256 x 256 tile with NS stages, wave tile 64 x WN
template <int NS, int WN, bool H1>
double probe(const GemmH3Args& a, int iters) {
  const dim3 grid(((a.R + 255) / 256) * (a.Nout / 256)), block((256 / 64) * (256 / WN) * 64);
  return timed([&] { hipLaunchKernelGGL((gemm_h3_kernel<EPI_PROBE, 256, NS, 256, WN, 1, H1>), grid, block, 0, 0, a); }, iters);
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 3, iters = 20;
  const Shape shapes[] = {{131072, 256, 768, "qkv"}, {131072, 512, 512, "ffn0"}, {131072, 512, 256, "ffn3"}};
  for (const Shape& s : shapes) {
    float *A, *W, *bias, *Y;
    _Float16 *ap, *wp, *yp;
    CK(hipMalloc(&A, (size_t)s.R * s.K * 4)); CK(hipMalloc(&W, (size_t)s.N * s.K * 4));
    CK(hipMalloc(&bias, s.N * 4)); CK(hipMalloc(&Y, (size_t)s.R * s.N * 4));
    CK(hipMalloc(&ap, (size_t)2 * s.R * s.K * 2)); CK(hipMalloc(&wp, (size_t)2 * s.N * s.K * 2));
    CK(hipMalloc(&yp, (size_t)2 * s.R * s.N * 2));
    fill_kernel<<<(unsigned)(((size_t)s.R * s.K + 255) / 256), 256>>>(A, (size_t)s.R * s.K, 1);
    fill_kernel<<<(unsigned)(((size_t)s.N * s.K + 255) / 256), 256>>>(W, (size_t)s.N * s.K, 2);
    fill_kernel<<<(s.N + 255) / 256, 256>>>(bias, s.N, 3);
    CK(split_weight_h3(W, s.N, s.K, 8.f, wp, 0));  // max|W| < 1: max|W 2^3| < 16
    RangeOut none;
    memset(&none, 0, sizeof(none));
    CK(rows_to_planes(A, s.R, s.K, s.K, ap, s.R, 0, none, 0));
    CK(hipDeviceSynchronize());
    GemmH3Args a;
    memset(&a, 0, sizeof(a));
    a.A0 = {ap, (long long)s.R * s.K, s.R}; a.K0 = s.K; a.K = s.K;
    a.W = {wp, (long long)s.N * s.K, s.N}; a.R = s.R; a.Nout = s.N;
    a.out_scale = 1.f; a.bias = bias; a.Y = Y; a.ldy = s.N;
    a.Yp = yp; a.yps = (long long)s.R * s.N; a.yrows_pad = s.R;
    a.a0_slot = a.a1_slot = -1;
    a.stream = (size_t)s.R * s.K * 4 >= ((size_t)128 << 20);  // what gemm_h3 sets for the production launches
    const double fl = 2.0 * s.R * s.K * s.N;
    for (int r = 0; r < rounds; ++r) {
      auto rep = [&](const char* name, double ms) {
        printf("round %d %-5s %-44s %8.1f us %7.1f TF/s\n", r, s.name, name, ms * 1e3, fl / ms / 1e9);
      };
      GemmH3Args h3 = a, h1 = a;
      h3.acc_scale = ldexpf(1.f, -(11 + 3));
      h1.acc_scale = ldexpf(1.f, -3); h1.h1 = 1;
      rep("fp16x3 k-loop, 2 stages, 64 x 64 waves", probe<2, 64, false>(h3, iters));
      rep("H1 k-loop, 2 stages, 64 x 64 waves", probe<2, 64, true>(h1, iters));
      rep("H1 k-loop, 3 stages, 64 x 64 waves", probe<3, 64, true>(h1, iters));
      rep("H1 k-loop, 4 stages, 64 x 64 waves", probe<4, 64, true>(h1, iters));
      rep("H1 k-loop, 2 stages, 64 x 128 waves", probe<2, 128, true>(h1, iters));
      rep("H1 k-loop, 4 stages, 64 x 128 waves", probe<4, 128, true>(h1, iters));
      rep("fp16x3 fp32 + planes out (production)", timed([&] { CK(gemm_h3(h3, EPI_STORE, 0)); }, iters));
      rep("H1 fp32 + planes out (production)", timed([&] { CK(gemm_h3(h1, EPI_STORE, 0)); }, iters));
    }
    CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(bias)); CK(hipFree(Y)); CK(hipFree(ap)); CK(hipFree(wp)); CK(hipFree(yp));
  }
  return 0;
}
