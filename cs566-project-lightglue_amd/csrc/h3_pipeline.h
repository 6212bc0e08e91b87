// The LDS-DMA tile pipeline of the fp16x3 matrix kernels (gemm_h3.hip, assign_h3.hip,
// superpoint.hip): plane-image k-tiles are copied to LDS by global_load_lds_dwordx4 (common.h
// dma16), a counted s_waitcnt vmcnt(N) and a barrier follow, then the 16x16x32 mfma_h3_16 block.
//
// THE INVARIANT THE COUNTED WAIT RESTS ON
//   * vmcnt counts every vector-memory load of the wave that has not returned, in issue order:
//     the LDS-DMA copies AND every ordinary global load the compiler emits.  (Stores count too;
//     they are younger than the copies a kernel waits for, so they can only make a wait longer.)
//   * dma16 is inline asm.  The compiler's own s_waitcnt insertion neither counts it nor orders
//     LDS reads behind it: nothing but dma_wait + lds_barrier stands between a copy and the
//     fragment reads of its stage.
//   * dma_wait<N>() therefore means "all but my N youngest VMEM loads have landed".  It is right
//     only if the N youngest are exactly the copies of the stages still allowed in flight, i.e.
//     if NO compiler-issued VMEM load is placed between a stage's issue and its wait.  A load
//     scheduled in there leaves an awaited copy in flight when the LDS is read.
//   * Loads that exist before the loop today: the range exponents (gemm_h3.hip
//     range_slot_exp / range_exponent at the top of the kernel, "read here so the loads are long
//     done by the epilogue"; the same reads at the top of the sim and conv kernels).  They are
//     older than every copy, so a wait that covers a copy covers them.  Bias, row-mask or
//     statistics reads moved into the loop would break the count.
//   * The halo convolution's count PW + PH (superpoint.hip sp_conv3x3_halo_kernel) follows the
//     same rule: younger than the awaited weights W(gs) are W(gs + 1), PW copies, and at taps 1-2
//     the next halo, PH copies, and nothing else.
// A change to what the waits wait for (scheduling fences, drains) belongs here, once.
//
// The k-loop itself (prologue issue -> per k-tile: ring_wait, lds_barrier, refill, multiply ->
// final lds_barrier) is written out in each kernel from these pieces.  As one function template
// taking the kernel's issue and multiply as callables it cost registers: 14 of gemm_h3's 26
// kernels gained VGPRs (113 -> 118 on the 256 x 256 tile).  gemm_h3_kernel and sim_h3_kernel also
// keep their MFMA block in place (each says why); the halo convolution keeps its own load / mma
// split.
#pragma once

#include "common.h"

namespace lg {

// workgroup id -> tile so that each XCD (workgroups go to the 8 XCDs round-robin by id) owns a
// contiguous range of the n tiles (the tiles sharing an operand panel share one L2); bijective
// for every n.  rev: each XCD walks its range backwards.
__device__ __forceinline__ int xcd_remap(int id, int n, bool rev = false) {
  const int xcd = id & 7, local = id >> 3;
  const int base = n >> 3, extra = n & 7;
  const int cnt = base + (xcd < extra ? 1 : 0);
  return xcd * base + (xcd < extra ? xcd : extra) + (rev ? cnt - 1 - local : local);
}

// the counted wait: all but this wave's N youngest VMEM loads have landed (the invariant above)
template <int N>
__device__ __forceinline__ void dma_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS traffic of this wave done, every wave of the workgroup here, and no LDS access moved across
// by the compiler: after a dma_wait, everyone's copies have landed and everyone is done reading
// the stage about to be refilled.  SYNC = false for single-wave groups (no s_barrier).
template <bool SYNC = true>
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (SYNC) __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// One LDS stage of a BM x BN x 32 tile copied by NW waves: the four plane tiles
// [A h | A l | W h | W l], cut into 1 KiB LDS-DMA pieces, PPW per wave.
template <int BM, int BN, int NW>
struct H3Stage {
  static constexpr int APT = BM * kKB * 2;  // one A plane tile (bytes)
  static constexpr int WPT = BN * kKB * 2;  // one W plane tile
  static constexpr int STAGE_BYTES = 2 * APT + 2 * WPT;
  static constexpr int PIECES = STAGE_BYTES / 1024;
  static constexpr int PPW = PIECES / NW;
  static_assert(PIECES % NW == 0, "pieces per wave");
};

// The stage of the single-product fp16 GEMM (gemm_h3.hip, GemmH3Args.h1): the high planes only,
// [A h | W h] -- half the bytes and half the LDS-DMA pieces of H3Stage.  The pieces are dealt to the
// waves round-robin (piece q = i * NW + wave), so when NW does not divide PIECES (the LayerNorm
// tiles: 40 pieces / 16 waves, 36 / 8) the first PIECES % NW waves copy PPW pieces per k-tile and
// the others PPW - 1; each wave's counted wait uses its own count (h1_ring_wait).
template <int BM, int BN, int NW>
struct H1Stage {
  static constexpr int APT = BM * kKB * 2;  // the A high-plane tile (bytes)
  static constexpr int WPT = BN * kKB * 2;  // the W high-plane tile
  static constexpr int STAGE_BYTES = APT + WPT;
  static constexpr int PIECES = STAGE_BYTES / 1024;
  static constexpr int PPW = (PIECES + NW - 1) / NW;
  static constexpr bool EVEN = PIECES % NW == 0;
  static constexpr int FULL = EVEN ? NW : PIECES % NW;  // waves that copy PPW pieces
};

// fragment (row r, 16-byte k-chunk c) of the plane tile at byte offset t0 of a stage (the chunk
// swizzle of the plane images, common.h plane_swz)
__device__ __forceinline__ f16x8 h3_frag(const char* st, int t0, int r, int c) {
  return *reinterpret_cast<const f16x8*>(st + t0 + r * (kKB * 2) + ((c ^ plane_swz(r)) << 4));
}

// Ring of NSTAGE stages, NSTAGE - 1 k-tiles in flight, PPW copies per wave and k-tile: wait for
// this wave's copies of the oldest k-tile while `ahead` younger ones stay in flight.
template <int NSTAGE, int PPW>
__device__ __forceinline__ void ring_wait(int ahead) {
  static_assert(NSTAGE >= 2 && NSTAGE <= 4, "ring depth");
  if (NSTAGE >= 4 && ahead >= 2) dma_wait<2 * PPW>();
  else if (NSTAGE >= 3 && ahead >= 1) dma_wait<PPW>();
  else dma_wait<0>();
}

// ring_wait for an H1Stage: `wave` copies S::PPW pieces per k-tile if it is one of the first S::FULL
// waves, S::PPW - 1 otherwise (wave-uniform branch; the counts are immediates)
template <int NSTAGE, class S>
__device__ __forceinline__ void h1_ring_wait(int ahead, int wave) {
  if constexpr (S::EVEN) {
    ring_wait<NSTAGE, S::PPW>(ahead);
  } else {
    if (wave < S::FULL) ring_wait<NSTAGE, S::PPW>(ahead);
    else ring_wait<NSTAGE, S::PPW - 1>(ahead);
  }
}

// The MFMA block of one k-tile: the wave's 64 x (16 TJ) tile, rows wm0.. of A and wn0.. of W in
// the stage at st (geometry S), acc[i][j] += A_i . W_j^T as three fp16 MFMAs (common.h mfma_h3_16).
// Lane: row (lane & 15) of each 16-row block, k chunk lane >> 4 (k = 8c .. 8c+7).
template <class S, int TJ>
__device__ __forceinline__ void h3_mma_stage(const char* st, int wm0, int wn0, int lane, f32x4 (&acc)[4][TJ]) {
  const int c = lane >> 4, r16 = lane & 15;
  f16x8 ah[4], al[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wm0 + i * 16 + r16;
    ah[i] = h3_frag(st, 0, r, c);
    al[i] = h3_frag(st, S::APT, r, c);
  }
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int r = wn0 + j * 16 + r16;
    const f16x8 wh = h3_frag(st, 2 * S::APT, r, c);
    const f16x8 wl = h3_frag(st, 2 * S::APT + S::WPT, r, c);
    const f16x8 whs = wh * (_Float16)kLoScale;  // exact: |W_h| < 16
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][j] = mfma_h3_16(ah[i], al[i], whs, wl, wh, acc[i][j]);
  }
}

}  // namespace lg
