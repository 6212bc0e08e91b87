// Line ground truth from a homography on the device: gt_line_matches_from_homography (reference
// gluefactory/geometry/gt_generation.py:409-558 over sample_pts :160-170, torch_perp_dist :173-204 and
// warp_points_torch, geometry/homography.py:161-180) without any [B, n0, n1, npts] intermediate and
// without the host: the reference copies the [B, n0, n1] cost to the host and runs SciPy's
// linear_sum_assignment per pair; here the same algorithm runs one pair per wave.
//
// Stage A (counts)
//   gl_prepare   one thread per line of either image: clamp the endpoints to the image, the segment
//                in the form the distance test reads it (second endpoint, unit direction, fp16-rounded
//                length), the npts samples warped into the other image ([B, n, npts, 2], the largest
//                thing kept), and the line's out-of-image flag from an integer count threshold
//   gl_counts    a workgroup owns a 16 x 16 tile of (i, j); the warped samples of its 16 lines of
//                either image are staged in LDS (an odd row stride in 8-byte units: the 16 lines a wave
//                reads at once fall in 16 different bank pairs) and thread (i, j) counts how many of
//                line j's samples are close to segment i of image 0, and how many of line i's are close
//                to segment j of image 1.  VALU work; two byte stores per entry.
// Stage B (labels)
//   gl_flags     unmatched0/1 (no mask_close entry in the row / column, or out of the image), the
//                rows / columns the cost blocks (unmatched or invalid) and the default labels
//   gl_cost      the fp64 cost -cnt0 * cnt1t with 1e6 on blocked rows and columns, stored so that the
//                solver's rows are the shorter side
//   lsa_solve    SciPy's rectangular_lsap (shortest augmenting paths, Crouse's variant) with its scan
//                order and its tie rule, one wave per pair, state in LDS (global memory for sides too
//                long for 64 KiB); also what lg_linear_sum_assignment runs
//   gl_pairs     the ones of `positive` and the matched labels from the assignment
//
// The pose-and-depth variant, gt_line_matches_from_pose_depth (:207-406), shares everything but the
// front end and the thresholds:
//   gld_prepare  one wave per line of either image, the lanes over its samples: clamp to the depth map,
//                the segment record, per sample the depth (sample_depth) and the projection into the
//                other camera (gt_depth_common.h, the chain of gtd_points), the counts of visible
//                samples, of samples with valid depth and of samples outside the other image by wave
//                ballots, and the projected samples with NaN coordinates where a sample is not visible:
//                close_pt is false for a NaN, so gl_counts runs unchanged and `close * visible` needs
//                no second input
//   gl_flags / gl_pairs<PerLineMin>  mask_close with a minimum count per row and per column, looked up
//                from the line's visible count (:329-336), out_of only in unmatched0/1 (:341-342), and
//                the depth-ignore flag or-ed into the ignored lines (:345-352)
//
// The "close" test follows the reference's CPU path in fp32.  Its CUDA branch casts the rotation and
// the centred samples to fp16 "to reduce memory"; that is not reproduced (the fixtures come from the
// CPU path).  This TU is built with -ffp-contract=off (Makefile): every product and sum is rounded on
// its own, as the reference's separate torch passes do.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "gt_common.h"
#include "gt_depth_common.h"
#include "kernels.h"

namespace lg {
namespace {

using namespace gt;

constexpr int kTile = 16;  // gl_counts: lines of either image per workgroup

// ---------------------------------------------------------------------------------------------
// Stage A

// per line: seg [8] = (x2, y2, nx, ny, size, -, -, -): torch_perp_dist's second endpoint, dir / size
// and size = ||dir|| rounded to fp16 (:177-179); a zero-length segment has nx = ny = NaN and every
// comparison of the test is then false, as in the reference
__global__ __launch_bounds__(256) void gl_prepare(const float* __restrict__ lines0, const float* __restrict__ lines1,
                                                  const float* __restrict__ H, int B, int n0, int n1, int w0, int h0,
                                                  int w1, int h1, int npts, int vis_min, float* __restrict__ seg0,
                                                  float* __restrict__ seg1, float* __restrict__ pts01,
                                                  float* __restrict__ pts10, uint8_t* __restrict__ out_of0,
                                                  uint8_t* __restrict__ out_of1) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t na = (size_t)B * n0, nb = (size_t)B * n1;
  if (t >= na + nb) return;
  const bool second = t >= na;
  const size_t l = second ? t - na : t;  // flat line index of its side
  const size_t b = l / (second ? n1 : n0);
  const float* ln = (second ? lines1 : lines0) + l * 4;
  // own image: the clamp (:441-448); other image: the out-of-image test (:461-470)
  const float wc = (float)((second ? w1 : w0) - 1), hc = (float)((second ? h1 : h0) - 1);
  const float wo = (float)(second ? w0 : w1), ho = (float)(second ? h0 : h1);
  float h[9], hm[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = H[b * 9 + k];
  if (second) {
    invert_h(h, hm);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) hm[k] = h[k];
  }
  const float x1 = fminf(fmaxf(ln[0], 0.f), wc), y1 = fminf(fmaxf(ln[1], 0.f), hc);
  const float x2 = fminf(fmaxf(ln[2], 0.f), wc), y2 = fminf(fmaxf(ln[3], 0.f), hc);
  const float dx = x2 - x1, dy = y2 - y1;
  const float size = __half2float(__float2half_rn(sqrtf(dx * dx + dy * dy)));
  float* sg = (second ? seg1 : seg0) + l * 8;
  *reinterpret_cast<float4*>(sg) = make_float4(x2, y2, dx / size, dy / size);
  *reinterpret_cast<float4*>(sg + 4) = make_float4(size, 0.f, 0.f, 0.f);
  // sample_pts (:165-168): dir = (end - start) / (npts - 1), pt_k = start + dir * k
  const float den = (float)(npts - 1);
  const float ddx = dx / den, ddy = dy / den;
  float2* out = reinterpret_cast<float2*>(second ? pts10 : pts01) + l * (size_t)npts;
  int nout = 0;
  for (int k = 0; k < npts; ++k) {
    const float fk = (float)k;
    const float px = x1 + ddx * fk, py = y1 + ddy * fk;
    const float2 q = warp(hm, px, py);
    out[k] = q;
    nout += (q.x < 0.f || q.y < 0.f || q.x >= wo || q.y >= ho) ? 1 : 0;
  }
  // lines of image 1 leave image 0 (out_of0 [B, n1]) and the other way round
  (second ? out_of0 : out_of1)[l] = nout >= vis_min;
}

struct LineDepthArgs {
  const float *lines0, *lines1, *depth0, *depth1, *cam0, *cam1, *T01, *T10;
  int B, n0, n1, H0, W0, H1, W1, ih0, iw0, ih1, iw1, nd, npts;
  int out_min, valid_min;  // gt_line_count_threshold_visibility / _valid_depth
  float *seg0, *seg1, *pts01, *pts10;
  uint8_t *out_of0, *out_of1, *ignd0, *ignd1, *nvis0, *nvis1;
};

// One wave per line; lane k takes samples k, k + 64, ...: the four depth taps of neighbouring samples
// fall in the same or adjacent cache lines, and a line's npts serial gather chains become
// ceil(npts / 64).  The clamp is to the depth map (:250-260), the out-of-image test uses the image
// size (:290-302) and runs on the projected coordinates before they are masked.
__global__ __launch_bounds__(256) void gld_prepare(LineDepthArgs a) {
  const size_t t = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const size_t na = (size_t)a.B * a.n0, nb = (size_t)a.B * a.n1;
  if (t >= na + nb) return;  // the whole wave
  const bool second = t >= na;
  const size_t l = second ? t - na : t;  // flat line index of its side
  const size_t b = l / (second ? a.n1 : a.n0);
  const float* ln = (second ? a.lines1 : a.lines0) + l * 4;
  const int Hi = second ? a.H1 : a.H0, Wi = second ? a.W1 : a.W0;
  const float wc = (float)(Wi - 1), hc = (float)(Hi - 1);
  const float wo = (float)(second ? a.iw0 : a.iw1), ho = (float)(second ? a.ih0 : a.ih1);
  const int cw = 6 + a.nd;
  const Cam ci = load_cam((second ? a.cam1 : a.cam0) + b * cw, a.nd);  // the line's own camera
  const Cam cj = load_cam((second ? a.cam0 : a.cam1) + b * cw, a.nd);  // the one it is projected into
  const PoseRt T = load_pose((second ? a.T10 : a.T01) + b * 12);
  const float* map = (second ? a.depth1 : a.depth0) + b * (size_t)Hi * Wi;

  const float x1 = fminf(fmaxf(ln[0], 0.f), wc), y1 = fminf(fmaxf(ln[1], 0.f), hc);
  const float x2 = fminf(fmaxf(ln[2], 0.f), wc), y2 = fminf(fmaxf(ln[3], 0.f), hc);
  const float dx = x2 - x1, dy = y2 - y1;
  if (lane == 0) {
    const float size = __half2float(__float2half_rn(sqrtf(dx * dx + dy * dy)));
    float* sg = (second ? a.seg1 : a.seg0) + l * 8;
    *reinterpret_cast<float4*>(sg) = make_float4(x2, y2, dx / size, dy / size);
    *reinterpret_cast<float4*>(sg + 4) = make_float4(size, 0.f, 0.f, 0.f);
  }
  const float den = (float)(a.npts - 1);
  const float ddx = dx / den, ddy = dy / den;
  float2* out = reinterpret_cast<float2*>(second ? a.pts10 : a.pts01) + l * (size_t)a.npts;
  int nvis = 0, nvalid = 0, nout = 0;
  for (int k0 = 0; k0 < a.npts; k0 += 64) {
    const int k = k0 + lane;
    bool vis = false, valid = false, outside = false;
    if (k < a.npts) {
      const float fk = (float)k;
      const float px = x1 + ddx * fk, py = y1 + ddy * fk;
      const float d = sample_depth(map, Hi, Wi, px, py);
      valid = depth_valid(d);
      const P2 q = project_to(ci, cj, a.nd, T, px, py, d);  // NaN without depth
      vis = valid && q.ok;
      outside = q.x < 0.f || q.y < 0.f || q.x >= wo || q.y >= ho;  // false for NaN, as :293-302
      const float nan = __builtin_nanf("");
      out[k] = vis ? make_float2(q.x, q.y) : make_float2(nan, nan);
    }
    nvis += __popcll(__ballot(vis));
    nvalid += __popcll(__ballot(valid));
    nout += __popcll(__ballot(outside));
  }
  if (lane == 0) {
    // lines of image 1 leave image 0 (out_of0 [B, n1]) and the other way round
    (second ? a.out_of0 : a.out_of1)[l] = nout >= a.out_min;
    (second ? a.ignd1 : a.ignd0)[l] = nvalid < a.valid_min;
    (second ? a.nvis1 : a.nvis0)[l] = (uint8_t)nvis;
  }
}

// (perp_dist < dist_th) & overlaping of torch_perp_dist for one sample
__device__ __forceinline__ int close_pt(float4 s, float size, float2 p, float dth) {
  const float cx = p.x - s.x, cy = p.y - s.y;
  const float rx = s.z * cx + s.w * cy;
  const float ry = (-s.w) * cx + s.z * cy;
  return (fabsf(ry) < dth && rx <= 0.f && fabsf(rx) <= size) ? 1 : 0;
}

__global__ __launch_bounds__(kTile* kTile) void gl_counts(const float* __restrict__ seg0, const float* __restrict__ seg1,
                                                          const float* __restrict__ pts01, const float* __restrict__ pts10,
                                                          int n0, int n1, int ti_n, int tj_n, int npts, int stride,
                                                          float dth, uint8_t* __restrict__ cnt0,
                                                          uint8_t* __restrict__ cnt1t) {
  extern __shared__ float2 smem[];
  float2* sI = smem;                   // warped samples of kTile lines of image 0 (in image 1)
  float2* sJ = smem + kTile * stride;  // warped samples of kTile lines of image 1 (in image 0)
  unsigned blk = blockIdx.x;
  const unsigned tj_b = blk % tj_n;
  blk /= tj_n;
  const unsigned ti_b = blk % ti_n;
  const size_t b = blk / ti_n;
  const int i0 = ti_b * kTile, j0 = tj_b * kTile;
  const float2* gI = reinterpret_cast<const float2*>(pts01) + (b * n0 + i0) * (size_t)npts;
  const float2* gJ = reinterpret_cast<const float2*>(pts10) + (b * n1 + j0) * (size_t)npts;
  const int li = min(kTile, n0 - i0), lj = min(kTile, n1 - j0);
  for (int e = threadIdx.x; e < kTile * npts; e += kTile * kTile) {
    const int l = e / npts, k = e - l * npts;
    if (l < li) sI[l * stride + k] = gI[e];
    if (l < lj) sJ[l * stride + k] = gJ[e];
  }
  __syncthreads();
  const int ti = threadIdx.x / kTile, tj = threadIdx.x % kTile;
  if (ti >= li || tj >= lj) return;
  const size_t i = b * n0 + i0 + ti, j = b * n1 + j0 + tj;
  const float4 a = *reinterpret_cast<const float4*>(seg0 + i * 8);
  const float asz = seg0[i * 8 + 4];
  const float4 c = *reinterpret_cast<const float4*>(seg1 + j * 8);
  const float csz = seg1[j * 8 + 4];
  const float2* pj = sJ + tj * stride;
  const float2* pi = sI + ti * stride;
  int c0 = 0, c1 = 0;
#pragma unroll 2
  for (int k = 0; k < npts; ++k) {
    c0 += close_pt(a, asz, pj[k], dth);
    c1 += close_pt(c, csz, pi[k], dth);
  }
  const size_t o = i * n1 + j0 + tj;
  cnt0[o] = (uint8_t)c0;
  cnt1t[o] = (uint8_t)c1;
}

// ---------------------------------------------------------------------------------------------
// Stage B

// What differs between the two variants of stage B, as a policy of gl_flags and gl_pairs.
// OneMin (homography, :491-500): one minimum count for every entry, out_of part of mask_close, only
// invalid lines ignored.
struct OneMin {
  static constexpr bool kOutOfInMask = true;
  int ov_min;
  __device__ __forceinline__ int row_min(size_t) const { return ov_min; }
  __device__ __forceinline__ int col_min(size_t) const { return ov_min; }
  __device__ __forceinline__ bool ignored_row(size_t) const { return false; }
  __device__ __forceinline__ bool ignored_col(size_t) const { return false; }
};
// PerLineMin (pose and depth, :329-352): cnt1t[i, j] against the minimum for the visible count of line
// i, cnt0[i, j] against that of line j; out_of only in unmatched0/1; a line without enough valid depth
// is ignored like an invalid one.  min_close[v] for v past npts is npts + 1: nothing passes.
struct CloseTable {
  uint16_t min_close[256];
};
struct PerLineMin {
  static constexpr bool kOutOfInMask = false;
  const uint8_t *nvis0, *nvis1, *ignd0, *ignd1;
  CloseTable tab;
  __device__ __forceinline__ int row_min(size_t row) const { return tab.min_close[nvis0[row]]; }
  __device__ __forceinline__ int col_min(size_t col) const { return tab.min_close[nvis1[col]]; }
  __device__ __forceinline__ bool ignored_row(size_t row) const { return ignd0[row] != 0; }
  __device__ __forceinline__ bool ignored_col(size_t col) const { return ignd1[col] != 0; }
};

// Blocks [0, rb): one wave per row of a pair, the lanes stride its columns.  The rest: one thread per
// column, walking the rows (adjacent threads read adjacent bytes).  mask_close is cnt1t >= the row's
// minimum and cnt0 >= the column's (and, OneMin, neither line out of the image); unmatched = no
// mask_close entry, or out of the image; dead = unmatched | ignored, what the cost and `positive` block.
template <class Min>
__global__ __launch_bounds__(256) void gl_flags(const uint8_t* __restrict__ cnt0, const uint8_t* __restrict__ cnt1t,
                                                const uint8_t* __restrict__ out_of0, const uint8_t* __restrict__ out_of1,
                                                const uint8_t* __restrict__ valid0, const uint8_t* __restrict__ valid1,
                                                int B, int n0, int n1, Min mn, unsigned rb,
                                                uint8_t* __restrict__ dead0, uint8_t* __restrict__ dead1,
                                                int64_t* __restrict__ m0, int64_t* __restrict__ m1) {
  if (blockIdx.x < rb) {
    const size_t row = (size_t)blockIdx.x * 4 + threadIdx.x / 64;  // flat (b, i)
    if (row >= (size_t)B * n0) return;
    const size_t b = row / n0;
    const int lane = threadIdx.x & 63;
    const bool out_i = out_of1[row] != 0;
    const int min_i = mn.row_min(row);
    int any = 0;
    if (!(Min::kOutOfInMask && out_i))
      for (int j = lane; j < n1; j += 64) {
        const size_t o = row * n1 + j, col = b * n1 + j;
        any |= (cnt0[o] >= mn.col_min(col) && cnt1t[o] >= min_i && !(Min::kOutOfInMask && out_of0[col])) ? 1 : 0;
      }
    any = __any(any);
    if (lane == 0) {
      const bool ign = valid0[row] == 0 || mn.ignored_row(row);
      dead0[row] = (!any || out_i || ign) ? 1 : 0;
      m0[row] = ign ? -2 : -1;
    }
  } else {
    const size_t col = (size_t)(blockIdx.x - rb) * 256 + threadIdx.x;  // flat (b, j)
    if (col >= (size_t)B * n1) return;
    const size_t b = col / n1;
    const int j = (int)(col - b * n1);
    const bool out_j = out_of0[col] != 0;
    const int min_j = mn.col_min(col);
    int any = 0;
    if (!(Min::kOutOfInMask && out_j))
      for (int i = 0; i < n0; ++i) {
        const size_t row = b * n0 + i, o = row * n1 + j;
        any |= (cnt0[o] >= min_j && cnt1t[o] >= mn.row_min(row) && !(Min::kOutOfInMask && out_of1[row])) ? 1 : 0;
      }
    const bool ign = valid1[col] == 0 || mn.ignored_col(col);
    dead1[col] = (!any || out_j || ign) ? 1 : 0;
    m1[col] = ign ? -2 : -1;
  }
}

// cost = -(cnt0 * cnt1t), 1e6 on dead rows, then on dead columns (:506-513); the values are the
// reference's int64 matrix.  tr: stored transposed ([n1, n0]) so that the solver's rows are the
// shorter side.
__global__ __launch_bounds__(256) void gl_cost(const uint8_t* __restrict__ cnt0, const uint8_t* __restrict__ cnt1t,
                                               const uint8_t* __restrict__ dead0, const uint8_t* __restrict__ dead1,
                                               size_t total, int n0, int n1, bool tr, double* __restrict__ cost) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t row = t / n1;  // flat (b, i)
  const int j = (int)(t - row * n1);
  const size_t b = row / n0;
  const int i = (int)(row - b * n0);
  const bool dead = dead0[row] || dead1[b * n1 + j];
  const double v = dead ? 1e6 : -(double)((int)cnt0[t] * (int)cnt1t[t]);
  cost[tr ? (b * n1 + j) * n0 + i : t] = v;
}

template <class Min>
__global__ __launch_bounds__(256) void gl_pairs(const uint8_t* __restrict__ cnt0, const uint8_t* __restrict__ cnt1t,
                                                const uint8_t* __restrict__ dead0, const uint8_t* __restrict__ dead1,
                                                const int64_t* __restrict__ row_ind, const int64_t* __restrict__ col_ind,
                                                int B, int n0, int n1, int nmin, Min mn,
                                                uint8_t* __restrict__ positive, int64_t* __restrict__ m0,
                                                int64_t* __restrict__ m1) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)B * nmin) return;
  const size_t b = t / nmin;
  const int64_t i = row_ind[t], j = col_ind[t];
  if (i < 0 || j < 0 || i >= n0 || j >= n1) return;  // an infeasible cost leaves no assignment
  const size_t o = (b * n0 + i) * n1 + j;
  // positive & mask_close with the unmatched / ignored rows and columns removed (:539-546); a row
  // without a positive stays -1, an ignored one -2 (:547-552), which gl_flags already wrote
  if (cnt0[o] >= mn.col_min(b * n1 + j) && cnt1t[o] >= mn.row_min(b * n0 + i) && !dead0[b * n0 + i] && !dead1[b * n1 + j]) {
    positive[o] = 1;
    m0[b * n0 + i] = j;
    m1[b * n1 + j] = i;
  }
}

// ---------------------------------------------------------------------------------------------
// The assignment solver: SciPy's rectangular_lsap, one pair per wave.
//
// The serial algorithm: rows 0..nr-1 in order; each row searches a shortest augmenting path by steps.
// A step scans the remaining columns in slot order it = 0..num_remaining-1, relaxes
// shortest[j] / path[j] on strict <, and picks the column with the least shortest[j]; among equal ones
// the last unassigned column of the scan if there is one, else the first.  Stated as a reduction over
// (value, key): the least value, then the largest key, with key = it + 2^30 for an unassigned column
// and -it for an assigned one.  Here the lanes take the slots strided by 64 and a butterfly reduces
// (value, key); the order of the relaxations does not matter (each touches its own column).
//
// Instead of the SR / SC flags: the picked slot is swapped with the last live one, not merely
// overwritten, so remaining[num_remaining..nc) lists the visited columns (the algorithm never reads
// past num_remaining), and the visited rows other than the current one are row4col of those columns.
//
// One wave is the whole workgroup: __syncthreads() orders the wave's LDS / global accesses between the
// phases and costs no workgroup barrier.

struct LsaState {
  double *shortest, *v, *u;
  int *remaining, *path, *row4col, *col4row;
};

__host__ __device__ inline size_t lsa_state_bytes(int nr, int nc) {
  return 8 * (2 * (size_t)nc + nr) + 4 * (3 * (size_t)nc + nr);
}

__device__ __forceinline__ LsaState lsa_carve(char* base, int nr, int nc) {
  LsaState s;
  s.shortest = reinterpret_cast<double*>(base);
  s.v = s.shortest + nc;
  s.u = s.v + nc;
  s.remaining = reinterpret_cast<int*>(s.u + nr);
  s.path = s.remaining + nc;
  s.row4col = s.path + nc;
  s.col4row = s.row4col + nc;
  return s;
}

constexpr int kUnassigned = 1 << 30;

// nr <= nc: the working matrix, entry (i, j) at cost[i * rs + j * cs].  tr: the working matrix is the
// transpose of the caller's; the pairs come out sorted by the caller's row index.
template <bool kLds>
__global__ __launch_bounds__(64) void lsa_solve(const double* __restrict__ cost, size_t pair_stride, int nr, int nc,
                                                size_t rs, size_t cs, bool tr, int64_t* __restrict__ row_ind,
                                                int64_t* __restrict__ col_ind, char* __restrict__ gstate,
                                                size_t state_stride) {
  extern __shared__ double lsa_smem[];
  const int lane = threadIdx.x;
  const size_t b = blockIdx.x;
  const LsaState s = lsa_carve(kLds ? reinterpret_cast<char*>(lsa_smem) : gstate + b * state_stride, nr, nc);
  const double* c = cost + b * pair_stride;
  int64_t* ri = row_ind + b * nr;
  int64_t* ci = col_ind + b * nr;
  const double inf = __builtin_inf();

  for (int j = lane; j < nc; j += 64) {
    s.v[j] = 0.0;
    s.row4col[j] = -1;
  }
  for (int i = lane; i < nr; i += 64) {
    s.u[i] = 0.0;
    s.col4row[i] = -1;
  }
  bool feasible = true;
  for (int cur = 0; cur < nr && feasible; ++cur) {
    // filled in reverse, as SciPy does (a constant matrix then solves to the identity)
    for (int it = lane; it < nc; it += 64) {
      s.remaining[it] = nc - 1 - it;
      s.shortest[it] = inf;
    }
    __syncthreads();
    int nrem = nc, i = cur, sink = -1;
    double min_val = 0.0;
    while (sink == -1) {
      const double ui = s.u[i];
      const double* crow = c + (size_t)i * rs;
      double best = inf;
      int key = INT_MIN;
      for (int it = lane; it < nrem; it += 64) {
        const int j = s.remaining[it];
        const double r = ((min_val + crow[(size_t)j * cs]) - ui) - s.v[j];
        double sh = s.shortest[j];
        if (r < sh) {
          s.path[j] = i;
          s.shortest[j] = sh = r;
        }
        const int k = s.row4col[j] == -1 ? it + kUnassigned : -it;
        if (sh < best || (sh == best && k > key)) {
          best = sh;
          key = k;
        }
      }
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const double ob = __shfl_xor(best, m);
        const int ok = __shfl_xor(key, m);
        if (ob < best || (ob == best && ok > key)) {
          best = ob;
          key = ok;
        }
      }
      if (!(best < inf)) {  // an infeasible matrix (SciPy raises); also what NaNs end in
        feasible = false;
        break;
      }
      min_val = best;
      const int itw = __builtin_amdgcn_readfirstlane(key > 0 ? key - kUnassigned : -key);
      const int j = __builtin_amdgcn_readfirstlane(s.remaining[itw]);
      const int r4 = __builtin_amdgcn_readfirstlane(s.row4col[j]);
      if (r4 == -1)
        sink = j;
      else
        i = r4;
      --nrem;
      __syncthreads();  // every lane has read remaining[itw]
      if (lane == 0) {
        s.remaining[itw] = s.remaining[nrem];
        s.remaining[nrem] = j;
      }
      __syncthreads();
    }
    if (!feasible) break;
    // dual variables: u[cur] += minVal; visited rows u[i] += minVal - shortest[col4row[i]]; visited
    // columns v[j] -= minVal - shortest[j]
    if (lane == 0) s.u[cur] += min_val;
    for (int t = nrem + lane; t < nc; t += 64) {
      const int j = s.remaining[t];
      const double d = min_val - s.shortest[j];
      s.v[j] -= d;
      const int r4 = s.row4col[j];
      if (r4 != -1) s.u[r4] += d;
    }
    __syncthreads();
    // augment along path[] from the sink back to the current row
    if (lane == 0) {
      int j = sink;
      while (true) {
        const int pi = s.path[j];
        s.row4col[j] = pi;
        const int t = s.col4row[pi];
        s.col4row[pi] = j;
        j = t;
        if (pi == cur) break;
      }
    }
    __syncthreads();
  }
  if (!feasible) {
    for (int k = lane; k < nr; k += 64) ri[k] = ci[k] = -1;
    return;
  }
  if (!tr) {
    for (int k = lane; k < nr; k += 64) {
      ri[k] = k;
      ci[k] = s.col4row[k];
    }
    return;
  }
  // the working columns are the caller's rows: ascending, those that are assigned
  int base = 0;
  for (int j0 = 0; j0 < nc; j0 += 64) {
    const int j = j0 + lane;
    const int r4 = j < nc ? s.row4col[j] : -1;
    const unsigned long long bal = __ballot(r4 != -1);
    if (r4 != -1) {
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      ri[pos] = j;
      ci[pos] = r4;
    }
    base += __popcll(bal);
  }
}

constexpr size_t kLdsLimit = 64 * 1024;

hipError_t launch_lsa(const double* cost, int B, int nr, int nc, size_t rs, size_t cs, bool tr, int64_t* row_ind,
                      int64_t* col_ind, void* state, hipStream_t st) {
  const size_t sb = lsa_state_bytes(nr, nc);
  if (sb <= kLdsLimit)
    lsa_solve<true><<<dim3((unsigned)B), dim3(64), sb, st>>>(cost, (size_t)nr * nc, nr, nc, rs, cs, tr, row_ind, col_ind,
                                                              nullptr, 0);
  else
    lsa_solve<false><<<dim3((unsigned)B), dim3(64), 0, st>>>(cost, (size_t)nr * nc, nr, nc, rs, cs, tr, row_ind, col_ind,
                                                             static_cast<char*>(state), up256(sb));
  return hipGetLastError();
}

size_t lsa_global_state_bytes(int B, int nr, int nc) {
  const size_t sb = lsa_state_bytes(nr, nc);
  return sb <= kLdsLimit ? 0 : (size_t)B * up256(sb);
}

inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side

int gt_line_count_threshold_visibility(int npts, double min_visibility_th) {
  // mean(out) >= 1 - min_visibility_th (:465): an fp32 mean against the Python float, which torch
  // compares as fp32
  const float rhs = (float)(1.0 - min_visibility_th);
  for (int c = 0; c <= npts; ++c)
    if ((float)c / (float)npts >= rhs) return c;
  return npts + 1;
}

int gt_line_count_threshold_overlap(int npts, double overlap_th) {
  // count > npts * overlap_th (:492-493): the integer count and the Python product, both as fp32
  const float rhs = (float)((double)npts * overlap_th);
  for (int c = 0; c <= npts; ++c)
    if ((float)c > rhs) return c;
  return npts + 1;
}

int gt_line_count_threshold_valid_depth(int npts, double min_visibility_th) {
  // ignored: mean(valid) < min_visibility_th (:345-347), fp32 as above; the smallest count that is not
  const float rhs = (float)min_visibility_th;
  for (int c = 0; c <= npts; ++c)
    if (!((float)c / (float)npts < rhs)) return c;
  return npts + 1;
}

void gt_line_min_close_table(int npts, double overlap_th, int* min_close) {
  // count > visible.float().sum(-1) * overlap_th (:329-336): the int64 count as fp32 against the fp32
  // product of the fp32 sum and the Python float
  const float th = (float)overlap_th;
  for (int v = 0; v <= npts; ++v) {
    const float rhs = (float)v * th;
    int c = 0;
    while (c <= npts && !((float)c > rhs)) ++c;
    min_close[v] = c;  // npts + 1: no count qualifies
  }
}

size_t gt_line_counts_workspace_bytes(int B, int n0, int n1, int npts) {
  const size_t l0 = (size_t)B * n0, l1 = (size_t)B * n1;
  return up256(l0 * 32) + up256(l1 * 32) + up256(l0 * npts * 8) + up256(l1 * npts * 8);
}

hipError_t gt_line_counts_homography(const float* lines0, const float* lines1, const float* H, int B, int n0, int n1, int w0,
                                     int h0, int w1, int h1, int npts, float dist_th, int vis_min, uint8_t* cnt0,
                                     uint8_t* cnt1t, uint8_t* out_of0, uint8_t* out_of1, void* workspace, hipStream_t st) {
  char* w = static_cast<char*>(workspace);
  const size_t l0 = (size_t)B * n0, l1 = (size_t)B * n1;
  float* seg0 = reinterpret_cast<float*>(w);
  w += up256(l0 * 32);
  float* seg1 = reinterpret_cast<float*>(w);
  w += up256(l1 * 32);
  float* pts01 = reinterpret_cast<float*>(w);
  w += up256(l0 * npts * 8);
  float* pts10 = reinterpret_cast<float*>(w);
  gl_prepare<<<dim3((unsigned)((l0 + l1 + 255) / 256)), dim3(256), 0, st>>>(lines0, lines1, H, B, n0, n1, w0, h0, w1, h1, npts,
                                                                           vis_min, seg0, seg1, pts01, pts10, out_of0,
                                                                           out_of1);
  const int ti_n = (n0 + kTile - 1) / kTile, tj_n = (n1 + kTile - 1) / kTile;
  const int stride = npts | 1;
  const size_t lds = (size_t)2 * kTile * stride * sizeof(float2);  // at most 65280 bytes (npts <= 255)
  gl_counts<<<dim3((unsigned)((size_t)B * ti_n * tj_n)), dim3(kTile * kTile), lds, st>>>(seg0, seg1, pts01, pts10, n0, n1, ti_n,
                                                                                        tj_n, npts, stride, dist_th, cnt0,
                                                                                        cnt1t);
  return hipGetLastError();
}

hipError_t gt_line_counts_pose_depth(const GtLineDepthCall& c, void* workspace, hipStream_t st) {
  char* w = static_cast<char*>(workspace);
  const size_t l0 = (size_t)c.B * c.n0, l1 = (size_t)c.B * c.n1;
  LineDepthArgs a;
  a.lines0 = c.lines0, a.lines1 = c.lines1, a.depth0 = c.depth0, a.depth1 = c.depth1, a.cam0 = c.cam0, a.cam1 = c.cam1;
  a.T01 = c.T_0to1, a.T10 = c.T_1to0;
  a.B = c.B, a.n0 = c.n0, a.n1 = c.n1, a.H0 = c.H0, a.W0 = c.W0, a.H1 = c.H1, a.W1 = c.W1;
  a.ih0 = c.ih0, a.iw0 = c.iw0, a.ih1 = c.ih1, a.iw1 = c.iw1, a.nd = c.n_dist, a.npts = c.npts;
  a.out_min = c.out_min, a.valid_min = c.valid_min;
  a.seg0 = reinterpret_cast<float*>(w);
  w += up256(l0 * 32);
  a.seg1 = reinterpret_cast<float*>(w);
  w += up256(l1 * 32);
  a.pts01 = reinterpret_cast<float*>(w);
  w += up256(l0 * c.npts * 8);
  a.pts10 = reinterpret_cast<float*>(w);
  a.out_of0 = c.out_of0, a.out_of1 = c.out_of1, a.ignd0 = c.ignore_depth0, a.ignd1 = c.ignore_depth1;
  a.nvis0 = c.num_visible0, a.nvis1 = c.num_visible1;
  gld_prepare<<<dim3((unsigned)((l0 + l1 + 3) / 4)), dim3(256), 0, st>>>(a);
  const int ti_n = (c.n0 + kTile - 1) / kTile, tj_n = (c.n1 + kTile - 1) / kTile;
  const int stride = c.npts | 1;
  const size_t lds = (size_t)2 * kTile * stride * sizeof(float2);
  gl_counts<<<dim3((unsigned)((size_t)c.B * ti_n * tj_n)), dim3(kTile * kTile), lds, st>>>(
      a.seg0, a.seg1, a.pts01, a.pts10, c.n0, c.n1, ti_n, tj_n, c.npts, stride, c.dist_th, c.cnt0, c.cnt1t);
  return hipGetLastError();
}

size_t linear_sum_assignment_workspace_bytes(int B, int nr, int nc) {
  return lsa_global_state_bytes(B, imin(nr, nc), imax(nr, nc));
}

hipError_t linear_sum_assignment(const double* cost, int B, int nr, int nc, int64_t* row_ind, int64_t* col_ind,
                                 void* workspace, hipStream_t st) {
  if (nc >= nr) return launch_lsa(cost, B, nr, nc, (size_t)nc, 1, false, row_ind, col_ind, workspace, st);
  return launch_lsa(cost, B, nc, nr, 1, (size_t)nc, true, row_ind, col_ind, workspace, st);
}

size_t gt_line_labels_workspace_bytes(int B, int n0, int n1) {
  const int nmin = imin(n0, n1), nmax = imax(n0, n1);
  return up256((size_t)B * n0 * n1 * 8) + 2 * up256((size_t)B * nmin * 8) + up256((size_t)B * n0) + up256((size_t)B * n1) +
         lsa_global_state_bytes(B, nmin, nmax);
}

namespace {
template <class Min>
hipError_t line_labels(const uint8_t* cnt0, const uint8_t* cnt1t, const uint8_t* out_of0, const uint8_t* out_of1,
                       const uint8_t* valid0, const uint8_t* valid1, int B, int n0, int n1, const Min& mn, uint8_t* positive,
                       int64_t* m0, int64_t* m1, void* workspace, hipStream_t st) {
  const int nmin = imin(n0, n1), nmax = imax(n0, n1);
  char* w = static_cast<char*>(workspace);
  double* cost = reinterpret_cast<double*>(w);
  w += up256((size_t)B * n0 * n1 * 8);
  int64_t* row_ind = reinterpret_cast<int64_t*>(w);
  w += up256((size_t)B * nmin * 8);
  int64_t* col_ind = reinterpret_cast<int64_t*>(w);
  w += up256((size_t)B * nmin * 8);
  uint8_t* dead0 = reinterpret_cast<uint8_t*>(w);
  w += up256((size_t)B * n0);
  uint8_t* dead1 = reinterpret_cast<uint8_t*>(w);
  w += up256((size_t)B * n1);
  const size_t total = (size_t)B * n0 * n1;
  const unsigned rb = (unsigned)(((size_t)B * n0 + 3) / 4), cb = (unsigned)(((size_t)B * n1 + 255) / 256);
  gl_flags<Min><<<dim3(rb + cb), dim3(256), 0, st>>>(cnt0, cnt1t, out_of0, out_of1, valid0, valid1, B, n0, n1, mn, rb, dead0,
                                                     dead1, m0, m1);
  const bool tr = n1 < n0;
  gl_cost<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(cnt0, cnt1t, dead0, dead1, total, n0, n1, tr, cost);
  // the transposed cost is stored contiguous, so the solver walks rows of unit stride either way
  hipError_t e = launch_lsa(cost, B, nmin, nmax, (size_t)nmax, 1, tr, row_ind, col_ind, w, st);
  if (e != hipSuccess) return e;
  launch_fill0(positive, total, st);
  gl_pairs<Min><<<dim3((unsigned)(((size_t)B * nmin + 255) / 256)), dim3(256), 0, st>>>(cnt0, cnt1t, dead0, dead1, row_ind,
                                                                                       col_ind, B, n0, n1, nmin, mn, positive,
                                                                                       m0, m1);
  return hipGetLastError();
}
}  // namespace

hipError_t gt_line_labels(const uint8_t* cnt0, const uint8_t* cnt1t, const uint8_t* out_of0, const uint8_t* out_of1,
                          const uint8_t* valid0, const uint8_t* valid1, int B, int n0, int n1, int ov_min, uint8_t* positive,
                          int64_t* m0, int64_t* m1, void* workspace, hipStream_t st) {
  return line_labels(cnt0, cnt1t, out_of0, out_of1, valid0, valid1, B, n0, n1, OneMin{ov_min}, positive, m0, m1, workspace, st);
}

hipError_t gt_line_labels_visibility(const uint8_t* cnt0, const uint8_t* cnt1t, const uint8_t* out_of0, const uint8_t* out_of1,
                                     const uint8_t* ignore_depth0, const uint8_t* ignore_depth1, const uint8_t* num_visible0,
                                     const uint8_t* num_visible1, const uint8_t* valid0, const uint8_t* valid1, int B, int n0,
                                     int n1, int npts, const int* min_close, uint8_t* positive, int64_t* m0, int64_t* m1,
                                     void* workspace, hipStream_t st) {
  PerLineMin mn;
  mn.nvis0 = num_visible0, mn.nvis1 = num_visible1, mn.ignd0 = ignore_depth0, mn.ignd1 = ignore_depth1;
  for (int v = 0; v < 256; ++v) mn.tab.min_close[v] = (uint16_t)(v <= npts ? min_close[v] : npts + 1);
  return line_labels(cnt0, cnt1t, out_of0, out_of1, valid0, valid1, B, n0, n1, mn, positive, m0, m1, workspace, st);
}

}  // namespace lg
