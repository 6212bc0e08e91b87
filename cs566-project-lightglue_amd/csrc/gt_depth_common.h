// The reference's depth sampling and camera chain in fp32, shared by the two translation units that
// project through a depth map: gt_depth.hip (keypoints, gt_generation.py:13-106) and gt_lines.hip
// (samples along lines, gt_generation.py:207-406).  sample_depth is geometry/depth.py:8-25, the
// camera is Camera.image2cam / cam2image of geometry/wrappers.py:337-398 with distort_points
// (geometry/utils.py:90-127), the pose is Pose.transform (wrappers.py:186-193).  Every function rounds
// each product and sum on its own, in the reference's order; both TUs are built with
// -ffp-contract=off (Makefile), so a point gets the same bits in either.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lg {
namespace gt {

struct Cam {
  float w, h, fx, fy, cx, cy, k1, k2, p1, p2;
};
__device__ __forceinline__ Cam load_cam(const float* r, int nd) {
  Cam c = {r[0], r[1], r[2], r[3], r[4], r[5], 0.f, 0.f, 0.f, 0.f};
  if (nd > 0) {
    c.k1 = r[6];
    c.k2 = r[7];
  }
  if (nd > 2) {
    c.p1 = r[8];
    c.p2 = r[9];
  }
  return c;
}

// depth.py:8-25.  The map value with <= 0 (and NaN) as NaN.  (cx, cy) are integral floats.
__device__ __forceinline__ bool in_map(float cx, float cy, int H, int W) {
  return cx >= 0.f && cy >= 0.f && cx <= (float)(W - 1) && cy <= (float)(H - 1);  // false for NaN
}
__device__ __forceinline__ float map_at(const float* depth, int W, float cx, float cy) {
  const float v = depth[(size_t)(int)cy * W + (int)cx];
  return v > 0.f ? v : __builtin_nanf("");
}
// grid_sample(align_corners=False, padding zeros): corners outside the map are skipped, a corner
// inside is added even when its weight is 0 (a NaN neighbour makes the sum NaN), and a NaN sum
// falls back to the nearest sample (round half to even; 0 outside the map).
__device__ __forceinline__ float sample_depth(const float* depth, int H, int W, float x, float y) {
  const float fw = (float)W, fh = (float)H;
  const float ix = ((((x / fw) * 2.f - 1.f) + 1.f) * fw - 1.f) / 2.f;
  const float iy = ((((y / fh) * 2.f - 1.f) + 1.f) * fh - 1.f) / 2.f;
  const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
  const float nw = (x1 - ix) * (y1 - iy), ne = (ix - x0) * (y1 - iy);
  const float sw = (x1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0);
  float acc = 0.f;
  if (in_map(x0, y0, H, W)) acc += map_at(depth, W, x0, y0) * nw;
  if (in_map(x1, y0, H, W)) acc += map_at(depth, W, x1, y0) * ne;
  if (in_map(x0, y1, H, W)) acc += map_at(depth, W, x0, y1) * sw;
  if (in_map(x1, y1, H, W)) acc += map_at(depth, W, x1, y1) * se;
  if (acc != acc) {
    const float nx = rintf(ix), ny = rintf(iy);
    acc = in_map(nx, ny, H, W) ? map_at(depth, W, nx, ny) : 0.f;
  }
  return acc;
}
// depth.py:24: what sample_depth's second result says of a sampled value
__device__ __forceinline__ bool depth_valid(float d) { return d == d && d > 0.f; }

struct P2 {
  float x, y;
  bool ok;
};
// Camera.cam2image (wrappers.py:337-385): project, distort (utils.py:90-127), denormalize, in_image
__device__ __forceinline__ P2 cam2image(const Cam& c, int nd, float X, float Y, float Z) {
  bool ok = Z > 1e-4f;
  const float z = Z < 1e-4f ? 1e-4f : Z;  // clamp(min=eps); a NaN stays NaN
  float x = X / z, y = Y / z;
  if (nd > 0) {
    const float r2 = x * x + y * y;
    const float radial = c.k1 * r2 + c.k2 * (r2 * r2);
    float ux = x + x * radial, uy = y + y * radial;
    const float disc = 9.f * (c.k1 * c.k1) - 20.f * c.k2;
    const bool limited = (c.k2 > 0.f && disc > 0.f) || (c.k2 <= 0.f && c.k1 > 0.f);
    if (limited) {
      const float limit = fabsf(c.k2 > 0.f ? (sqrtf(disc) - 3.f * c.k1) / (10.f * c.k2) : 1.f / (3.f * c.k1));
      ok = ok && r2 < limit;
    }
    if (nd > 2) {
      const float uv = x * y;
      ux = (ux + (2.f * c.p1) * uv) + c.p2 * (r2 + 2.f * (x * x));
      uy = (uy + (2.f * c.p2) * uv) + c.p1 * (r2 + 2.f * (y * y));
    }
    x = ux;
    y = uy;
  }
  x = x * c.fx + c.cx;
  y = y * c.fy + c.cy;
  ok = ok && x >= 0.f && y >= 0.f && x <= c.w - 1.f && y <= c.h - 1.f;
  return {x, y, ok};
}

// A pose row: R row-major, then t.
struct PoseRt {
  float R[9], t[3];
};
__device__ __forceinline__ PoseRt load_pose(const float* T) {
  PoseRt p;
#pragma unroll
  for (int k = 0; k < 9; ++k) p.R[k] = T[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p.t[k] = T[9 + k];
  return p;
}

// depth.py:52-59 without the consistency check: image2cam of camera ci (no undistortion), times the
// depth, T.transform, cam2image of camera cj.  A NaN depth gives NaN coordinates and ok = false.
__device__ __forceinline__ P2 project_to(const Cam& ci, const Cam& cj, int nd, const PoseRt& T, float x, float y, float d) {
  const float nx = (x - ci.cx) / ci.fx, ny = (y - ci.cy) / ci.fy;
  const float X = nx * d, Y = ny * d, Z = 1.f * d;
  const float qx = ((X * T.R[0] + Y * T.R[1]) + Z * T.R[2]) + T.t[0];
  const float qy = ((X * T.R[3] + Y * T.R[4]) + Z * T.R[5]) + T.t[1];
  const float qz = ((X * T.R[6] + Y * T.R[7]) + Z * T.R[8]) + T.t[2];
  return cam2image(cj, nd, qx, qy, qz);
}

}  // namespace gt
}  // namespace lg
