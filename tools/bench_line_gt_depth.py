#!/usr/bin/env python3
"""Time the HIP pose-and-depth line ground truth (lightglue_amd.line_gt.gt_line_matches_from_pose_depth)
against a reference-style chain in the same process: the formula of gt_generation.py:207-406 written with
dense fp32 torch ops on the same GPU (four ``grid_sample`` calls, the camera chain, two
[B, n0, n1, npts] passes masked by visibility), the [B, n0, n1] cost copied to the host, SciPy's
linear_sum_assignment per pair (where SciPy imports; otherwise only the dense part is timed) and the
labels scattered back on the device -- what a caller had before.

Shapes: B = 32 and B = 1 with 250 x 250 lines, npts = 50 and 480 x 640 depth maps (the training shape of
the superpoint+lsd+gluestick-megadepth configuration), pinhole cameras, the scene of
tests/gt_depth_ref.py:plane_scene.  Per shape: the whole call, stage A (projection and counts) and stage B
(labels with the solver) of the HIP path, and the chain with its dense part and its host part separately.
Timing and peak memory as tools/bench_line_gt.py measures them (HIP-event times per call over ``--iters``
back-to-back calls after ``--warmup`` calls, the implementations alternating in ``--rounds`` rounds;
``torch.cuda.max_memory_allocated`` above what was allocated before the call).  The labels of both are
compared before timing and the disagreements counted (near-ties of the fp32 arithmetic).

    python tools/bench_line_gt_depth.py [--json profiles/line_gt_depth/bench_line_gt_depth.json]

Needs a HIP device; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lgamd  # noqa: E402,F401
from bench_line_gt import chain_labels, peak_above_baseline, scipy_lsa, time_calls  # noqa: E402
from gt_depth_ref import plane_scene  # noqa: E402
from lightglue_amd import line_gt  # noqa: E402

W, H_IMG = 640, 480


def sample_depth(pts, depth):  # depth.py:8-25
    d = torch.where(depth > 0, depth, depth.new_tensor(float("nan")))[:, None]
    grid = (pts / pts.new_tensor([W, H_IMG]) * 2 - 1)[:, None]
    lin = torch.nn.functional.grid_sample(d, grid, align_corners=False, mode="bilinear")
    near = torch.nn.functional.grid_sample(d, grid, align_corners=False, mode="nearest")
    d = torch.where(torch.isnan(lin), near, lin)[:, 0, 0]
    return d, ~torch.isnan(d) & (d > 0)


def project(pts, d, valid, cam_i, cam_j, T):  # depth.py:37-59, pinhole cameras
    p = (pts - cam_i[:, None, 4:6]) / cam_i[:, None, 2:4]
    p3 = torch.cat([p, torch.ones_like(p[..., :1])], -1) * d[..., None]
    q = p3 @ T[:, :9].reshape(-1, 3, 3).transpose(1, 2) + T[:, None, 9:]
    z = q[..., 2]
    uv = q[..., :2] / z.clamp(min=1e-4)[..., None] * cam_j[:, None, 2:4] + cam_j[:, None, 4:6]
    inside = ((uv >= 0) & (uv <= cam_j[:, None, :2] - 1)).all(-1)
    return uv, valid & (z > 1e-4) & inside


def chain_dense(l0, l1, v0, v1, scene, npts, dist_th, overlap_th, vis_th):
    """The dense half of the chain: everything up to the cost matrix, in fp32 on the device."""
    dev = l0.device
    B, n0, n1 = l0.shape[0], l0.shape[1], l1.shape[1]

    def clamp(l):
        return torch.minimum(l.clamp_min(0.0), l.new_tensor([W - 1, H_IMG - 1, W - 1, H_IMG - 1]))

    def samples(l):
        step = (l[..., 2:] - l[..., :2]) / (npts - 1)
        return l[..., None, :2] + step[..., None, :] * torch.arange(npts, device=dev, dtype=l.dtype)[:, None]

    def counts(seg, pts, vis):  # [B, nseg, nlines]
        d = seg[..., 2:] - seg[..., :2]
        size = d.norm(dim=-1).half().float()
        nd = d / size[..., None]
        c = pts[:, None] - seg[:, :, None, None, 2:]
        nx, ny = nd[..., 0, None, None], nd[..., 1, None, None]
        along = nx * c[..., 0] + ny * c[..., 1]
        across = nx * c[..., 1] - ny * c[..., 0]
        close = (across.abs() < dist_th) & (along <= 0) & (along.abs() <= size[..., None, None])
        return (close & vis[:, None]).sum(-1)

    def leaves(p):
        out = (p < 0).any(-1) | (p >= p.new_tensor([W, H_IMG])).any(-1)
        return out.float().mean(-1) >= (1 - vis_th)

    c0, c1 = clamp(l0), clamp(l1)
    s0, s1 = samples(c0).reshape(B, n0 * npts, 2), samples(c1).reshape(B, n1 * npts, 2)
    d0, val0 = sample_depth(s0, scene["depth0"])
    d1, val1 = sample_depth(s1, scene["depth1"])
    p01, vis0 = project(s0, d0, val0, scene["camera0"], scene["camera1"], scene["T_0to1"])
    p10, vis1 = project(s1, d1, val1, scene["camera1"], scene["camera0"], scene["T_1to0"])
    p01, p10 = p01.reshape(B, n0, npts, 2), p10.reshape(B, n1, npts, 2)
    vis0, vis1 = vis0.reshape(B, n0, npts), vis1.reshape(B, n1, npts)
    out0, out1 = leaves(p10), leaves(p01)
    n_a, n_b = counts(c0, p10, vis1), counts(c1, p01, vis0).transpose(1, 2)
    mask = (n_b > vis0.float().sum(-1)[:, :, None] * overlap_th) & (n_a > vis1.float().sum(-1)[:, None] * overlap_th)
    keep0 = v0 & ~(val0.reshape(B, n0, npts).float().mean(-1) < vis_th)
    keep1 = v1 & ~(val1.reshape(B, n1, npts).float().mean(-1) < vis_th)
    dead0 = ~mask.any(2) | out1 | ~keep0
    dead1 = ~mask.any(1) | out0 | ~keep1
    cost = -(n_a * n_b)
    cost = torch.where(dead0[:, :, None] | dead1[:, None], torch.full_like(cost, 1000000), cost)
    return n_a, n_b, mask, dead0, dead1, cost, keep0, keep1


def make_inputs(B, n0, n1, seed, dev):
    """plane_scene at 640 x 480 without distortion; lines as in tests/golden/make_line_gt_depth_golden.py:
    two thirds of image 1 are lines of image 0 carried over by the scene's projection plus 1.5 px of noise."""
    g = plane_scene(seed, B, 8, 8, n_dist=0, width=W, height=H_IMG)
    scene = {k: torch.from_numpy(g[k]).to(dev) for k in ("depth0", "depth1", "camera0", "camera1", "T_0to1", "T_1to0")}
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    size = np.array([W, H_IMG], float)

    def segments(n):
        a = rng.random((B, n, 2)) * (size + 40.0) - 20.0
        ang = rng.uniform(0, 2 * np.pi, (B, n))
        ln = rng.uniform(20.0, 200.0, (B, n))
        return np.concatenate([a, a + ln[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)], -1).astype(np.float32)

    l0, l1 = torch.from_numpy(segments(n0)).to(dev), torch.from_numpy(segments(n1)).to(dev)
    ends = torch.minimum(l0.clamp_min(0.0), l0.new_tensor([W - 1, H_IMG - 1, W - 1, H_IMG - 1])).reshape(B, n0 * 2, 2)
    d, val = sample_depth(ends, scene["depth0"])
    p, vis = project(ends, d, val, scene["camera0"], scene["camera1"], scene["T_0to1"])
    p, vis = p.reshape(B, n0, 4), vis.reshape(B, n0, 2).all(-1)
    nw = min(2 * n1 // 3, n0)
    noise = torch.from_numpy(rng.standard_normal((B, nw, 4)).astype(np.float32) * 1.5).to(dev)
    l1[:, :nw] = torch.where(vis[:, :nw, None], p[:, :nw] + noise, l1[:, :nw])
    v0, v1 = rng.random((B, n0)) > 1 / 12, rng.random((B, n1)) > 1 / 12
    data = {"view0": {"camera": scene["camera0"], "depth": scene["depth0"]},
            "view1": {"camera": scene["camera1"], "depth": scene["depth1"]}, "T_0to1": scene["T_0to1"], "T_1to0": scene["T_1to0"]}
    return l0, l1, torch.from_numpy(v0).to(dev), torch.from_numpy(v1).to(dev), scene, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_line_gt_depth.py needs a HIP device")
    dev = torch.device("cuda", 0)
    npts, dist_th, overlap_th, vis_th = 50, 5, 0.2, 0.5
    rows = []
    for B, n0, n1 in ((32, 250, 250), (1, 250, 250)):
        l0, l1, v0, v1, scene, data = make_inputs(B, n0, n1, 7, dev)
        cnt = line_gt.close_point_counts_from_pose_depth(l0, l1, data, npts, dist_th, vis_th)
        stage_a = [cnt[k] for k in ("num_close_pts0", "num_close_pts1_t", "out_of0", "out_of1", "ignore_depth0", "ignore_depth1",
                                    "num_visible0", "num_visible1")]
        dense = chain_dense(l0, l1, v0, v1, scene, npts, dist_th, overlap_th, vis_th)
        fns = {
            "hip_total": lambda: line_gt.gt_line_matches_from_pose_depth(l0, l1, v0, v1, data, npts, dist_th, overlap_th, vis_th),
            "hip_counts": lambda: line_gt.close_point_counts_from_pose_depth(l0, l1, data, npts, dist_th, vis_th),
            "hip_labels": lambda: line_gt.line_labels_from_visibility_counts(*stage_a, v0, v1, npts, overlap_th),
            "chain_dense": lambda: chain_dense(l0, l1, v0, v1, scene, npts, dist_th, overlap_th, vis_th),
        }
        row = {"B": B, "n0": n0, "n1": n1, "npts": npts, "depth_hw": [H_IMG, W], "scipy": scipy_lsa is not None}
        if scipy_lsa is not None:
            fns["chain_host"] = lambda: chain_labels(*dense[2:6], dense[6], dense[7])
            fns["chain_total"] = lambda: (lambda d: chain_labels(*d[2:6], d[6], d[7]))(
                chain_dense(l0, l1, v0, v1, scene, npts, dist_th, overlap_th, vis_th))
            # the same labels first (near-ties aside: count the disagreements, do not hide them)
            oh, oc = fns["hip_total"](), fns["chain_total"]()
            row["entries_differing"] = {k: int((x != y).sum()) for k, x, y in zip(("positive", "m0", "m1"), oh, oc)}
            row["positives"] = int(oh[0].sum())
            del oh, oc
        row["counts_differing_from_chain"] = [int((stage_a[0] != dense[0]).sum()), int((stage_a[1] != dense[1]).sum())]
        peak = {k: peak_above_baseline(fns[k]) for k in ("hip_total", "chain_dense")}
        for f in fns.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):  # alternate the implementations in every round
            for k, f in fns.items():
                ms[k].append(time_calls(f, a.iters))
        for k in fns:
            row[f"{k}_ms_median"] = statistics.median(ms[k])
            row[f"{k}_ms_min"], row[f"{k}_ms_max"] = min(ms[k]), max(ms[k])
        row["hip_peak_bytes"], row["chain_dense_peak_bytes"] = peak["hip_total"], peak["chain_dense"]
        ref = "chain_total" if scipy_lsa is not None else "chain_dense"
        row["speedup_vs_" + ref] = row[ref + "_ms_median"] / row["hip_total_ms_median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
