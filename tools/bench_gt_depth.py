#!/usr/bin/env python3
"""Time the HIP pose-and-depth ground truth (lightglue_amd.depth_matcher) against the torch chain it
replaces: the reference's gt_matches_from_pose_depth formula (gt_generation.py:13-106 over
depth.py:8-68, the Camera / Pose arithmetic of wrappers.py, utils.py:90-127 and epipolar.py:59-72)
restated below with torch ops and run on the same GPU -- what a caller had for ground truth on the
device before.

Shapes: 32 x 2048 x 2048 with 480 x 640 depth maps (the training shape) and 1 x 1024 x 1024; with and
without ``reward``; plain, with ``th_consistency``, and with ``th_consistency`` + ``th_epi``.  Times
are HIP-event times per call over ``--iters`` back-to-back calls after ``--warmup`` calls, the two
implementations alternating in ``--rounds`` rounds (median and min..max over rounds reported); peak
memory is ``torch.cuda.max_memory_allocated`` above what was allocated before the call.  The outputs
of both are compared before timing (near-ties aside: the disagreements are counted, not hidden).

    python tools/bench_gt_depth.py [--json out.json]

Needs a HIP device; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lgamd  # noqa: E402,F401
from lightglue_amd.depth_matcher import gt_matches_from_pose_depth as hip_gt  # noqa: E402


# ---------------------------------------------------------------------------------------------
# the baseline: the reference's formula, as written, on the device
def sample_depth(pts, depth_):
    depth = torch.where(depth_ > 0, depth_, depth_.new_tensor(float("nan")))[:, None]
    h, w = depth.shape[-2:]
    grid = (pts / pts.new_tensor([[w, h]]) * 2 - 1)[:, None]
    lin = torch.nn.functional.grid_sample(depth, grid, align_corners=False, mode="bilinear")
    nn = torch.nn.functional.grid_sample(depth, grid, align_corners=False, mode="nearest")
    interp = torch.where(torch.isnan(lin), nn, lin)[:, :, 0].permute(0, 2, 1).squeeze(-1)
    return interp, (~torch.isnan(interp)) & (interp > 0)


def distort_points(pts, dist):
    dist = dist.unsqueeze(-2)
    undist, valid = pts, torch.ones(pts.shape[:-1], device=pts.device, dtype=torch.bool)
    if dist.shape[-1] > 0:
        k1, k2 = dist[..., :2].split(1, -1)
        r2 = torch.sum(pts**2, -1, keepdim=True)
        undist = undist + pts * (k1 * r2 + k2 * r2**2)
        limited = ((k2 > 0) & ((9 * k1**2 - 20 * k2) > 0)) | ((k2 <= 0) & (k1 > 0))
        limit = torch.abs(torch.where(k2 > 0, (torch.sqrt(9 * k1**2 - 20 * k2) - 3 * k1) / (10 * k2), 1 / (3 * k1)))
        valid = valid & torch.squeeze(~limited | (r2 < limit), -1)
        if dist.shape[-1] > 2:
            p12 = dist[..., 2:]
            undist = undist + 2 * p12 * torch.prod(pts, -1, keepdim=True) + p12.flip(-1) * (r2 + 2 * pts**2)
    return undist, valid


def image2cam(cam, p2d):
    p = (p2d - cam[..., 4:6].unsqueeze(-2)) / cam[..., 2:4].unsqueeze(-2)
    return torch.cat([p, p.new_ones(p.shape[:-1] + (1,))], -1)


def cam2image(cam, p3d):
    z = p3d[..., -1]
    visible = z > 1e-4
    p2d = p3d[..., :-1] / z.clamp(min=1e-4).unsqueeze(-1)
    p2d, mask = distort_points(p2d, cam[..., 6:])
    p2d = p2d * cam[..., 2:4].unsqueeze(-2) + cam[..., 4:6].unsqueeze(-2)
    inside = torch.all((p2d >= 0) & (p2d <= (cam[..., :2].unsqueeze(-2) - 1)), -1)
    return p2d, visible & mask & inside


def pose_R(T):
    return T[..., :9].reshape(T.shape[:-1] + (3, 3))


def transform(T, p3d):
    return p3d @ pose_R(T).transpose(-1, -2) + T[..., -3:].unsqueeze(-2)


def pose_inv(T):
    R = pose_R(T).transpose(-1, -2)
    t = -(R @ T[..., -3:].unsqueeze(-1)).squeeze(-1)
    return torch.cat([R.flatten(start_dim=-2), t], -1)


def project(kpi, di, depthj, cam_i, cam_j, T, validi, ccth):
    kpi_j, validj = cam2image(cam_j, transform(T, image2cam(cam_i, kpi) * di[..., None]))
    validi = validi & validj
    if ccth is None:
        return kpi_j, validi
    dj, validj = sample_depth(kpi_j, depthj)
    back, valid_back = cam2image(cam_i, transform(pose_inv(T), image2cam(cam_j, kpi_j) * dj[..., None]))
    consistent = ((kpi - back) ** 2).sum(-1) < ccth
    return kpi_j, validi & consistent & valid_back & validj


def calibration_matrix(cam):
    K = torch.zeros(*cam.shape[:-1], 3, 3, device=cam.device, dtype=cam.dtype)
    K[..., 0, 2], K[..., 1, 2], K[..., 0, 0], K[..., 1, 1], K[..., 2, 2] = cam[..., 4], cam[..., 5], cam[..., 2], cam[..., 3], 1.0
    return K


def skew(v):
    z = torch.zeros_like(v[..., 0])
    return torch.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], -1).reshape(
        v.shape[:-1] + (3, 3))


def sym_epipolar_distance_all(p0, p1, E, eps=1e-15):
    hom = lambda p: torch.cat([p, p.new_ones(p.shape[:-1] + (1,))], -1)  # noqa: E731
    p0, p1 = hom(p0), hom(p1)
    p1_E_p0 = torch.einsum("...mi,...ij,...nj->...nm", p1, E, p0).abs()
    E_p0 = torch.einsum("...ij,...nj->...ni", E, p0)
    Et_p1 = torch.einsum("...ij,...mi->...mj", E, p1)
    d0 = p1_E_p0 / (E_p0[..., None, 0] ** 2 + E_p0[..., None, 1] ** 2 + eps).sqrt()
    d1 = p1_E_p0 / (Et_p1[..., None, :, 0] ** 2 + Et_p1[..., None, :, 1] ** 2 + eps).sqrt()
    return (d0 + d1) / 2


@torch.no_grad()
def torch_gt(kp0, kp1, s, pos_th, neg_th, epi_th, cc_th, reward=True):
    """gt_generation.py:26-106 as written, on the device (the reward only when asked for, as the HIP path)."""
    d0, valid0 = sample_depth(kp0, s["depth0"])
    d1, valid1 = sample_depth(kp1, s["depth1"])
    kp0_1, visible0 = project(kp0, d0, s["depth1"], s["cam0"], s["cam1"], s["T01"], valid0, cc_th)
    kp1_0, visible1 = project(kp1, d1, s["depth0"], s["cam1"], s["cam0"], s["T10"], valid1, cc_th)
    mask_visible = visible0.unsqueeze(-1) & visible1.unsqueeze(-2)
    dist0 = torch.sum((kp0_1.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2, -1)
    dist1 = torch.sum((kp0.unsqueeze(-2) - kp1_0.unsqueeze(-3)) ** 2, -1)
    dist = torch.max(dist0, dist1)
    inf = dist.new_tensor(float("inf"))
    dist = torch.where(mask_visible, dist, inf)
    min0 = dist.min(-1).indices
    min1 = dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < pos_th**2)
    negative0 = (dist0.min(-1).values > neg_th**2) & valid0
    negative1 = (dist1.min(-2).values > neg_th**2) & valid1
    unmatched, ignore = min0.new_tensor(-1), min0.new_tensor(-2)
    m0 = torch.where(positive.any(-1), min0, ignore)
    m1 = torch.where(positive.any(-2), min1, ignore)
    m0 = torch.where(negative0, unmatched, m0)
    m1 = torch.where(negative1, unmatched, m1)
    out = {"assignment": positive}
    if reward or epi_th is not None:
        F = (calibration_matrix(s["cam1"]).inverse().transpose(-1, -2) @ (skew(s["T01"][..., -3:]) @ pose_R(s["T01"]))
             @ calibration_matrix(s["cam0"]).inverse())
        epi_dist = sym_epipolar_distance_all(kp0, kp1, F)
        if epi_th is not None:
            mask_ignore = (m0.unsqueeze(-1) == ignore) & (m1.unsqueeze(-2) == ignore)
            epi_dist = torch.where(mask_ignore, epi_dist, inf)
            m0 = torch.where((~valid0) & (epi_dist.min(-1).values > neg_th), ignore.new_tensor(-1), m0)
            m1 = torch.where((~valid1) & (epi_dist.min(-2).values > neg_th), ignore.new_tensor(-1), m1)
        if reward:
            out["reward"] = (dist < pos_th**2).float() - (epi_dist > neg_th).float()
    out.update({"matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(), "matching_scores1": (m1 > -1).float(),
                "depth_keypoints0": d0, "depth_keypoints1": d1, "proj_0to1": kp0_1, "proj_1to0": kp1_0, "visible0": visible0,
                "visible1": visible1})
    return out


# ---------------------------------------------------------------------------------------------
def make_inputs(B, M, N, H, W, seed, dev):
    """A tilted plane at depth ~5 seen by two pinhole-plus-radial cameras (rotation 0.08 rad about a
    random axis, baseline 0.2 .. 0.4), 12 zero rectangles per depth map; half of image 1 is the
    reprojection of image-0 points plus 1 px noise."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    n_ = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    f = 0.95 * W
    cam0 = torch.tensor([W, H, f, 1.02 * f, W / 2 + 1.5, H / 2 - 2.5, -0.06, 0.015], dtype=torch.float64).repeat(B, 1)
    cam1 = cam0.clone()
    cam1[:, 2:4] *= 1.03
    aa = n_(B, 3)
    aa = aa / aa.norm(dim=-1, keepdim=True) * 0.08
    K = skew(aa / 0.08)
    R = torch.eye(3, dtype=torch.float64) + torch.sin(torch.tensor(0.08)) * K + (1 - torch.cos(torch.tensor(0.08))) * K @ K
    t = n_(B, 3)
    t = t / t.norm(dim=-1, keepdim=True) * (0.2 + 0.2 * r(B, 1))
    T01 = torch.cat([R.flatten(start_dim=-2), t], -1)
    T10 = pose_inv(T01)
    nrm = torch.cat([0.3 * r(B, 2) - 0.15, torch.ones(B, 1, dtype=torch.float64)], -1)
    nrm1 = (R @ nrm.unsqueeze(-1)).squeeze(-1)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    maps = []
    for cam, nn, h in ((cam0, nrm, torch.full((B,), 5.0, dtype=torch.float64)), (cam1, nrm1, 5.0 + (nrm1 * t).sum(-1))):
        ray = torch.stack([(u[None] - cam[:, 4, None, None]) / cam[:, 2, None, None],
                           (v[None] - cam[:, 5, None, None]) / cam[:, 3, None, None], torch.ones(B, H, W, dtype=torch.float64)], -1)
        d = h[:, None, None] / (ray * nn[:, None, None, :]).sum(-1)
        for b in range(B):
            for _ in range(12):
                hw, hh = int(8 + r(1) * W / 6), int(8 + r(1) * H / 6)
                x0, y0 = int(r(1) * (W - hw)), int(r(1) * (H - hh))
                d[b, y0:y0 + hh, x0:x0 + hw] = 0.0
        maps.append(d)
    size = torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)
    kp0, kp1 = r(B, M, 2) * size, r(B, N, 2) * size
    d0, v0 = sample_depth(kp0, maps[0])
    p01, _ = project(kp0, d0, None, cam0, cam1, T01, v0, None)
    nw = min(N // 2, M)
    ok = torch.isfinite(p01[:, :nw]).all(-1, keepdim=True)
    kp1[:, :nw] = torch.where(ok, (p01[:, :nw] + n_(B, nw, 2)).clamp(min=torch.zeros(2, dtype=torch.float64), max=size), kp1[:, :nw])
    f32 = lambda x: x.to(torch.float32).to(dev).contiguous()  # noqa: E731
    return f32(kp0), f32(kp1), {"depth0": f32(maps[0]), "depth1": f32(maps[1]), "cam0": f32(cam0), "cam1": f32(cam1),
                                "T01": f32(T01), "T10": f32(T10)}


def time_calls(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_above_baseline(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gt_depth.py needs a HIP device")
    dev = torch.device("cuda", 0)
    pos, neg = 3.0, 5.0
    rows = []
    for B, M, N, H, W in ((32, 2048, 2048, 480, 640), (1, 1024, 1024, 480, 640)):
        kp0, kp1, s = make_inputs(B, M, N, H, W, 7, dev)
        data = {"view0": {"camera": s["cam0"], "depth": s["depth0"]}, "view1": {"camera": s["cam1"], "depth": s["depth1"]},
                "T_0to1": s["T01"], "T_1to0": s["T10"]}
        for variant, cc, epi in (("plain", None, None), ("th_consistency", 4.0, None), ("th_consistency+th_epi", 4.0, 1.0)):
            for reward in (True, False):
                fns = {"hip": lambda: hip_gt(kp0, kp1, data, pos, neg, epi, cc, reward=reward),
                       "torch": lambda: torch_gt(kp0, kp1, s, pos, neg, epi, cc, reward=reward)}
                oh, ot = fns["hip"](), fns["torch"]()
                keys = ["assignment", "matches0", "matches1", "visible0", "visible1"] + (["reward"] if reward else [])
                diff = {k: int((oh[k] != ot[k]).sum()) for k in keys}
                labels = {"matched": int((oh["matches0"] > -1).sum()), "unmatched": int((oh["matches0"] == -1).sum()),
                          "ignored": int((oh["matches0"] == -2).sum())}
                del oh, ot
                peak = {k: peak_above_baseline(f) for k, f in fns.items()}
                for f in fns.values():
                    for _ in range(a.warmup):
                        f()
                torch.cuda.synchronize()
                ms = {k: [] for k in fns}
                for _ in range(a.rounds):  # alternate the two in every round
                    for k, f in fns.items():
                        ms[k].append(time_calls(f, a.iters))
                written = (5 if reward else 1) * B * M * N + B * (M + N) * (8 + 4 + 8 + 4 + 1)
                row = {"B": B, "M": M, "N": N, "H": H, "W": W, "variant": variant, "reward": reward, "labels_image0": labels,
                       "entries_differing": diff, "bytes_written_hip": written}
                for k in fns:
                    row[f"{k}_ms_median"] = statistics.median(ms[k])
                    row[f"{k}_ms_min"], row[f"{k}_ms_max"] = min(ms[k]), max(ms[k])
                    row[f"{k}_peak_bytes"] = peak[k]
                row["hip_write_GBps"] = written / (row["hip_ms_median"] * 1e-3) / 1e9
                row["speedup"] = row["torch_ms_median"] / row["hip_ms_median"]
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
