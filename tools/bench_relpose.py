#!/usr/bin/env python3
"""Time the batched robust relative pose (lightglue_amd.relative_pose: one launch of
``lg_ransac_relpose`` for every pair of a batch).

Shape: 32 x 2048 x 2048 with 600 matches per pair, half of them views of 3-D points under the pair's
pose with 0.7 px of noise and half anywhere, MegaDepth-like intrinsics (f about 1000 px, 1600 x 1200), at
the thresholds 1.0 and 0.5 px (``max_iters`` 2000, confidence 0.9999, the defaults).  Times are HIP-event
times per batch over ``--iters`` back-to-back batches after ``--warmup`` batches, in ``--rounds`` rounds
(median and min..max over rounds); the mean number of rounds of 256 samples, the success rate, the inlier
counts and the median ``rel_pose_error`` come from the call.  The solve / score split is measured on one
round (``max_iters`` 256): the same batch against one cut to 8 matches per pair, where scoring is
negligible and the solve phase is all that is left.  There is no baseline on the same machine: the
reference's estimators are OpenCV, PoseLib and pycolmap, which are not installed where this project runs.

    python tools/bench_relpose.py [--json profiles/relpose/bench_relpose.json]

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
from lightglue_amd import relative_pose as rp  # noqa: E402


def make_inputs(B, M, N, live, ratio, seed, dev):
    g = torch.Generator().manual_seed(seed)
    W, Hh = 1600.0, 1200.0
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    cam = torch.tensor([W, Hh, 1000.0, 1000.0, W / 2, Hh / 2], dtype=torch.float64).repeat(B, 1)
    cam[:, 2:4] += 40 * (u(B, 2) - 0.5)
    size = torch.tensor([W, Hh], dtype=torch.float64)
    k0, k1 = u(B, M, 2) * size, u(B, N, 2) * size
    m0 = torch.full((B, M), -1, dtype=torch.int64)
    T = torch.zeros(B, 12, dtype=torch.float64)
    good = int(round(live * ratio))
    for b in range(B):
        a = n(3)
        a = a / a.norm()
        kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
        ang = 0.05 + 0.2 * float(u(1))
        R = torch.eye(3, dtype=torch.float64) + torch.sin(torch.tensor(ang)) * kx + (1 - torch.cos(torch.tensor(ang))) * kx @ kx
        t = n(3)
        t = t / t.norm()
        T[b] = torch.cat([R.reshape(9), t])
        sel, dst = torch.randperm(M, generator=g)[:live], torch.randperm(N, generator=g)[:live]
        f, c = cam[b, 2:4], cam[b, 4:6]
        z = 4 + 5 * u(good)
        X = torch.cat([(k0[b, sel[:good]] - c) / f * z[:, None], z[:, None]], 1)
        Y = X @ R.T + t
        k1[b, dst[:good]] = Y[:, :2] / Y[:, 2:] * f + c + 0.7 * n(good, 2)
        m0[b, sel] = dst
    f32 = lambda x: x.float().to(dev).contiguous()  # noqa: E731
    pred = {"keypoints0": f32(k0), "keypoints1": f32(k1), "matches0": m0.to(dev), "matching_scores0": f32(u(B, M))}
    data = {"T_0to1": f32(T), "view0": {"camera": f32(cam)}, "view1": {"camera": f32(cam)}}
    return data, pred


def time_calls(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "relpose", "bench_relpose.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_relpose.py needs a HIP device")
    dev = torch.device("cuda", 0)
    B, M, N, live, ratio = 32, 2048, 2048, 600, 0.5
    data, pred = make_inputs(B, M, N, live, ratio, 7, dev)
    cams = (data["view0"]["camera"], data["view1"]["camera"])
    # the first 8 live matches of every pair: one round of it is the solve phase alone
    few = pred["matches0"].clone()
    few[(few > -1).cumsum(1) > 8] = -1
    rows = []
    for th in (1.0, 0.5):
        conf = {"estimator": "hip", "ransac_th": th}
        o = rp.RelativePoseEstimator.default_conf["options"]
        call = lambda m0, **kw: rp.ransac_relpose(  # noqa: E731
            pred["keypoints0"], pred["keypoints1"], m0, *cams, th, T_gt=data["T_0to1"], **{**o, **kw})
        fns = {"kernel_call": lambda: call(pred["matches0"]),
               "eval_relative_pose_robust": lambda: rp.eval_relative_pose_robust(data, pred, conf),
               "one_round": lambda: call(pred["matches0"], max_iters=256),
               "one_round_solve_only": lambda: call(few, max_iters=256)}
        out = fns["kernel_call"]()
        info, err = out["info"].cpu(), out["rel_pose_error"].cpu()
        for f in fns.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                ms[k].append(time_calls(f, a.iters))
        row = {"B": B, "M": M, "N": N, "matches_per_pair": live, "inlier_ratio": ratio, "ransac_th": th, **o,
               "device": torch.cuda.get_device_name(0),
               "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "warmup": a.warmup, "iters": a.iters,
               "rounds": a.rounds, "mean_rounds_of_256": float(info[:, 5].float().mean()),
               "rounds_per_pair": info[:, 5].tolist(), "success_rate": float(info[:, 0].float().mean()),
               "mean_inliers": float(info[:, 2].float().mean()),
               "mean_candidates_per_sample": float((info[:, 7].float() / info[:, 6].float().clamp(min=1)).mean()),
               "median_rel_pose_error": float(err.median())}
        for k, v in ms.items():
            row[f"{k}_ms_median"], row[f"{k}_ms_min"], row[f"{k}_ms_max"] = statistics.median(v), min(v), max(v)
        row["solve_share_of_one_round"] = row["one_round_solve_only_ms_median"] / row["one_round_ms_median"]
        row["pairs_per_s"] = 1e3 * B / row["kernel_call_ms_median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
