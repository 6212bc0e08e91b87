#!/usr/bin/env python3
"""Time the batched robust homography estimation (lightglue_amd.robust: one launch of
``lg_ransac_homography`` for every pair of a batch).

Shape: 32 x 2048 x 2048 with 600 matches per pair, half of them on the pair's homography with 0.7 px
of noise and half anywhere, at the thresholds 0.5 and 3.0 px (``max_iters`` 3000, confidence 0.995, the
defaults).  Times are HIP-event times per batch over ``--iters`` back-to-back batches after ``--warmup``
batches, in ``--rounds`` rounds (median and min..max over rounds); the mean number of rounds of 256
hypotheses, the success rate and the inlier counts come from the call's ``info``.  There is no baseline
on the same machine: the reference's estimators are OpenCV and PoseLib, which are not installed where
this project runs.

    python tools/bench_ransac.py [--json profiles/ransac/bench_ransac.json]

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
from lightglue_amd import robust  # noqa: E402


def make_inputs(B, M, N, live, ratio, seed, dev):
    g = torch.Generator().manual_seed(seed)
    W, Hh = 640.0, 480.0
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    H = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    H[:, :2, :2] += 0.1 * (u(B, 2, 2) - 0.5)
    H[:, :2, 2] = 40 * (u(B, 2) - 0.5)
    H[:, 2, :2] = 1e-4 * (u(B, 2) - 0.5)
    size = torch.tensor([W, Hh], dtype=torch.float64)
    k0, k1 = u(B, M, 2) * size, u(B, N, 2) * size
    m0 = torch.full((B, M), -1, dtype=torch.int64)
    good = int(round(live * ratio))
    for b in range(B):
        sel, dst = torch.randperm(M, generator=g)[:live], torch.randperm(N, generator=g)[:live]
        q = torch.cat([k0[b, sel[:good]], torch.ones(good, 1, dtype=torch.float64)], 1) @ H[b].T
        k1[b, dst[:good]] = q[:, :2] / q[:, 2:] + 0.7 * torch.randn(good, 2, generator=g, dtype=torch.float64)
        m0[b, sel] = dst
    f = lambda x: x.float().to(dev).contiguous()  # noqa: E731
    pred = {"keypoints0": f(k0), "keypoints1": f(k1), "matches0": m0.to(dev), "matching_scores0": f(u(B, M))}
    data = {"H_0to1": f(H), "view0": {"image_size": f(size.repeat(B, 1))}}
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
                                                   "ransac", "bench_ransac.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ransac.py needs a HIP device")
    dev = torch.device("cuda", 0)
    B, M, N, live, ratio = 32, 2048, 2048, 600, 0.5
    data, pred = make_inputs(B, M, N, live, ratio, 7, dev)
    rows = []
    for th in (0.5, 3.0):
        conf = {"estimator": "hip", "ransac_th": th}
        o = robust.HomographyEstimator.default_conf["options"]
        run = lambda: robust.ransac_homography(  # noqa: E731
            pred["keypoints0"], pred["keypoints1"], pred["matches0"], th, H_gt=data["H_0to1"],
            image_size0=data["view0"]["image_size"], **o)
        full = lambda: robust.eval_homography_robust(data, pred, conf)  # noqa: E731
        info = run()["info"].cpu()
        err = full()["H_error_ransac"].cpu()
        for f in (run, full):
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        ms = {"kernel_call": [], "eval_homography_robust": []}
        for _ in range(a.rounds):
            ms["kernel_call"].append(time_calls(run, a.iters))
            ms["eval_homography_robust"].append(time_calls(full, a.iters))
        row = {"B": B, "M": M, "N": N, "matches_per_pair": live, "inlier_ratio": ratio, "ransac_th": th, **o,
               "device": torch.cuda.get_device_name(0),
               "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
               "mean_rounds_of_256": float(info[:, 5].float().mean()), "success_rate": float(info[:, 0].float().mean()),
               "mean_inliers": float(info[:, 2].float().mean()), "median_H_error_ransac": float(err.median())}
        for k, v in ms.items():
            row[f"{k}_ms_median"], row[f"{k}_ms_min"], row[f"{k}_ms_max"] = statistics.median(v), min(v), max(v)
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
