#!/usr/bin/env python3
"""Time the HIP homography ground truth (lightglue_amd.gt_matcher) against the torch chain it
replaces: the reference's gt_matches_from_homography formula (gt_generation.py:109-161) run with
torch ops on the same GPU -- what a caller had for ground truth on the device before.

Shapes: 32 x 2048 x 2048 (the training shape) and 1 x 1024 x 1024, with and without ``reward``.
Times are HIP-event times per call over ``--iters`` back-to-back calls after ``--warmup`` calls, the
two implementations alternating in ``--rounds`` rounds (median and min..max over rounds reported);
peak memory is ``torch.cuda.max_memory_allocated`` above what was allocated before the call.  The
HIP path writes 5 B M N bytes with reward (1 B M N without) plus O(B (M + N)); its achieved write
bandwidth is those bytes over its time.  The outputs of both are compared before timing.

    python tools/bench_gt.py [--json out.json]

Needs a HIP device; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lgamd  # noqa: E402,F401
from lightglue_amd.gt_matcher import gt_matches_from_homography as hip_gt  # noqa: E402


def torch_gt(kp0, kp1, H, pos_th, neg_th, reward=True):
    """gt_generation.py:109-161 / homography.py:161-180 as written, on the device."""
    def warp(points, Hm):
        points = torch.cat([points, points.new_ones(points.shape[:-1] + (1,))], dim=-1)
        w = torch.einsum("...nj,...ji->...ni", points, Hm.transpose(-2, -1))
        return w[..., :-1] / (w[..., -1:] + 1e-5)

    kp0_1 = warp(kp0, H)
    kp1_0 = warp(kp1, torch.inverse(H))
    dist0 = torch.sum((kp0_1.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2, -1)
    dist1 = torch.sum((kp0.unsqueeze(-2) - kp1_0.unsqueeze(-3)) ** 2, -1)
    dist = torch.max(dist0, dist1)
    out = {}
    if reward:
        out["reward"] = (dist < pos_th**2).float() - (dist > neg_th**2).float()
    min0 = dist.min(-1).indices
    min1 = dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < pos_th**2)
    negative0 = dist0.min(-1).values > neg_th**2
    negative1 = dist1.min(-2).values > neg_th**2
    unmatched, ignore = min0.new_tensor(-1), min0.new_tensor(-2)
    m0 = torch.where(positive.any(-1), min0, ignore)
    m1 = torch.where(positive.any(-2), min1, ignore)
    m0 = torch.where(negative0, unmatched, m0)
    m1 = torch.where(negative1, unmatched, m1)
    out.update({"assignment": positive, "matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(),
                "matching_scores1": (m1 > -1).float(), "proj_0to1": kp0_1, "proj_1to0": kp1_0})
    return out


def make_inputs(B, M, N, seed, dev):
    rng = np.random.Generator(np.random.PCG64(seed))
    size = np.array([640.0, 480.0])
    H = np.tile(np.eye(3), (B, 1, 1))
    H[:, :2, :2] += rng.standard_normal((B, 2, 2)) * 0.05
    H[:, :2, 2] = rng.uniform(-30.0, 30.0, (B, 2))
    H[:, 2, :2] = rng.standard_normal((B, 2)) * 1e-4
    kp0 = rng.random((B, M, 2)) * size
    kp1 = rng.random((B, N, 2)) * size
    nw = min(N // 2, M)
    for b in range(B):
        ph = np.concatenate([kp0[b, :nw], np.ones((nw, 1))], 1) @ H[b].T
        kp1[b, :nw] = ph[:, :2] / ph[:, 2:] + rng.standard_normal((nw, 2)) * 1.5
    return tuple(torch.from_numpy(x.astype(np.float32)).to(dev) for x in (kp0, kp1, H))


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gt.py needs a HIP device")
    dev = torch.device("cuda", 0)
    pos, neg = 3.0, 3.0
    rows = []
    for B, M, N in ((32, 2048, 2048), (1, 1024, 1024)):
        kp0, kp1, H = make_inputs(B, M, N, 7, dev)
        for reward in (True, False):
            fns = {"hip": lambda: hip_gt(kp0, kp1, H, pos, neg, reward=reward),
                   "torch": lambda: torch_gt(kp0, kp1, H, pos, neg, reward=reward)}
            # same results first (near-ties aside: count the disagreements, do not hide them)
            oh, ot = fns["hip"](), fns["torch"]()
            diff = {k: int((oh[k] != ot[k]).sum()) for k in ("assignment", "matches0", "matches1")}
            if reward:
                diff["reward"] = int((oh["reward"] != ot["reward"]).sum())
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
            written = (5 if reward else 1) * B * M * N + B * (M + N) * (8 + 4 + 8)
            row = {"B": B, "M": M, "N": N, "reward": reward, "entries_differing": diff, "bytes_written_hip": written}
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
