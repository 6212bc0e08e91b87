#!/usr/bin/env python3
"""Time the batched hybrid point-and-line robust homography estimation (lightglue_amd.robust: one launch
of ``lg_ransac_homography_lines`` for every pair of a batch).

Shape: 32 pairs with 600 point matches and 250 line matches each (GlueStick's training line count), half
of each on the pair's homography with 0.7 px of noise and half anywhere, at the thresholds 2.0 and 0.5 px
(``max_iters`` 3000, confidence 0.995, the defaults).  Times are HIP-event times per batch over ``--iters``
back-to-back batches after ``--warmup`` batches, in ``--rounds`` rounds (median and min..max over
rounds); the mean number of rounds of 256 hypotheses, the success rate and the inlier counts come from
the call's ``info``.  For context the same process runs ``lg_ransac_homography`` on the point part alone
(a different, cheaper minimal problem).  There is no baseline on the same machine: the reference's
estimator is the external ``homography_est`` library, which is not installed where this project runs.

The last row splits a round of 256 hypotheses into solving and scoring: features with no model behind
them never stop the run (confidence 0.999999), so runs of 16 and of 48 rounds are timed with all 850
features and with 32 + 32 of them.  The slope between the two lengths is the cost of a round without
phase 0, the result and (nearly all of) the local optimisations; the difference between the two feature
sets is the scoring of the other 786 features, scaled to 850.

    python tools/bench_ransac_lines.py [--json profiles/ransac_lines/bench_ransac_lines.json]

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

W, HH = 640.0, 480.0


def warp(H, p):
    q = torch.cat([p, torch.ones_like(p[..., :1])], -1) @ H.transpose(-1, -2)
    return q[..., :2] / q[..., 2:]


def make_inputs(B, n_points, n_lines, ratio, seed, dev):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    size = torch.tensor([W, HH], dtype=torch.float64)
    H = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    H[:, :2, :2] += 0.1 * (u(B, 2, 2) - 0.5)
    H[:, :2, 2] = 40 * (u(B, 2) - 0.5)
    H[:, 2, :2] = 1e-4 * (u(B, 2) - 0.5)
    k0 = u(B, n_points, 2) * size
    k1 = warp(H, k0) + 0.7 * n(B, n_points, 2)
    a = u(B, n_lines, 1, 2) * (size - 130) + 20
    l0 = torch.cat([a, a + 30 + 60 * u(B, n_lines, 1, 2)], 2)
    l1 = warp(H[:, None], l0) + 0.7 * n(B, n_lines, 2, 2)
    bad_p, bad_l = n_points - int(round(n_points * ratio)), n_lines - int(round(n_lines * ratio))
    k1[:, :bad_p] = u(B, bad_p, 2) * size
    b = u(B, bad_l, 1, 2) * (size - 130) + 20
    l1[:, :bad_l] = torch.cat([b, b + 30 + 60 * u(B, bad_l, 1, 2)], 2)
    f = lambda x: x.float().to(dev).contiguous()  # noqa: E731
    return {"kpts0": f(k0), "kpts1": f(k1), "lines0": f(l0), "lines1": f(l1), "H_gt": f(H), "size0": f(size.repeat(B, 1))}


def time_calls(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(fn, a):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    v = [time_calls(fn, a.iters) for _ in range(a.rounds)]
    return {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "ransac_lines", "bench_ransac_lines.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ransac_lines.py needs a HIP device")
    dev = torch.device("cuda", 0)
    B, n_points, n_lines, ratio = 32, 600, 250, 0.5
    d = make_inputs(B, n_points, n_lines, ratio, 7, dev)
    common = {"B": B, "point_matches_per_pair": n_points, "line_matches_per_pair": n_lines, "inlier_ratio": ratio,
              "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds}
    o = robust.PointLineHomographyEstimator.default_conf["options"]
    rows = []
    for th in (2.0, 0.5):
        run = lambda: robust.ransac_homography_lines(  # noqa: E731
            d["kpts0"], d["kpts1"], None, d["lines0"], d["lines1"], None, th, H_gt=d["H_gt"], image_size0=d["size0"], **o)
        pts = lambda: robust.ransac_homography(  # noqa: E731
            d["kpts0"], d["kpts1"], None, th, H_gt=d["H_gt"], image_size0=d["size0"])
        r, p = run(), pts()
        info, pinfo = r["info"].cpu().float(), p["info"].cpu().float()
        row = {**common, "ransac_th": th, **o, "ms_per_batch": measure(run, a),
               "rounds_per_pair": float(info[:, 7].mean()), "success_rate": float(info[:, 0].mean()),
               "mean_point_inliers": float(info[:, 3].mean()), "mean_line_inliers": float(info[:, 4].mean()),
               "mean_valid_hypotheses_per_round": float((info[:, 8] / info[:, 7].clamp(min=1)).mean()),
               "median_H_error_ransac": float(r["H_error"].cpu().median()),
               "points_alone_lg_ransac_homography": {
                   "ms_per_batch": measure(pts, a), "rounds_per_pair": float(pinfo[:, 5].mean()),
                   "mean_inliers": float(pinfo[:, 2].mean()), "median_H_error_ransac": float(p["H_error"].cpu().median())}}
        row["pairs_per_s"] = 1e3 * B / row["ms_per_batch"]["ms_median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the solve / score split of a round: runs that cannot stop, 16 and 48 rounds, all features against 32 + 32
    n = make_inputs(B, n_points, n_lines, 0.0, 8, dev)
    split = {**common, "what": "round split", "rounds_timed": [16, 48], "ransac_th": 0.5}
    per_round = {}
    for name, kp, kl in (("all_features", n_points, n_lines), ("few_features", 32, 32)):
        c = torch.full((B,), kp, dtype=torch.int32, device=dev), torch.full((B,), kl, dtype=torch.int32, device=dev)
        split[name] = {}
        for n_rounds in (16, 48):
            run = lambda: robust.ransac_homography_lines(  # noqa: E731
                n["kpts0"], n["kpts1"], None, n["lines0"], n["lines1"], None, 0.5, c[0], c[0], c[1], c[1],
                max_iters=256 * n_rounds, confidence=0.999999, seed=0)
            info = run()["info"].cpu()
            assert (info[:, 7] == n_rounds).all(), "the split's runs must not stop early"
            split[name][f"rounds_{n_rounds}"] = {**measure(run, a), "mean_valid_hypotheses_per_round":
                                                 float((info[:, 8].float() / n_rounds).mean())}
        per_round[name] = (split[name]["rounds_48"]["ms_median"] - split[name]["rounds_16"]["ms_median"]) / 32
        split[name]["ms_per_round"] = per_round[name]
    K, few = n_points + n_lines, 64
    per = (per_round["all_features"] - per_round["few_features"]) / (K - few)
    split["ms_per_round_score"] = per * K
    split["ms_per_round_solve"] = per_round["few_features"] - per * few
    print(json.dumps(split), flush=True)
    rows.append(split)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
