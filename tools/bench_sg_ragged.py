#!/usr/bin/env python3
"""Throughput of a ragged SuperGlue batch (data["num_keypoints0/1"]) against the two alternatives.

Workload: one seeded set of 32 pairs at capacity 2048 with counts uniform in [1024, 2048] per
image, the default SuperGlue (18 GNN layers, 50 Sinkhorn iterations) on seeded random weights.
Three variants, timed in one process with device events over windows of at least one second, every
shape warmed up first, and alternated three times:

  ragged    one forward over the whole batch with the per-pair counts
  per_pair  the same pairs one per forward at their own sizes (the only exact alternative without
            counts: padding changes the attention, the Sinkhorn marginals and the mutual filter)
  uniform   for context, 32 x 2048 with every slot full

Prints one JSON line and writes it to --out (pairs/s per repeat, mean, and the spread
(max - min) / mean of the repeats).  The feature has delivered when ragged exceeds per_pair by
more than the spread of the repeats."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lgamd  # noqa: E402,F401
from lightglue_amd import SuperGlue  # noqa: E402
from lightglue_amd.sg_weights import superglue_state_dict, synthetic_scores  # noqa: E402
from lightglue_amd.weights import synthetic_pair  # noqa: E402


def timed(fn, device, min_seconds):
    """Seconds per call of fn over a window of at least min_seconds (device events)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize(device)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize(device)
    once = max(start.elapsed_time(stop) * 1e-3, 1e-6)
    iters = max(2, int(np.ceil(min_seconds / once)) + 1)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize(device)
    total = start.elapsed_time(stop) * 1e-3
    assert total >= 0.5 * min_seconds, (total, min_seconds)
    return total / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--capacity", type=int, default=2048)
    ap.add_argument("--min-count", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sg_ragged", "bench_sg_ragged.json"))
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    B, cap = args.batch, args.capacity
    conf = {"weights": None}
    model = SuperGlue(conf).eval().to(device)
    full = model.state_dict()
    full.update({k: torch.from_numpy(np.asarray(v).copy()) for k, v in superglue_state_dict(conf, seed=0).items()})
    model.load_state_dict(full, strict=True)
    data = synthetic_pair(B=B, M=cap, N=cap, seed=args.seed, width=640, height=480)
    data["keypoint_scores0"] = synthetic_scores(B, cap, seed=args.seed + 1)
    data["keypoint_scores1"] = synthetic_scores(B, cap, seed=args.seed + 2)
    rng = np.random.Generator(np.random.PCG64(args.seed))
    n0 = rng.integers(args.min_count, cap + 1, B)
    n1 = rng.integers(args.min_count, cap + 1, B)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    keys = ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "keypoint_scores0", "keypoint_scores1")
    size = np.tile([[640.0, 480.0]], (B, 1)).astype(np.float32)
    uniform = {k: dev(data[k]) for k in keys}
    uniform["view0"] = {"image_size": dev(size)}
    uniform["view1"] = {"image_size": dev(size)}
    ragged = dict(uniform, num_keypoints0=dev(n0.astype(np.int32)), num_keypoints1=dev(n1.astype(np.int32)))
    singles = []
    for b in range(B):
        one = {k: dev(data[k][b:b + 1, :(n0[b] if k.endswith("0") else n1[b])]) for k in keys}
        one["view0"] = {"image_size": dev(size[b:b + 1])}
        one["view1"] = {"image_size": dev(size[b:b + 1])}
        singles.append(one)

    def run_ragged():
        model(ragged)

    def run_per_pair():
        for one in singles:
            model(one)

    def run_uniform():
        model(uniform)

    variants = {"ragged": run_ragged, "per_pair": run_per_pair, "uniform": run_uniform}
    rates = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():  # warm-up of every shape (workspace growth, lazy init)
            fn()
            fn()
        torch.cuda.synchronize(device)
        # the ragged forward and the single-pair forwards agree (a cheap guard on what is timed)
        pr = model(ragged)
        for b in (0, B - 1):
            ps = model(singles[b])
            same = (pr["matches0"][b, :n0[b]] == ps["matches0"][0]).float().mean().item()
            assert same > 0.99, (b, same)
        for _ in range(args.repeats):
            for name, fn in variants.items():
                rates[name].append(B / timed(fn, device, args.window))
    result = {"workload": {"pairs": B, "capacity": cap, "counts": [args.min_count, cap], "seed": args.seed,
                           "mean_count": float(np.concatenate([n0, n1]).mean()), "gnn_layers": len(model.conf.GNN_layers),
                           "sinkhorn_iterations": int(model.conf.num_sinkhorn_iterations)},
              "device": torch.cuda.get_device_name(device), "window_s": args.window, "unit": "pairs/s"}
    for name, r in rates.items():
        result[name] = {"repeats": [round(x, 2) for x in r], "mean": round(float(np.mean(r)), 2),
                        "spread": round(float((max(r) - min(r)) / np.mean(r)), 4)}
    result["ragged_over_per_pair"] = round(result["ragged"]["mean"] / result["per_pair"]["mean"], 3)
    result["delivered"] = bool(min(rates["ragged"]) > max(rates["per_pair"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
