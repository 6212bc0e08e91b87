#!/usr/bin/env python3
"""Throughput of the ALIKED extractor, with SuperPoint and the aliked + LightGlue pipeline for context.

Workload: ``aliked-n16`` on recipe weights, 480 x 640 synthetic images, top-k mode with k = 2048,
B = 16 images per forward.  Timed in one process with device events over windows of at least one
second, every shape warmed up first, the variants alternated three times:

  aliked        lightglue_amd.ALIKED, images/s, and the per-stage split of one forward (encoder /
                deformable blocks / aggregation + score head / DKD / SDDH, from the library's own
                stage events, sp_aliked_set_profile)
  superpoint    lightglue_amd.SuperPoint at the same shape and k, images/s
  aliked_lg     TwoViewPipeline(extractors.aliked, matchers.lightglue input_dim 128) on 32 pairs,
                pairs/s (two forwards of 16 pairs: 32 + 32 images through the extractor)

There is no baseline: the reference does not run on this device and earlier revisions have no
ALIKED.  The numbers are reported, nothing is asserted.  Also printed: the bytes the dense stage
moves per image (every map written once and read by its consumers, counted from the layer list)
against the 157 MB that the concatenated full-resolution feature map alone would take.

Prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lgamd  # noqa: E402,F401
from lightglue_amd import _lib  # noqa: E402
from lightglue_amd.aliked_weights import ALIKED_CFGS, aliked_state_dict  # noqa: E402
from lightglue_amd.sp_weights import superpoint_state_dict, synthetic_images  # noqa: E402

STAGES = ("encoder", "deformable_blocks", "head", "dkd", "sddh")


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
    return start.elapsed_time(stop) * 1e-3 / iters


def dense_bytes(model_name, H, W):
    """Bytes the dense stage reads and writes per image (fp32, padded size), map by map: each
    entry is (channels, level divisor, writes + reads)."""
    g = ALIKED_CFGS[model_name]
    c1, c2, c3, c4, dq = g["c1"], g["c2"], g["c3"], g["c4"], g["dim"] // 4
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    maps = [
        (3, 1, 1),                                    # image: read by block1.conv1
        (c1, 1, 2), (c1, 1, 3),                       # block1's two maps (x1: pool + conv1 1x1)
        (c1, 2, 3), (c2, 2, 2), (c2, 2, 2), (c2, 2, 3),   # pooled, downsample, block2's two maps
        (c2, 8, 4), (18, 8, 4), (c3, 8, 2), (c3, 8, 3), (c3, 8, 3),
        (c3, 32, 4), (c4, 32, 2), (c4, 32, 3), (c4, 32, 2),
        (dq, 1, 2), (dq, 2, 2), (dq, 8, 2), (dq, 32, 2),  # aggregated levels: written (with their score partials), read by the head
        (8, 1, 2), (8, 2, 2), (8, 8, 2), (8, 32, 2),      # score partials
        (8, 1, 2), (1, 1, 1), (4, 1, 2), (4, 1, 2), (1, 1, 1),  # S8, inverse norm, score head maps, score map
    ]
    total = sum(4 * c * (Hp // d) * (Wp // d) * n for c, d, n in maps)
    return {"dense_stage_bytes_per_image": int(total), "concatenated_map_bytes": int(4 * g["dim"] * Hp * Wp),
            "largest_map_bytes": int(4 * dq * Hp * Wp)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="aliked-n16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aliked", "bench_aliked.json"))
    args = ap.parse_args()
    from lightglue_amd import ALIKED, SuperPoint
    from lightglue_amd.pipeline import TwoViewPipeline
    from lightglue_amd.weights import synthetic_state_dict

    device = torch.device("cuda", 0)
    B, H, W, k = args.batch, args.height, args.width, args.keypoints

    def tsd(sd):
        return {n: torch.from_numpy(v.copy()) if v.ndim else torch.tensor(int(v)) for n, v in sd.items()}

    base = synthetic_images(4, 3, H, W, seed=7)
    images = torch.from_numpy(np.concatenate([base] * ((B + 3) // 4))[:B].copy()).to(device)
    gray = images.mean(1, keepdim=True).contiguous()
    econf = {"model_name": args.model, "max_num_keypoints": k, "detection_threshold": 0.0}
    aliked = ALIKED(econf).eval().to(device)
    aliked.load_state_dict(tsd(aliked_state_dict(args.model, seed=0)), strict=True)
    sp = SuperPoint({"max_num_keypoints": k, "force_num_keypoints": True, "detection_threshold": 0.0}).eval().to(device)
    sp.load_state_dict({n: torch.from_numpy(v) for n, v in superpoint_state_dict(None, seed=0).items()})
    pipe = TwoViewPipeline({"extractor": dict(econf, name="extractors.aliked"),
                            "matcher": {"name": "matchers.lightglue", "input_dim": ALIKED_CFGS[args.model]["dim"],
                                        "filter_threshold": 0.1}}).eval().to(device)
    pipe.extractor.load_state_dict(tsd(aliked_state_dict(args.model, seed=0)), strict=True)
    msd = synthetic_state_dict({"input_dim": ALIKED_CFGS[args.model]["dim"]}, seed=0)
    pipe.matcher.load_state_dict({n: torch.from_numpy(v) for n, v in msd.items()})
    size = torch.tensor([[float(W), float(H)]] * B, device=device)
    pair_data = {"view0": {"image": images, "image_size": size},
                 "view1": {"image": torch.roll(images, 1, 0).contiguous(), "image_size": size}}
    calls = max(1, args.pairs // B)

    def run_aliked():
        aliked({"image": images})

    def run_sp():
        sp({"image": gray})

    def run_pipe():
        for _ in range(calls):
            pipe(pair_data)

    variants = {"aliked": (run_aliked, B), "superpoint": (run_sp, B), "aliked_lg": (run_pipe, calls * B)}
    rates = {n: [] for n in variants}
    with torch.no_grad():
        for fn, _ in variants.values():
            fn()
            fn()
        torch.cuda.synchronize(device)
        for _ in range(args.repeats):
            for name, (fn, items) in variants.items():
                rates[name].append(items / timed(fn, device, args.window))
        lib = _lib.load()
        _lib.check(lib.sp_aliked_set_profile(aliked._handle, 1), "sp_aliked_set_profile")
        ms = (ctypes.c_float * 5)()
        stage = np.zeros(5)
        reps = 5
        for _ in range(reps):
            run_aliked()
            _lib.check(lib.sp_aliked_stage_ms(aliked._handle, ms), "sp_aliked_stage_ms")
            stage += np.asarray(list(ms))
        _lib.check(lib.sp_aliked_set_profile(aliked._handle, 0), "sp_aliked_set_profile")
    result = {"workload": {"model": args.model, "batch": B, "height": H, "width": W, "keypoints": k, "pairs": calls * B},
              "device": torch.cuda.get_device_name(device), "window_s": args.window}
    for name, r in rates.items():
        result[name] = {"unit": "pairs/s" if name == "aliked_lg" else "images/s", "repeats": [round(x, 2) for x in r],
                        "mean": round(float(np.mean(r)), 2), "spread": round(float((max(r) - min(r)) / np.mean(r)), 4)}
    result["aliked_stage_ms_per_forward"] = {s: round(float(v / reps), 3) for s, v in zip(STAGES, stage)}
    result.update(dense_bytes(args.model, H, W))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
