#!/usr/bin/env python3
"""GlueStick forward on one MI355X: the HIP path against the fp32 torch restatement on the same GPU.

    python tools/bench_gluestick.py [--batches 32,1] [--rounds R] [--window S] [--out profiles/gluestick/bench_gluestick.json]

Shapes are the reference's training config for the wireframe pipeline: 1000 points + 500 junction
slots per image (1500 keypoints), 250 lines, the default 18 GNN layers, one line iteration; B = 32
(training / batched evaluation) and B = 1 (the eval configs).  Inputs come from the seeded wireframe
generator and are resident in HBM; weights are the recipe's.

Per batch size: the HIP forward, the restatement (tests/gluestick_ref.py, fp32, every op a torch-ROCm
kernel) in the same process, and a split of the HIP forward by whole-forward differences --
``lines`` = full minus the same weights with ``num_line_iterations = 0``, ``trunk`` = that minus a
model without GNN layers, ``encoders_heads`` = the model without GNN layers (both encoders, the final
projections, both double-softmax heads and filters; its line head still runs).  Times are host clocks
around a device synchronise: every arm is warmed up, its repetitions are sized to a window of about
``--window`` seconds, and ``--rounds`` rounds time the four arms one after the other; the median per
arm is reported with its minimum and maximum.  The outputs of the two paths are compared so that the
speed-up is over equal results.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgamd  # noqa: E402,F401
from gluestick_ref import gluestick_forward  # noqa: E402
from lightglue_amd import GlueStick  # noqa: E402
from lightglue_amd.gs_weights import gluestick_state_dict, wireframe_pair  # noqa: E402

POINTS, JUNCTIONS, LINES, SIZE = 1000, 500, 250, (640, 480)
INPUTS = ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "keypoint_scores0", "keypoint_scores1", "lines0",
          "lines1", "lines_junc_idx0", "lines_junc_idx1", "line_scores0", "line_scores1")


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def timed_arms(arms, rounds, seconds):
    """Every arm warmed up, its repetitions sized so that one window lasts about ``seconds``; then
    ``rounds`` rounds that time the arms one after the other, so drift hits all of them alike.
    Returns {name: (median s, min s, max s, reps per window, last output)}."""
    reps, out = {}, {}
    for name, fn in arms.items():
        window(fn, 3)
        t, _ = window(fn, 3)
        reps[name] = max(3, int(seconds / t))
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            t, out[name] = window(fn, reps[name])
            times[name].append(t)
    return {n: (float(np.median(v)), min(v), max(v), reps[n], out[n]) for n, v in times.items()}


def model_for(conf, sd, dev):
    m = GlueStick(conf).eval().to(dev)
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k in own}, strict=True)
    return m


def run(B, rounds, seconds, dev):
    pair = wireframe_pair(B, (JUNCTIONS, JUNCTIONS), (POINTS, POINTS), (LINES, LINES), seed=7, width=SIZE[0], height=SIZE[1])
    sd = gluestick_state_dict({}, seed=0, proj_gain=15.0)
    size = torch.tensor([SIZE] * B, dtype=torch.float32, device=dev)
    data = {k: torch.from_numpy(pair[k]).to(dev) for k in INPUTS}
    data["view0"] = data["view1"] = {"image_size": size}
    ref_data = {**{k: data[k] for k in INPUTS}, "image_size0": size, "image_size1": size}
    sd_dev = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}
    full = model_for({}, sd, dev)
    no_lines = model_for({"num_line_iterations": 0}, sd, dev)
    no_gnn = model_for({"GNN_layers": []}, sd, dev)
    arms = {"hip": lambda: full(data), "hip_no_lines": lambda: no_lines(data), "hip_no_gnn": lambda: no_gnn(data),
            "torch_fp32": lambda: gluestick_forward(sd_dev, ref_data, {}, torch.float32, dev)}
    with torch.no_grad():
        r = timed_arms(arms, rounds, seconds)
    pred, ref = r["hip"][4], r["torch_fp32"][4]
    same0 = float((pred["matches0"] == ref["matches0"]).float().mean())
    same_l = float((pred["line_matches0"] == ref["line_matches0"]).float().mean())
    err = float((pred["log_assignment"] - ref["log_assignment"]).abs().max())
    ms = {n: {"median": round(1e3 * v[0], 3), "min": round(1e3 * v[1], 3), "max": round(1e3 * v[2], 3),
              "reps_per_window": v[3]} for n, v in r.items()}
    t_full, t_nl, t_ng, t_ref = (r[n][0] for n in ("hip", "hip_no_lines", "hip_no_gnn", "torch_fp32"))
    return {
        "config": f"GlueStick eval forward, B={B}, {POINTS}+{JUNCTIONS} keypoints, {LINES} lines, 18 layers, 1 GPU",
        "hip_ms": round(1e3 * t_full, 3), "torch_fp32_ms": round(1e3 * t_ref, 3), "speedup": round(t_ref / t_full, 2),
        "pairs_per_s": round(B / t_full, 2),
        # medians over `rounds` alternated windows of about `window_s` each; min / max are the spread
        "arms_ms": ms, "rounds": rounds, "window_s": seconds,
        "split_ms": {"trunk": round(1e3 * (t_nl - t_ng), 3), "lines": round(1e3 * (t_full - t_nl), 3),
                     "encoders_heads": round(1e3 * t_ng, 3)},
        "matches": int((pred["matches0"] > -1).sum()), "line_matches": int((pred["line_matches0"] > -1).sum()),
        "matches0_equal_fraction": round(same0, 5), "line_matches0_equal_fraction": round(same_l, 5),
        "log_assignment_max_abs_diff": err,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window of an arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gluestick", "bench_gluestick.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gluestick.py needs a HIP device: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    rows = []
    for B in (int(b) for b in a.batches.split(",")):
        rows.append(run(B, a.rounds, a.window, dev))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
