#!/usr/bin/env python3
"""Time `flash: true` (fp16 attention, DESIGN.md §5 "fp16 attention") against `flash: false` on the
same box, in the same process, from the same weights.

Shapes: configs[2] (N = 2048, B = 32, 9 layers), B = 1 N = 1024, and B = 1 N = 2048 with pruning
on (width = depth = 0.95, the configs[3] weights).  Protocol of tools/bench_configs.py (2 warm-up
forwards, then ``--reps`` forwards back to back), timed with HIP events around the forwards, the two
models alternating in ``--rounds`` rounds; the profiler stays off.

The attention kernels' summed time per forward comes from a SEPARATE run of each model under
``rocprofv3 --kernel-trace --stats`` (no counters): with ``--attn-trace`` this script starts one
fresh child per (model, shape) -- ``--forwards MODEL --shape NAME`` is that child's mode -- and
sums the durations of the attention kernels (attention_h3g_kernel, attn_split_combine_kernel) in
its kernel trace.

    python tools/bench_flash.py [--attn-trace] [--json profiles/flash/bench_flash.json]

Acceptance (recorded under "acceptance"): at configs[2] `flash: true` is faster in every round; at
the two B = 1 shapes it is not slower than `flash: false` by more than the spread of that shape's
own `flash: false` rounds.  Needs a HIP device; there is no CPU fallback.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgamd  # noqa: E402,F401
from bench import BF16_MFMA_PEAK_TFLOPS, gpu_pairs  # noqa: E402
from lightglue_amd import LightGlue  # noqa: E402
from lightglue_amd.weights import prune_recipe_state_dict, synthetic_state_dict  # noqa: E402

PRUNE = {"width_confidence": 0.95, "depth_confidence": 0.95}
# name -> (B, N, conf overrides, weights, keypoint extent, default reps)
SHAPES = {
    "configs2": (32, 2048, {}, "synthetic", (640.0, 640.0), 10),
    "b1_n1024": (1, 1024, {}, "synthetic", (640.0, 640.0), 50),
    "b1_n2048_pruned": (1, 2048, PRUNE, "prune_recipe", (1600.0, 1200.0), 30),
}
ATTN_KERNELS = ("attention_h3g_kernel", "attn_split_combine_kernel", "attention_h3m_kernel", "attention_x6_kernel")


def model_for(shape, flash, dev):
    _, _, over, weights, _, _ = SHAPES[shape]
    conf = {"filter_threshold": 0.1, "flash": flash, **over}
    sd = prune_recipe_state_dict(conf) if weights == "prune_recipe" else synthetic_state_dict({"filter_threshold": 0.1}, seed=0)
    m = LightGlue(conf).eval().to(dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def inputs_for(shape, dev):
    B, N, _, _, size, _ = SHAPES[shape]
    return gpu_pairs(B, N, 256, seed=1 if B > 1 or N == 1024 else 3, device=dev, size=size)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def attention_flops_per_forward(B, N, layers=9, heads=4, hd=64):
    # per layer four attention sets (self x 2 images, cross x 2 directions), each Q K^T and P V
    return layers * 4 * 2 * 2.0 * B * heads * N * N * hd


def run_forwards(shape, flash, n):
    """Child mode of --attn-trace: n forwards of one model, nothing else."""
    dev = torch.device("cuda", 0)
    m, data = model_for(shape, flash, dev), inputs_for(shape, dev)
    with torch.no_grad():
        for _ in range(n):
            m(data)
    torch.cuda.synchronize()
    print(json.dumps({"shape": shape, "flash": flash, "forwards": n, "precision": m.last_precision_used}))


def traced_attention_ms(shape, flash, n, timeout):
    """Attention kernels' summed time per forward (ms) from a rocprofv3 kernel trace of a child."""
    out = tempfile.mkdtemp(prefix="bench_flash_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--forwards", "flash" if flash else "plain", "--shape", shape,
               "--n", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"traced child failed ({r.returncode}):\n{r.stdout[-2000:]}")
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel trace written")
        tot, launches = 0, 0
        for row in csv.DictReader(open(files[0])):
            if any(k in row["Kernel_Name"] for k in ATTN_KERNELS):
                tot += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                launches += 1
        return {"attention_ms_per_forward": tot * 1e-6 / n, "attention_launches_per_forward": launches / n}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=0, help="forwards per timing (0: the shape's default)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--attn-trace", action="store_true", help="also trace each model under rocprofv3 (separate children)")
    ap.add_argument("--trace-timeout", type=int, default=150)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "flash", "bench_flash.json"))
    ap.add_argument("--forwards", choices=["plain", "flash"], help="child mode: run --n forwards of one model and exit")
    ap.add_argument("--shape", default="configs2")
    ap.add_argument("--n", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flash.py needs a HIP device")
    if a.forwards:
        return run_forwards(a.shape, a.forwards == "flash", a.n)
    dev = torch.device("cuda", 0)
    rows = []
    for shape in a.shapes.split(","):
        B, N, over, _, _, reps = SHAPES[shape]
        reps = a.reps or reps
        models = {"plain": model_for(shape, False, dev), "flash": model_for(shape, True, dev)}
        data = inputs_for(shape, dev)
        rate = {k: [] for k in models}
        with torch.no_grad():
            for _ in range(a.rounds):  # alternate the two in every round
                for k, m in models.items():
                    rate[k].append(B / timed(lambda m=m: m(data), reps))
            preds = {k: m(data) for k, m in models.items()}
        torch.cuda.synchronize()
        row = {"shape": shape, "B": B, "N": N, "conf": over, "reps": reps,
               "precision": {k: m.last_precision_used for k, m in models.items()},
               "pairs_per_s": {k: [round(x, 2) for x in v] for k, v in rate.items()},
               "matches_image0": {k: int((p["matches0"] > -1).sum()) for k, p in preds.items()},
               "same_matches_image0": float((preds["plain"]["matches0"] == preds["flash"]["matches0"]).float().mean())}
        spread = max(rate["plain"]) - min(rate["plain"])
        row["plain_spread_pairs_per_s"] = round(spread, 2)
        row["speedup_per_round"] = [round(f / p, 4) for p, f in zip(rate["plain"], rate["flash"])]
        if B > 1:
            row["accepted"] = all(f > p for p, f in zip(rate["plain"], rate["flash"]))
        else:
            row["accepted"] = all(f >= p - spread for p, f in zip(rate["plain"], rate["flash"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del models, preds
    if a.attn_trace:
        for row in rows:
            tr = {k: traced_attention_ms(row["shape"], k == "flash", a.n, a.trace_timeout) for k in ("plain", "flash")}
            row["rocprofv3_kernel_trace"] = tr
            row["attention_time_ratio"] = round(tr["plain"]["attention_ms_per_forward"] / tr["flash"]["attention_ms_per_forward"], 4)
            if not row["conf"]:  # unpruned: every layer runs every key
                fl = attention_flops_per_forward(row["B"], row["N"])
                tf = fl / (tr["flash"]["attention_ms_per_forward"] * 1e-3) / 1e12
                row["flash_attention_tflops"] = round(tf, 1)
                row["fraction_of_dense_fp16_mfma_peak"] = round(tf / BF16_MFMA_PEAK_TFLOPS, 4)
                row["peak_note"] = f"dense fp16 MFMA peak {BF16_MFMA_PEAK_TFLOPS:.0f} TFLOP/s (MI355X, 256 CUs at 2.4 GHz)"
            print(json.dumps(row), flush=True)
    res = {"tool": "tools/bench_flash.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": rows,
           "acceptance": {r["shape"]: r["accepted"] for r in rows}}
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": os.path.relpath(a.json, ROOT), "acceptance": res["acceptance"]}))


if __name__ == "__main__":
    main()
