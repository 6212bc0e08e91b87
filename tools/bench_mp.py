#!/usr/bin/env python3
"""Time `mp: true` (fp16 GEMMs + fp16 attention, DESIGN.md §5 "fp16 GEMMs") against `flash: true` and the
default on the same box, in the same process, from the same weights.

Shapes, protocol and timing are tools/bench_flash.py's: configs[2] (N = 2048, B = 32, 9 layers), B = 1
N = 1024, and B = 1 N = 2048 with pruning on (width = depth = 0.95); 2 warm-up forwards, then the shape's
repetitions back to back between two HIP events; the three models alternate in ``--rounds`` rounds.

The GEMM-family and attention time per forward come from a SEPARATE run of each model under ``rocprofv3
--kernel-trace --stats`` (no counters): with ``--trace`` this script starts one fresh child per (model,
shape) -- ``--forwards MODEL --shape NAME`` is that child's mode -- and sums the kernel durations by family.

    python tools/bench_mp.py [--trace] [--json profiles/mp/bench_mp.json]

Acceptance (recorded under "acceptance"): at configs[2] `mp: true` reads more pairs/s than `flash: true` in
every round.  The two B = 1 shapes are reported as measured.  Needs a HIP device; there is no CPU fallback.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lgamd  # noqa: E402,F401
from bench import BF16_MFMA_PEAK_TFLOPS  # noqa: E402
from bench_flash import ATTN_KERNELS, SHAPES, inputs_for, timed  # noqa: E402
from lightglue_amd import LightGlue  # noqa: E402
from lightglue_amd.weights import prune_recipe_state_dict, synthetic_state_dict  # noqa: E402

MODELS = {"plain": {}, "flash": {"flash": True}, "mp": {"mp": True}}
GEMM_KERNELS = ("gemm_h3_kernel",)


def model_for(shape, which, dev):
    _, _, over, weights, _, _ = SHAPES[shape]
    conf = {"filter_threshold": 0.1, **MODELS[which], **over}
    sd = prune_recipe_state_dict(conf) if weights == "prune_recipe" else synthetic_state_dict({"filter_threshold": 0.1}, seed=0)
    m = LightGlue(conf).eval().to(dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def trunk_gemm_flops_per_forward(B, N, layers=9, d=256):
    # per layer and block (self, cross) and row: QKV (d x 3d or d x 2d), ffn.0 (2d x 2d), ffn.3 (2d x d)
    per_row = (3 * d * d + 4 * d * d + 2 * d * d) + (2 * d * d + 4 * d * d + 2 * d * d)
    return 2.0 * layers * per_row * 2 * B * N


def run_forwards(shape, which, n):
    """Child mode of --trace: n forwards of one model, nothing else."""
    dev = torch.device("cuda", 0)
    m, data = model_for(shape, which, dev), inputs_for(shape, dev)
    with torch.no_grad():
        for _ in range(n):
            m(data)
    torch.cuda.synchronize()
    print(json.dumps({"shape": shape, "model": which, "forwards": n, "precision": m.last_precision_used}))


def traced_ms(shape, which, n, timeout):
    """GEMM-family and attention kernels' summed time per forward (ms) from a rocprofv3 kernel trace of a child."""
    out = tempfile.mkdtemp(prefix="bench_mp_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--forwards", which, "--shape", shape, "--n", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"traced child failed ({r.returncode}):\n{r.stdout[-2000:]}")
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel trace written")
        tot = {"gemm": 0, "gemm_h1": 0, "attention": 0, "all": 0}
        for row in csv.DictReader(open(files[0])):
            dt = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            name = row["Kernel_Name"]
            tot["all"] += dt
            if any(k in name for k in GEMM_KERNELS):
                tot["gemm"] += dt
                if ", true>" in name or "Lb1E" in name:  # the H1 instantiations
                    tot["gemm_h1"] += dt
            elif any(k in name for k in ATTN_KERNELS):
                tot["attention"] += dt
        return {k + "_ms_per_forward": round(v * 1e-6 / n, 4) for k, v in tot.items()}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=0, help="forwards per timing (0: the shape's default)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--trace", action="store_true", help="also trace each model under rocprofv3 (separate children)")
    ap.add_argument("--trace-timeout", type=int, default=150)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "mp", "bench_mp.json"))
    ap.add_argument("--forwards", choices=list(MODELS), help="child mode: run --n forwards of one model and exit")
    ap.add_argument("--shape", default="configs2")
    ap.add_argument("--n", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mp.py needs a HIP device")
    if a.forwards:
        return run_forwards(a.shape, a.forwards, a.n)
    dev = torch.device("cuda", 0)
    rows = []
    for shape in a.shapes.split(","):
        B, N, over, _, _, reps = SHAPES[shape]
        reps = a.reps or reps
        models = {k: model_for(shape, k, dev) for k in MODELS}
        data = inputs_for(shape, dev)
        rate = {k: [] for k in models}
        with torch.no_grad():
            for _ in range(a.rounds):  # alternate the three in every round
                for k, m in models.items():
                    rate[k].append(B / timed(lambda m=m: m(data), reps))
            preds = {k: m(data) for k, m in models.items()}
        torch.cuda.synchronize()
        row = {"shape": shape, "B": B, "N": N, "conf": over, "reps": reps,
               "precision": {k: m.last_precision_used for k, m in models.items()},
               "pairs_per_s": {k: [round(x, 2) for x in v] for k, v in rate.items()},
               "matches_image0": {k: int((p["matches0"] > -1).sum()) for k, p in preds.items()},
               "same_matches_image0_as_plain": {k: float((preds["plain"]["matches0"] == preds[k]["matches0"]).float().mean())
                                                for k in ("flash", "mp")},
               "mp_over_flash_per_round": [round(m / f, 4) for f, m in zip(rate["flash"], rate["mp"])],
               "mp_over_plain_per_round": [round(m / p, 4) for p, m in zip(rate["plain"], rate["mp"])]}
        row["mp_faster_than_flash_every_round"] = all(m > f for f, m in zip(rate["flash"], rate["mp"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del models, preds
    if a.trace:
        for row in rows:
            tr = {k: traced_ms(row["shape"], k, a.n, a.trace_timeout) for k in MODELS}
            row["rocprofv3_kernel_trace"] = tr
            row["gemm_time_ratio_flash_over_mp"] = round(tr["flash"]["gemm_ms_per_forward"] / tr["mp"]["gemm_ms_per_forward"], 4)
            if not row["conf"]:  # unpruned: every layer runs every row
                fl = trunk_gemm_flops_per_forward(row["B"], row["N"])
                tf = fl / (tr["mp"]["gemm_h1_ms_per_forward"] * 1e-3) / 1e12
                row["mp_trunk_gemm_tflops"] = round(tf, 1)
                row["fraction_of_dense_fp16_mfma_peak"] = round(tf / BF16_MFMA_PEAK_TFLOPS, 4)
                row["peak_note"] = f"dense fp16 MFMA peak {BF16_MFMA_PEAK_TFLOPS:.0f} TFLOP/s (MI355X, 256 CUs at 2.4 GHz)"
            print(json.dumps(row), flush=True)
    res = {"tool": "tools/bench_mp.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": rows,
           "acceptance": {"configs2_mp_faster_than_flash_every_round":
                          next((r["mp_faster_than_flash_every_round"] for r in rows if r["shape"] == "configs2"), None)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": os.path.relpath(a.json, ROOT), "acceptance": res["acceptance"]}))


if __name__ == "__main__":
    main()
