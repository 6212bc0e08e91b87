#!/usr/bin/env python3
"""Per-tensor gradient accuracy of the HIP training step on a gradient golden (GPU box):

    python tools/grad_route_report.py <golden name> [--json out.json]

For every parameter (and the descriptor gradients): the GPU's max |g - g64| against the float64
oracle, the reference's own float32 spread (stored in the golden) and the float32 ORACLE's spread
(another plain fp32 implementation of the same step), the test bar 8 * spread32_ref + 1e-6 * max,
and err / bar (the tests' bar: 8 x the larger of the reference's and the oracle's float32
spreads; also against the reference's spread alone).  Each training product has one route; build a
variant library and point LIGHTGLUE_MI355X_LIB at it to see which change moves which tensor.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name")
    ap.add_argument("--json")
    a = ap.parse_args()
    from grad_golden_util import desc_golden, desc_pick

    rows = []
    if a.name.startswith("sgtrain_"):
        from sg_grad_golden_util import load_sgtrain, oracle_sg_step, sgtrain_case
        from test_gpu_sg_train import gpu_step

        g, meta = load_sgtrain(a.name)
        conf, sd, data, gt = sgtrain_case(meta)
        from oracle.superglue_train_ref import ReluMasks

        loss, grads, gd0, gd1, bufs, _, _ = gpu_step(conf, sd, data, gt)
        # the float64 / float32 oracle on the HIP forward's ReLU decisions (test_gpu_sg_train.py)
        relu = ReluMasks({k: [m.cpu() for m in v] for k, v in gpu_step.relu_masks.items()})
        _, og, od0, od1, _, _ = oracle_sg_step(conf, sd, data, gt, relu=relu)
        print("ReLU decisions differing from float64's (bn, image, |v64|):", relu.flips[:12])
        _, og32, o32d0, o32d1, _, _ = oracle_sg_step(
            conf, sd, data, gt, dtype=torch.float32,
            relu=ReluMasks({k: [m.cpu() for m in v] for k, v in gpu_step.relu_masks.items()}))
    else:
        from grad_golden_util import grad_case, load_grad, oracle_grads
        from test_gpu_train import _gpu_grads

        g, meta = load_grad(a.name)
        conf, sd, pair, gt = grad_case(meta)
        loss, grads, gd0, gd1, _ = _gpu_grads(conf, sd, pair, gt)
        _, og, od0, od1 = oracle_grads(conf, sd, pair, gt)
        _, og32, o32d0, o32d1 = oracle_grads(conf, sd, pair, gt, dtype=torch.float32)
    for n in meta["names"]:
        r64 = og[n].reshape(-1)
        mx = float(g[f"max64:{n}"])
        bar = 8 * float(g[f"spread32:{n}"]) + 1e-6 * mx + 1e-12
        diff = np.abs(grads[n].reshape(-1) - r64)
        err = float(diff.max())
        at = [int(i) for i in np.unravel_index(int(diff.argmax()), og[n].shape)]
        o32 = float(np.abs(og32[n].reshape(-1) - r64).max())
        bar2 = 8 * max(float(g[f"spread32:{n}"]), o32) + 1e-6 * mx + 1e-12
        rows.append({"tensor": n, "max64": mx, "err_gpu": err, "spread_ref32": float(g[f"spread32:{n}"]),
                     "spread_oracle32": o32, "bar": bar, "ratio_ref_bar": err / bar, "bar_tests": bar2,
                     "ratio": err / bar2, "argmax": at})
    for got, ref, r32, key in ((gd0, od0, o32d0, "gdesc0"), (gd1, od1, o32d1, "gdesc1")):
        _, _, mx = desc_golden(g, key)
        bar = 8 * float(g[f"spread_{key}"]) + 1e-6 * mx + 1e-12
        err = float(np.abs(got - ref).max())
        o32 = float(np.abs(r32 - ref).max())
        bar2 = 8 * max(float(g[f"spread_{key}"]), o32) + 1e-6 * mx + 1e-12
        rows.append({"tensor": key, "max64": mx, "err_gpu": err, "spread_ref32": float(g[f"spread_{key}"]),
                     "spread_oracle32": o32, "bar": bar, "ratio_ref_bar": err / bar, "bar_tests": bar2,
                     "ratio": err / bar2})
    rows.sort(key=lambda r: -r["ratio"])
    env = {k: v for k, v in os.environ.items() if k.startswith(("LG_", "SG_"))}
    print(a.name, "env", env, "loss", loss)
    # err/bar: the tests' bar (8 x the larger fp32 spread); err/refbar: 8 x the reference's alone
    print(f"{'tensor':48s} {'err/bar':>8s} {'err/refbar':>10s} {'err_gpu':>10s} {'ref32':>10s} {'oracle32':>10s} {'max64':>10s}")
    for r in rows[:14]:
        print(f"{r['tensor']:48s} {r['ratio']:8.3f} {r['ratio_ref_bar']:10.3f} {r['err_gpu']:10.3e} {r['spread_ref32']:10.3e} "
              f"{r['spread_oracle32']:10.3e} {r['max64']:10.3e} {r.get('argmax', '')}")
    # the GPU against a plain fp32 implementation: err_gpu / spread_oracle32 (scale-free)
    rel = sorted(((r["err_gpu"] / max(r["spread_oracle32"], 1e-30), r["tensor"]) for r in rows), reverse=True)
    print("worst err_gpu / spread_oracle32:", [(t, round(v, 2)) for v, t in rel[:8]])
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"name": a.name, "env": env, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
