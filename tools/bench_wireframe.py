#!/usr/bin/env python3
"""The wireframe step alone on one MI355X: the HIP path against the reference-style chain on the same GPU.

    python tools/bench_wireframe.py [--rounds R] [--window S] [--out profiles/wireframe/bench_wireframe.json]

Point features, the dense descriptor map and the segments are given and resident in HBM; what is timed
is everything ``WireframeExtractor`` does after its two extractors returned, at two shapes:

* eval: B = 1, a 480 x 640 image, 2048 keypoints, 512 lines, nothing forced;
* train: B = 32, 1000 keypoints, 250 lines, ``force_num_keypoints`` and ``force_num_lines``.

The chain it is measured against does what the reference does, with the same libraries: endpoints to
the host, ``sklearn.cluster.DBSCAN(eps, min_samples=1)``, labels back to the device, two
``scatter_reduce_`` means, the index assignments of the connectivity, ``grid_sample`` + ``normalize``,
``torch.norm`` for the keypoint merge, in a Python loop over the batch.  Both arms are warmed up, their
repetitions sized to a window of about ``--window`` seconds, and ``--rounds`` rounds time the arms one
after the other; medians with minimum and maximum are reported.  The integer outputs of the two arms
are compared, so the speed-up is over equal results.  ``kernels_per_call`` counts the device kernels
of one call of each arm (torch.profiler).
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
import lgamd  # noqa: E402,F401
from lightglue_amd.pipeline import register_model  # noqa: E402
from lightglue_amd.wireframe import WireframeExtractor  # noqa: E402

RADIUS, S, DIM = 3, 8, 256
SHAPES = {
    "eval": dict(B=1, H=480, W=640, K=2048, L=512, forced=False),
    "train": dict(B=32, H=480, W=640, K=1000, L=250, forced=True),
}
HOLD = {}


class GivenPoints(torch.nn.Module):
    def __init__(self, conf):
        super().__init__()

    def forward(self, data):
        return dict(HOLD)


def inputs(B, H, W, K, L, dev, seed=0):
    """Segments of which every second one starts within a pixel of the end of the one before, keypoints of
    which a fifth lie within two pixels of an endpoint, unit descriptors and a random NHWC map."""
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor([W - 1.0, H - 1.0])
    lines = torch.rand((B, L, 2, 2), generator=g) * size
    lines[:, 1::2, 0] = lines[:, 0:-1:2, 1] + torch.rand((B, L // 2, 2), generator=g) - 0.5
    kp = torch.rand((B, K, 2), generator=g) * size
    near = lines.reshape(B, -1, 2)[:, torch.randint(0, 2 * L, (K // 5,), generator=g)]
    kp[:, : K // 5] = near + (torch.rand((B, K // 5, 2), generator=g) - 0.5) * 2.8
    desc = torch.nn.functional.normalize(torch.randn((B, K, DIM), generator=g), dim=-1)
    dense = torch.randn((B, H // S, W // S, DIM), generator=g)
    return {"lines": lines.to(dev), "line_scores": (torch.rand((B, L), generator=g) + 0.1).to(dev), "keypoints": kp.to(dev),
            "keypoint_scores": torch.rand((B, K), generator=g).to(dev), "descriptors": desc.to(dev),
            "dense_descriptors": dense.to(dev).permute(0, 3, 1, 2)}


def sample(points, dense, s):
    b, c, h, w = dense.shape
    grid = points / (points.new_tensor([w, h]) * s) * 2 - 1
    d = torch.nn.functional.grid_sample(dense, grid.view(b, 1, -1, 2), mode="bilinear", align_corners=False)
    return torch.nn.functional.normalize(d.reshape(b, c, -1), p=2, dim=1)


def torch_chain(x, forced, H, W):
    """What the reference's extractor does after its two extractors, op for op, on the device and host."""
    from sklearn.cluster import DBSCAN

    dev = x["lines"].device
    B, L = x["lines"].shape[:2]
    dense = x["dense_descriptors"]
    scores = x["line_scores"] / (x["line_scores"].max(dim=1)[0][:, None] + 1e-8)
    kp, ks, kd = x["keypoints"].clone(), x["keypoint_scores"].clone(), x["descriptors"].clone()
    ep = x["lines"].reshape(B, -1, 2)
    remove = torch.any(torch.norm(kp[:, :, None] - ep[:, None], dim=-1) < RADIUS, dim=2)
    if forced:
        n = remove.int().sum().item()
        kp[remove] = torch.rand(n, 2, device=dev) * kp.new_tensor([[W - 1, H - 1]])
        ks[remove] = 0
        for b in range(B):
            kd[b][remove[b]] = sample(kp[b][remove[b]][None], dense[b][None], S)[0].T
    else:
        kp, ks, kd = kp[0][~remove[0]][None], ks[0][~remove[0]][None], kd[0][~remove[0]][None]
    junctions, jscores, connect, new_lines, idx, n_true = [], [], [], [], [], []
    for b in range(B):
        labels = DBSCAN(eps=RADIUS, min_samples=1).fit(ep[b].cpu().numpy()).labels_
        n = len(set(labels))
        n_true.append(n)
        labels = torch.tensor(labels, dtype=torch.long, device=dev)
        j = torch.zeros(n, 2, device=dev).scatter_reduce_(0, labels[:, None].repeat(1, 2), ep[b], reduce="mean", include_self=False)
        js = torch.zeros(n, device=dev).scatter_reduce_(0, labels, torch.repeat_interleave(scores[b], 2), reduce="mean",
                                                        include_self=False)
        new_lines.append(j[labels].reshape(-1, 2, 2))
        idx.append(labels.reshape(-1, 2))
        slots = 2 * L if forced else n
        if forced:
            j = torch.cat([j, torch.rand(slots - n, 2).to(j) * j.new_tensor([[W - 1, H - 1]])])
            js = torch.cat([js, torch.zeros(slots - n, device=dev)])
        c = torch.eye(slots, dtype=torch.bool, device=dev)
        c[idx[-1][:, 0], idx[-1][:, 1]] = True
        c[idx[-1][:, 1], idx[-1][:, 0]] = True
        junctions.append(j), jscores.append(js), connect.append(c)
    junctions = torch.stack(junctions)
    jdesc = sample(junctions, dense, S).mT
    points, pscores, pdesc, assoc = [], [], [], []
    for b in range(B):
        points.append(torch.cat([junctions[b], kp[b]]))
        pscores.append(torch.cat([jscores[b], ks[b]]))
        pdesc.append(torch.cat([jdesc[b], kd[b]]))
        a = torch.eye(len(points[-1]), dtype=torch.bool, device=dev)
        a[: n_true[b], : n_true[b]] = connect[b][: n_true[b], : n_true[b]]
        assoc.append(a)
    return {"keypoints": torch.stack(points), "keypoint_scores": torch.stack(pscores), "descriptors": torch.stack(pdesc),
            "pl_associativity": torch.stack(assoc), "lines": torch.stack(new_lines), "lines_junc_idx": torch.stack(idx),
            "num_junctions": torch.tensor(n_true)}


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def timed_arms(arms, rounds, seconds):
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


def kernels_per_call(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name
                   and "emset" not in e.name)
    except Exception as e:  # a profiler that does not load is no reason to lose the timings
        return f"unavailable ({type(e).__name__})"


def run(name, shape, rounds, seconds, dev):
    B, H, W, K, L, forced = (shape[k] for k in ("B", "H", "W", "K", "L", "forced"))
    x = inputs(B, H, W, K, L, dev)
    HOLD.clear()
    HOLD.update({k: x[k] for k in ("keypoints", "keypoint_scores", "descriptors", "dense_descriptors")})
    register_model("bench_given_points", GivenPoints)
    model = WireframeExtractor({"point_extractor": {"name": "bench_given_points", "force_num_keypoints": forced},
                                "line_extractor": {"name": None, "force_num_lines": forced, "max_num_lines": L if forced else None},
                                "wireframe_params": {"nms_radius": RADIUS}}).eval()
    data = {"image": torch.zeros((B, 1, H, W), device=dev), "lines": x["lines"], "line_scores": x["line_scores"]}
    arms = {"hip": lambda: model(data), "torch_chain": lambda: torch_chain(x, forced, H, W)}
    with torch.no_grad():
        r = timed_arms(arms, rounds, seconds)
        launches = {n: kernels_per_call(fn) for n, fn in arms.items()}
    pred, ref = r["hip"][4], r["torch_chain"][4]
    equal = {k: bool(torch.equal(pred[k].cpu(), ref[k].cpu())) for k in ("lines_junc_idx", "num_junctions", "pl_associativity")}
    nj = pred["num_junctions"].cpu()
    coord = float((pred["lines"] - ref["lines"]).abs().max())
    ms = {n: {"median": round(1e3 * v[0], 4), "min": round(1e3 * v[1], 4), "max": round(1e3 * v[2], 4), "reps_per_window": v[3]}
          for n, v in r.items()}
    t_hip, t_ref = r["hip"][0], r["torch_chain"][0]
    return {"config": f"wireframe step ({name}), B={B}, {H}x{W}, {K} keypoints, {L} lines, D={DIM}, forced={forced}, 1 GPU",
            "hip_ms": round(1e3 * t_hip, 4), "torch_chain_ms": round(1e3 * t_ref, 4), "speedup": round(t_ref / t_hip, 2),
            "arms_ms": ms, "rounds": rounds, "window_s": seconds, "kernels_per_call": launches,
            "junctions_mean": float(nj.float().mean()), "endpoints": 2 * L, "integer_outputs_equal": equal,
            "lines_max_abs_diff": coord}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="eval,train")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window of an arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wireframe", "bench_wireframe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wireframe.py needs a HIP device: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    rows = []
    for name in a.shapes.split(","):
        rows.append(run(name, SHAPES[name], a.rounds, a.window, dev))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
