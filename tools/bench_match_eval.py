#!/usr/bin/env python3
"""Time the batched match evaluation (lightglue_amd.match_eval: one launch for every pair and all
three metrics) against the per-pair torch chain it replaces, on the same GPU and in the same process:
``hpatches_metrics.eval_homography_dlt`` plus the reference's two precision metrics
(eval/utils.py:40-91: boolean-mask gathers, sym_homography_error, generalized_epi_dist, ``.item()``)
restated below with torch ops, called once per pair as the reference's eval loop does.

Shape: 32 x 2048 x 2048 with about 600 matches per pair (planar scenes, noise of 0.3 / 2 / 20 px, as
tests/golden/make_match_eval_golden.py).  Times are HIP-event times per batch over ``--iters``
back-to-back batches after ``--warmup`` batches, the two implementations alternating in ``--rounds``
rounds (median and min..max over rounds).  (a) is timed without reading its results back (the caller
decides when); ``hip_with_readback`` adds one ``.cpu()`` of every result per batch.

    python tools/bench_match_eval.py [--json profiles/match_eval/bench_match_eval.json]

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
from lightglue_amd import hpatches_metrics as hm  # noqa: E402
from lightglue_amd import match_eval as me  # noqa: E402


# ---------------------------------------------------------------------------------------------
# the baseline: the reference's per-pair formulas, as written, on the device
def hom(p):
    return torch.cat([p, torch.ones_like(p[..., :1])], -1)


def unhom(p):
    return p[..., :-1] / p[..., -1:]


def torch_matches_homography(data, pred):
    H = data["H_0to1"]
    p0, p1, _ = hm.get_matches_scores(pred["keypoints0"], pred["keypoints1"], pred["matches0"], pred["matching_scores0"])
    d01 = ((unhom(hom(p0) @ H.transpose(-1, -2)) - p1) ** 2).sum(-1).sqrt()
    d10 = ((unhom(hom(p1) @ torch.pinverse(H.transpose(-1, -2))) - p0) ** 2).sum(-1).sqrt()
    err = (d01 + d10) / 2.0
    return {"prec@1px": (err < 1).float().mean().nan_to_num().item(), "prec@3px": (err < 3).float().mean().nan_to_num().item(),
            "num_matches": p0.shape[0]}


def torch_matches_epipolar(data, pred):
    cam0, cam1, T = data["view0"]["camera"], data["view1"]["camera"], data["T_0to1"]
    p0, p1, _ = hm.get_matches_scores(pred["keypoints0"], pred["keypoints1"], pred["matches0"], pred["matching_scores0"])
    R, t = T[:9].reshape(3, 3), T[9:]
    z = torch.zeros_like(t[0])
    E = torch.stack([z, -t[2], t[1], t[2], z, -t[0], -t[1], t[0], z]).reshape(3, 3) @ R
    a, b = hom((p0 - cam0[4:6]) / cam0[2:4]), hom((p1 - cam1[4:6]) / cam1[2:4])
    bEa = torch.einsum("ni,ij,nj->n", b, E, a)
    Ea, Etb = torch.einsum("ij,nj->ni", E, a), torch.einsum("ij,ni->nj", E, b)
    d0 = (Ea[..., 0] ** 2 + Ea[..., 1] ** 2).clamp(min=1e-6)
    d1 = (Etb[..., 0] ** 2 + Etb[..., 1] ** 2).clamp(min=1e-6)
    err = bEa.abs() * (1 / d0.sqrt() + 1 / d1.sqrt()) / 2
    return {k: (err < th).float().mean().item() for k, th in (("epi_prec@1e-4", 1e-4), ("epi_prec@5e-4", 5e-4),
                                                              ("epi_prec@1e-3", 1e-3))}


def torch_chain(data, pred):
    """The reference's eval loop: one pair at a time, every metric through .item()."""
    rows = []
    B = pred["matches0"].shape[0]
    for b in range(B):
        d = {"H_0to1": data["H_0to1"][b], "T_0to1": data["T_0to1"][b],
             "view0": {"image_size": data["view0"]["image_size"][b], "camera": data["view0"]["camera"][b]},
             "view1": {"camera": data["view1"]["camera"][b]}}
        p = {k: v[b] for k, v in pred.items()}
        rows.append({**torch_matches_homography(d, p), **torch_matches_epipolar(d, p), **hm.eval_homography_dlt(d, p)})
    return rows


# ---------------------------------------------------------------------------------------------
def make_inputs(B, M, N, live, seed, dev):
    g = torch.Generator().manual_seed(seed)
    W, Hh = 640.0, 480.0
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    cams, Ks = [], []
    for _ in range(2):
        fx = 400 + 200 * u(B)
        fy = fx * (0.9 + 0.2 * u(B))
        cx, cy = W / 2 + 40 * u(B) - 20, Hh / 2 + 40 * u(B) - 20
        cams.append(torch.stack([torch.full((B,), W, dtype=torch.float64), torch.full((B,), Hh, dtype=torch.float64),
                                 fx, fy, cx, cy], 1))
        K = torch.zeros(B, 3, 3, dtype=torch.float64)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = fx, fy, cx, cy, 1.0
        Ks.append(K)
    aa = 0.08 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    th = aa.norm(dim=1)[:, None, None]
    k = aa / aa.norm(dim=1, keepdim=True)
    Kx = torch.zeros(B, 3, 3, dtype=torch.float64)
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    R = torch.eye(3, dtype=torch.float64) + th.sin() * Kx + (1 - th.cos()) * Kx @ Kx
    t = 0.4 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    n = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    H = Ks[1] @ (R + t[:, :, None] * n[None, None, :] / 5.0) @ torch.linalg.inv(Ks[0])
    H = H / H[:, 2:, 2:]
    size = torch.tensor([W, Hh], dtype=torch.float64)
    k0, k1 = u(B, M, 2) * size, u(B, N, 2) * size
    m0 = torch.full((B, M), -1, dtype=torch.int64)
    for b in range(B):
        sel, dst = torch.randperm(M, generator=g)[:live], torch.randperm(N, generator=g)[:live]
        sigma = torch.tensor([0.3, 2.0, 20.0], dtype=torch.float64)[torch.randint(0, 3, (live,), generator=g)]
        k1[b, dst] = unhom(hom(k0[b, sel]) @ H[b].T) + torch.randn(live, 2, generator=g, dtype=torch.float64) * sigma[:, None]
        m0[b, sel] = dst
    f = lambda x: x.float().to(dev).contiguous()  # noqa: E731
    pred = {"keypoints0": f(k0), "keypoints1": f(k1), "matches0": m0.to(dev), "matching_scores0": f(0.1 + 0.9 * u(B, M))}
    data = {"H_0to1": f(H), "T_0to1": f(torch.cat([R.reshape(B, 9), t], 1)),
            "view0": {"image_size": f(size.repeat(B, 1)), "camera": f(cams[0])}, "view1": {"camera": f(cams[1])}}
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
                                                   "match_eval", "bench_match_eval.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_eval.py needs a HIP device")
    dev = torch.device("cuda", 0)
    B, M, N, live = 32, 2048, 2048, 600
    data, pred = make_inputs(B, M, N, live, 7, dev)
    fns = {"hip": lambda: me.eval_matches(data, pred),
           "hip_with_readback": lambda: {k: v.cpu() for k, v in me.eval_matches(data, pred).items()},
           "torch_per_pair": lambda: torch_chain(data, pred)}
    # before anything is timed: both against the same chain on fp64 copies of the fp32 inputs (the fp32
    # chain's ratios may differ from it by matches near a threshold, its DLT error by fp32 rounding)
    dbl = lambda t: t.double() if t.is_floating_point() else t  # noqa: E731
    data64 = {k: ({q: dbl(w) for q, w in v.items()} if isinstance(v, dict) else dbl(v)) for k, v in data.items()}
    out, rows = fns["hip_with_readback"](), fns["torch_per_pair"]()
    rows64 = torch_chain(data64, {k: dbl(v) for k, v in pred.items()})
    keys = ("prec@1px", "prec@3px", "epi_prec@1e-4", "epi_prec@5e-4", "epi_prec@1e-3")
    worst = {"hip_vs_fp64": {k: max(abs(float(out[k][b]) - rows64[b][k]) for b in range(B)) for k in keys},
             "torch_fp32_vs_fp64": {k: max(abs(rows[b][k] - rows64[b][k]) for b in range(B)) for k in keys}}
    worst["hip_vs_fp64"]["H_error_dlt_rel"] = max(
        abs(float(out["H_error_dlt"][b]) - rows64[b]["H_error_dlt"]) / rows64[b]["H_error_dlt"] for b in range(B))
    worst["torch_fp32_vs_fp64"]["H_error_dlt_rel"] = max(
        abs(rows[b]["H_error_dlt"] - rows64[b]["H_error_dlt"]) / rows64[b]["H_error_dlt"] for b in range(B))
    assert all(int(out["num_matches"][b]) == rows[b]["num_matches"] == live for b in range(B))
    for f in fns.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the implementations in every round
        for k, f in fns.items():
            ms[k].append(time_calls(f, a.iters))
    row = {"B": B, "M": M, "N": N, "matches_per_pair": live, "metrics": ["homography", "epipolar", "dlt"],
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "max_difference": worst}
    for k in fns:
        row[f"{k}_ms_median"] = statistics.median(ms[k])
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = min(ms[k]), max(ms[k])
        row[f"{k}_pairs_per_s"] = 1e3 * B / row[f"{k}_ms_median"]
    row["speedup"] = row["torch_per_pair_ms_median"] / row["hip_ms_median"]
    row["speedup_with_readback"] = row["torch_per_pair_ms_median"] / row["hip_with_readback_ms_median"]
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
