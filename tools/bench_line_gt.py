#!/usr/bin/env python3
"""Time the HIP line ground truth (lightglue_amd.line_gt) against a reference-style chain in the same
process: the formula of gt_line_matches_from_homography (gt_generation.py:409-558) written with dense
fp32 torch ops on the same GPU (two [B, n0, n1, npts] passes), the [B, n0, n1] cost copied to the host,
SciPy's linear_sum_assignment per pair (where SciPy imports; otherwise only the dense part is timed)
and the labels scattered back on the device -- what a caller had before.

Shapes: B = 32 and B = 1 with 250 x 250 lines and npts = 50 (the training shape of the
superpoint+lsd+gluestick-homography configuration).  Per shape: the whole call, stage A (counts) and
stage B (labels with the solver) of the HIP path, the solver alone on the costs of that shape, and the
chain with its dense part and its host part separately.  Times are HIP-event times per call over
``--iters`` back-to-back calls after ``--warmup`` calls (the events bracket the host work of the chain
too), the implementations alternating in ``--rounds`` rounds (median and min..max reported); peak
memory is ``torch.cuda.max_memory_allocated`` above what was allocated before the call.  The labels of
both are compared before timing and the disagreements counted (near-ties of the fp32 arithmetic).

    python tools/bench_line_gt.py [--json profiles/line_gt/bench_line_gt.json]

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
from lightglue_amd import line_gt  # noqa: E402

try:
    from scipy.optimize import linear_sum_assignment as scipy_lsa
except ImportError:
    scipy_lsa = None

W, H_IMG = 640, 480


def chain_dense(l0, l1, v0, v1, H, npts, dist_th, overlap_th, vis_th):
    """The dense half of the chain: everything up to the cost matrix, in fp32 on the device."""
    dev = l0.device

    def clamp(l):
        return torch.minimum(l.clamp_min(0.0), l.new_tensor([W - 1, H_IMG - 1, W - 1, H_IMG - 1]))

    def samples(l):
        step = (l[..., 2:] - l[..., :2]) / (npts - 1)
        return l[..., None, :2] + step[..., None, :] * torch.arange(npts, device=dev, dtype=l.dtype)[:, None]

    def warp(p, Hm):
        B, n = p.shape[:2]
        ph = torch.cat([p, p.new_ones(p.shape[:-1] + (1,))], -1).reshape(B, n * npts, 3) @ Hm.transpose(1, 2)
        return (ph[..., :2] / (ph[..., 2:] + 1e-5)).reshape(B, n, npts, 2)

    def counts(seg, pts):  # [B, nseg, nlines]
        d = seg[..., 2:] - seg[..., :2]
        size = d.norm(dim=-1).half().float()
        nd = d / size[..., None]
        c = pts[:, None] - seg[:, :, None, None, 2:]
        nx, ny = nd[..., 0, None, None], nd[..., 1, None, None]
        along = nx * c[..., 0] + ny * c[..., 1]
        across = nx * c[..., 1] - ny * c[..., 0]
        return ((across.abs() < dist_th) & (along <= 0) & (along.abs() <= size[..., None, None])).sum(-1)

    def leaves(p):
        out = (p < 0).any(-1) | (p >= p.new_tensor([W, H_IMG])).any(-1)
        return out.float().mean(-1) >= (1 - vis_th)

    c0, c1 = clamp(l0), clamp(l1)
    p01, p10 = warp(samples(c0), H), warp(samples(c1), torch.linalg.inv(H))
    out0, out1 = leaves(p10), leaves(p01)
    n_a, n_b = counts(c0, p10), counts(c1, p01).transpose(1, 2)
    mask = (n_a > npts * overlap_th) & (n_b > npts * overlap_th) & ~out0[:, None] & ~out1[:, :, None]
    dead0 = ~mask.any(2) | out1 | ~v0
    dead1 = ~mask.any(1) | out0 | ~v1
    cost = -(n_a * n_b)
    cost = torch.where(dead0[:, :, None] | dead1[:, None], torch.full_like(cost, 1000000), cost)
    return n_a, n_b, mask, dead0, dead1, cost


def chain_labels(mask, dead0, dead1, cost, v0, v1):
    """The host half: the cost to the host, SciPy per pair, the labels scattered on the device."""
    dev = cost.device
    B, n0, n1 = cost.shape
    pairs = np.stack([np.stack(scipy_lsa(c)) for c in cost.cpu().numpy()])
    pairs = torch.from_numpy(pairs).to(dev)
    rows, cols = pairs[:, 0], pairs[:, 1]
    b = torch.arange(B, device=dev)[:, None].expand_as(rows)
    keep = mask[b, rows, cols] & ~dead0[b, rows] & ~dead1[b, cols]
    positive = torch.zeros((B, n0, n1), dtype=torch.bool, device=dev)
    positive[b[keep], rows[keep], cols[keep]] = True
    minus1 = positive.new_full((), -1, dtype=torch.long)
    m0 = torch.where(positive.any(2), positive.int().argmax(2), minus1)
    m1 = torch.where(positive.any(1), positive.int().argmax(1), minus1)
    m0[~v0] = -2
    m1[~v1] = -2
    return positive, m0, m1


def make_inputs(B, n0, n1, seed, dev):
    """The recipe of the random fixtures (tests/golden/make_line_gt_golden.py)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    size = np.array([W, H_IMG], float)
    H = np.tile(np.eye(3), (B, 1, 1))
    H[:, :2, :2] += rng.standard_normal((B, 2, 2)) * 0.05
    H[:, :2, 2] = rng.uniform(-30.0, 30.0, (B, 2))
    H[:, 2, :2] = rng.standard_normal((B, 2)) * 1e-4

    def segments(n):
        a = rng.random((B, n, 2)) * (size + 40.0) - 20.0
        ang = rng.uniform(0, 2 * np.pi, (B, n))
        ln = rng.uniform(20.0, 200.0, (B, n))
        return np.concatenate([a, a + ln[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)], -1)

    l0, l1 = segments(n0), segments(n1)
    nw = min(2 * n1 // 3, n0)
    for b in range(B):
        p = np.concatenate([l0[b, :nw].reshape(nw * 2, 2), np.ones((nw * 2, 1))], 1) @ H[b].T
        l1[b, :nw] = (p[:, :2] / p[:, 2:]).reshape(nw, 4) + rng.standard_normal((nw, 4)) * 1.5
        l1[b] = l1[b, rng.permutation(n1)]
    v0, v1 = rng.random((B, n0)) > 1 / 12, rng.random((B, n1)) > 1 / 12
    f = [torch.from_numpy(x.astype(np.float32)).to(dev) for x in (l0, l1)]
    return f + [torch.from_numpy(v0).to(dev), torch.from_numpy(v1).to(dev), torch.from_numpy(H.astype(np.float32)).to(dev)]


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_line_gt.py needs a HIP device")
    dev = torch.device("cuda", 0)
    npts, dist_th, overlap_th, vis_th = 50, 5, 0.2, 0.5
    shape = (H_IMG, W)
    rows = []
    for B, n0, n1 in ((32, 250, 250), (1, 250, 250)):
        l0, l1, v0, v1, H = make_inputs(B, n0, n1, 7, dev)
        cnt = line_gt.close_point_counts_from_homography(l0, l1, shape, shape, H, npts, dist_th, vis_th)
        dense = chain_dense(l0, l1, v0, v1, H, npts, dist_th, overlap_th, vis_th)
        cost64 = dense[5].double()
        fns = {
            "hip_total": lambda: line_gt.gt_line_matches_from_homography(l0, l1, v0, v1, shape, shape, H, npts, dist_th,
                                                                         overlap_th, vis_th),
            "hip_counts": lambda: line_gt.close_point_counts_from_homography(l0, l1, shape, shape, H, npts, dist_th, vis_th),
            "hip_labels": lambda: line_gt.line_labels_from_counts(*cnt, v0, v1, npts, overlap_th),
            "hip_solver": lambda: line_gt.linear_sum_assignment(cost64),
            "chain_dense": lambda: chain_dense(l0, l1, v0, v1, H, npts, dist_th, overlap_th, vis_th),
        }
        row = {"B": B, "n0": n0, "n1": n1, "npts": npts, "scipy": scipy_lsa is not None}
        if scipy_lsa is not None:
            fns["chain_host"] = lambda: chain_labels(*dense[2:], v0, v1)
            fns["chain_total"] = lambda: chain_labels(*chain_dense(l0, l1, v0, v1, H, npts, dist_th, overlap_th, vis_th)[2:], v0, v1)
            # the same labels first (near-ties aside: count the disagreements, do not hide them)
            oh, oc = fns["hip_total"](), fns["chain_total"]()
            row["entries_differing"] = {k: int((x != y).sum()) for k, x, y in zip(("positive", "m0", "m1"), oh, oc)}
            row["positives"] = int(oh[0].sum())
            solver = fns["hip_solver"]()
            host = np.stack([np.stack(scipy_lsa(c)) for c in cost64.cpu().numpy()])
            row["solver_pairs_differing_from_scipy"] = int((torch.stack(solver, 1).cpu().numpy() != host).any((1, 2)).sum())
            del oh, oc
        row["counts_differing_from_chain"] = [int((cnt[0] != dense[0]).sum()), int((cnt[1] != dense[1]).sum())]
        peak = {k: peak_above_baseline(fns[k]) for k in ("hip_total", "chain_dense")}
        for f in fns.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):  # alternate the implementations in every round
            for k, f in fns.items():
                ms[k].append(time_calls(f, a.iters))
        for k in fns:
            row[f"{k}_ms_median"] = statistics.median(ms[k])
            row[f"{k}_ms_min"], row[f"{k}_ms_max"] = min(ms[k]), max(ms[k])
        row["hip_peak_bytes"], row["chain_dense_peak_bytes"] = peak["hip_total"], peak["chain_dense"]
        ref = "chain_total" if scipy_lsa is not None else "chain_dense"
        row["speedup_vs_" + ref] = row[ref + "_ms_median"] / row["hip_total_ms_median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
