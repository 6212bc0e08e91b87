#!/usr/bin/env python3
"""Time the HIP nearest-neighbour matcher (lightglue_amd.nn_matcher) against the torch chain it
replaces: the reference's formula (nearest_neighbor_matcher.py:16-72: einsum, two topk over the
similarity and its transposed view, the thresholds, the mutual check, two log_softmax) restated
below with torch ops and run on the same GPU -- what a caller had for the baseline matcher on the
device before.

Shapes: 32 x 2048 x 2048 x 256 and 1 x 1024 x 1024 x 128; with and without the two dense outputs
(``similarity`` / ``log_assignment``; the torch chain then skips the log_softmax passes but still
forms the similarity it searches); thresholds off, and ``ratio_thresh`` 0.8 + ``distance_thresh``
0.7.  Times are HIP-event times per call over ``--iters`` back-to-back calls after ``--warmup``
calls, the two implementations alternating in ``--rounds`` rounds (median and min..max over rounds
reported); peak memory is ``torch.cuda.max_memory_allocated`` above what was allocated before the
call.  The outputs of both are compared before timing (near-ties aside: the disagreements are
counted, not hidden).

    python tools/bench_nn.py [--json out.json]

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
from lightglue_amd.nn_matcher import nn_match as hip_nn  # noqa: E402


# ---------------------------------------------------------------------------------------------
# the baseline: the reference's formula, as written, on the device
def find_nn(sim, ratio_thresh, distance_thresh):
    val, ind = sim.topk(2 if ratio_thresh else 1, dim=-1, largest=True)
    dist = 2 * (1 - val)
    mask = torch.ones(ind.shape[:-1], dtype=torch.bool, device=sim.device)
    if ratio_thresh:
        mask = mask & (dist[..., 0] <= (ratio_thresh**2) * dist[..., 1])
    if distance_thresh:
        mask = mask & (dist[..., 0] <= distance_thresh**2)
    return torch.where(mask, ind[..., 0], ind.new_tensor(-1))


def mutual_check(m0, m1):
    i0 = torch.arange(m0.shape[-1], device=m0.device)
    i1 = torch.arange(m1.shape[-1], device=m1.device)
    loop0 = torch.gather(m1, -1, torch.where(m0 > -1, m0, m0.new_tensor(0)))
    loop1 = torch.gather(m0, -1, torch.where(m1 > -1, m1, m1.new_tensor(0)))
    return (torch.where((m0 > -1) & (i0 == loop0), m0, m0.new_tensor(-1)),
            torch.where((m1 > -1) & (i1 == loop1), m1, m1.new_tensor(-1)))


@torch.no_grad()
def torch_nn(d0, d1, ratio_thresh, distance_thresh, dense=True):
    sim = torch.einsum("bnd,bmd->bnm", d0, d1)
    m0 = find_nn(sim, ratio_thresh, distance_thresh)
    m1 = find_nn(sim.transpose(1, 2), ratio_thresh, distance_thresh)
    m0, m1 = mutual_check(m0, m1)
    out = {"matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(), "matching_scores1": (m1 > -1).float()}
    if dense:
        b, m, n = sim.shape
        la = sim.new_zeros(b, m + 1, n + 1)
        la[:, :-1, :-1] = torch.nn.functional.log_softmax(sim, -1) + torch.nn.functional.log_softmax(sim, -2)
        out["similarity"], out["log_assignment"] = sim, la
    return out


# ---------------------------------------------------------------------------------------------
def make_inputs(B, M, N, D, seed, dev):
    """Unit-normalised Gaussian descriptors; two thirds of image 1 are image-0 points plus noise of
    relative norm uniform in [0, 1.6] (tests/golden/make_nn_golden.py's recipe)."""
    g = torch.Generator().manual_seed(seed)
    d0 = torch.randn(B, M, D, generator=g)
    d1 = torch.randn(B, N, D, generator=g)
    nm = 2 * min(M, N) // 3
    for b in range(B):
        src = torch.randperm(M, generator=g)[:nm]
        dst = torch.randperm(N, generator=g)[:nm]
        lvl = torch.rand(nm, 1, generator=g) * 1.6
        d1[b, dst] = d0[b, src] + torch.randn(nm, D, generator=g) * lvl * d0[b, src].norm(dim=-1, keepdim=True) / D**0.5
    norm = lambda x: (x / x.norm(dim=-1, keepdim=True)).to(dev).contiguous()  # noqa: E731
    return norm(d0), norm(d1)


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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nn.py needs a HIP device")
    dev = torch.device("cuda", 0)
    rows = []
    for B, M, N, D in ((32, 2048, 2048, 256), (1, 1024, 1024, 128)):
        d0, d1 = make_inputs(B, M, N, D, 7, dev)
        for ratio, dist in ((None, None), (0.8, 0.7)):
            for dense in (True, False):
                fns = {"hip": lambda: hip_nn(d0, d1, ratio, dist, True, similarity=dense, log_assignment=dense),
                       "torch": lambda: torch_nn(d0, d1, ratio, dist, dense)}
                oh, ot = fns["hip"](), fns["torch"]()
                diff = {k: int((oh[k] != ot[k]).sum()) for k in ("matches0", "matches1")}
                if dense:
                    diff["similarity_max_abs"] = float((oh["similarity"] - ot["similarity"]).abs().max())
                    diff["log_assignment_max_abs"] = float((oh["log_assignment"] - ot["log_assignment"]).abs().max())
                matched = int((oh["matches0"] > -1).sum())
                del oh, ot
                peak = {k: peak_above_baseline(f) for k, f in fns.items()}
                for f in fns.values():
                    for _ in range(a.warmup):
                        f()
                torch.cuda.synchronize()
                ms = {k: [] for k in fns}
                for _ in range(a.rounds):  # alternate the two in every round
                    for k, f in fns.items():
                        ms[k].append(time_calls(f, a.iters))
                written = (4 * B * (M * N + (M + 1) * (N + 1)) if dense else 0) + B * (M + N) * 12
                row = {"B": B, "M": M, "N": N, "D": D, "ratio_thresh": ratio, "distance_thresh": dist, "dense_outputs": dense,
                       "matched_image0": matched, "differing": diff, "bytes_written_hip": written}
                for k in fns:
                    row[f"{k}_ms_median"] = statistics.median(ms[k])
                    row[f"{k}_ms_min"], row[f"{k}_ms_max"] = min(ms[k]), max(ms[k])
                    row[f"{k}_peak_bytes"] = peak[k]
                row["speedup"] = row["torch_ms_median"] / row["hip_ms_median"]
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
