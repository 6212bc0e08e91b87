#!/usr/bin/env python3
"""Generate the homography ground-truth fixtures by running the REAL reference.

Run from the repo root where the reference checkout exists (it does not on the GPU box)::

    python tests/golden/make_gt_golden.py

Imports the reference's ``gluefactory/geometry/gt_generation.py`` through synthetic ``gluefactory`` /
``gluefactory.geometry`` package objects whose ``__path__`` points into the reference (their
``__init__`` files are skipped) and stand-ins for ``omegaconf``, ``kornia`` and ``cv2`` (and
``scipy.optimize`` where SciPy is missing), none of which ``gt_matches_from_homography`` touches.
It runs ``gt_matches_from_homography`` in fp32 and in fp64 on inputs from NumPy PCG64 recipes and
writes ``tests/golden/gt/gt_*.npz``: the inputs, the reference's fp32 outputs (``assignment`` as index
triples, ``reward`` as int8) and the fp64 margins.

Near-tie gating (random cases; the exact case has none).  ``e`` is the largest
|dist_fp32 - dist_fp64| the reference itself shows over entries with
dist_fp64 < 4 max(pos_th, neg_th)^2 and tau = 4 e (a different inverse and a different sum order on
top of the reference's own fp32 error).  tests/gt_ref.py:margins defines the undecidable rows,
columns and reward entries from tau; the fixture stores those masks.  Asserted here (change a failing
seed, not the cap): undecidable rows + columns <= 3 %, undecidable reward entries <= 0.1 %, and the
reference's own fp32 and fp64 runs agree on every decidable item.  The projection tolerance is
4 max|proj_fp32 - proj_fp64| of the reference.
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gt_ref  # noqa: E402


def install_shim():
    for name in ("omegaconf", "kornia", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    try:
        import scipy.optimize  # noqa: F401
    except ImportError:
        sp, so = types.ModuleType("scipy"), types.ModuleType("scipy.optimize")
        so.linear_sum_assignment = None
        sp.optimize = so
        sys.modules["scipy"], sys.modules["scipy.optimize"] = sp, so
    for name, path in [("gluefactory", "gluefactory"), ("gluefactory.geometry", "gluefactory/geometry")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    return importlib.import_module("gluefactory.geometry.gt_generation")


def random_case(seed, B, M, N):
    """Random perspective H (identity + N(0, 0.05) on the 2x2 block, a shift within +-30 px,
    N(0, 1e-4) on the last row); 640x480 points; half of image 1 is image 0 warped plus 1.5 px of
    noise, the rest uniform; image 1 shuffled."""
    rng = np.random.Generator(np.random.PCG64(seed))
    size = np.array([640.0, 480.0])
    H = np.tile(np.eye(3), (B, 1, 1))
    H[:, :2, :2] += rng.standard_normal((B, 2, 2)) * 0.05
    H[:, :2, 2] = rng.uniform(-30.0, 30.0, (B, 2))
    H[:, 2, :2] = rng.standard_normal((B, 2)) * 1e-4
    kp0 = rng.random((B, M, 2)) * size
    kp1 = rng.random((B, N, 2)) * size
    nw = min(N // 2, M)
    for b in range(B):
        src = rng.permutation(M)[:nw]
        ph = np.concatenate([kp0[b, src], np.ones((nw, 1))], 1) @ H[b].T
        kp1[b, :nw] = ph[:, :2] / ph[:, 2:] + rng.standard_normal((nw, 2)) * 1.5
        kp1[b] = kp1[b, rng.permutation(N)]
    return kp0.astype(np.float32), kp1.astype(np.float32), H.astype(np.float32)


def exact_case(seed, B, M, N):
    """Identity H, integer keypoints in [0, 40), image 1 = image 0 plus integer offsets, points
    duplicated in both images (tied minima in rows and columns)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kp0 = rng.integers(0, 40, (B, M, 2)).astype(np.float64)
    kp0[:, M - M // 4:] = kp0[:, : M // 4]  # duplicates in image 0
    kp1 = np.empty((B, N, 2))
    for b in range(B):
        src = rng.permutation(M)[:N]
        kp1[b] = np.clip(kp0[b, src] + rng.integers(-3, 4, (N, 2)), 0, 39)
    kp1[:, N - N // 4:] = kp1[:, : N // 4]  # duplicates in image 1
    H = np.tile(np.eye(3), (B, 1, 1))
    return kp0.astype(np.float32), kp1.astype(np.float32), H.astype(np.float32)


CASES = [
    # name, recipe, seed, B, M, N, th_positive, th_negative
    ("gt_exact_b3_m64_n48", exact_case, 11, 3, 64, 48, 3.0, 3.0),
    ("gt_rand_b2_m300_n257", random_case, 12, 2, 300, 257, 3.0, 3.0),
    # seed 16, not 13: with seed 13's H the reference's fp32 projections happened to be within 2.3e-4 px
    # of fp64 on the generating host and 9.4e-4 px on another (torch's fp32 inverse and matmul round
    # differently from CPU to CPU), so the tolerance recorded from the first rejected the reference's
    # own formula on the second; this H shows an error of the usual size on both
    ("gt_rand_b1_m37_n4100", random_case, 16, 1, 37, 4100, 3.0, 3.0),
    ("gt_rand_b1_m4100_n37", random_case, 14, 1, 4100, 37, 3.0, 3.0),
    ("gt_th_p3n2_b2_m128_n128", random_case, 15, 2, 128, 128, 3.0, 2.0),
    ("gt_th_p3n6_b2_m128_n128", random_case, 15, 2, 128, 128, 3.0, 6.0),
]


def dist_of(kp0, kp1, p01, p10):  # gt_generation.py:124-126 on the reference's own projections
    d0 = torch.sum((p01.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2, -1)
    d1 = torch.sum((kp0.unsqueeze(-2) - p10.unsqueeze(-3)) ** 2, -1)
    return torch.max(d0, d1)


def main():
    gen = install_shim()
    for name, recipe, seed, B, M, N, pos, neg in CASES:
        kp0, kp1, H = recipe(seed, B, M, N)
        exact = recipe is exact_case
        t0, t1, tH = torch.from_numpy(kp0), torch.from_numpy(kp1), torch.from_numpy(H)
        if exact:
            assert torch.equal(torch.inverse(tH), tH), "the reference's inverse of the identity is not the identity"
        r32 = gen.gt_matches_from_homography(t0, t1, tH, pos_th=pos, neg_th=neg)
        r64 = gen.gt_matches_from_homography(t0.double(), t1.double(), tH.double(), pos_th=pos, neg_th=neg)
        assert r32["reward"].dtype == torch.float32 and r32["matches0"].dtype == torch.int64
        out = {"keypoints0": kp0, "keypoints1": kp1, "H_0to1": H}
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0"):
            out[k] = r32[k].numpy()
        out["assignment_idx"] = np.argwhere(r32["assignment"].numpy()).astype(np.int32)
        rw = r32["reward"].numpy()
        assert np.isin(rw, (-1.0, 0.0, 1.0)).all()
        out["reward_i8"] = rw.astype(np.int8)
        meta = {"B": B, "M": M, "N": N, "th_positive": pos, "th_negative": neg, "seed": seed, "exact": exact}
        if exact:
            # every row / column decided, no tolerance: the masks exist so one loader serves all
            out["und_rows"], out["und_cols"] = np.zeros((B, M), bool), np.zeros((B, N), bool)
            out["und_reward_idx"] = np.zeros((0, 3), np.int32)
            ties = int((r32["reward"] == 0).sum())
            print(f"{name}: positives {len(out['assignment_idx'])}, entries at a threshold {ties}")
        else:
            d32 = dist_of(t0, t1, r32["proj_0to1"], r32["proj_1to0"]).double()
            d64 = dist_of(t0.double(), t1.double(), r64["proj_0to1"], r64["proj_1to0"])
            near = d64 < 4.0 * max(pos, neg) ** 2
            e = float((d32 - d64)[near].abs().max())
            tau = 4.0 * e
            mg = gt_ref.margins(kp0, kp1, H, pos, neg, tau)
            ur, uc, ue = mg["und_rows"], mg["und_cols"], mg["und_reward"]
            frac_rc = (ur.sum() + uc.sum()) / (ur.size + uc.size)
            frac_e = ue.sum() / ue.size
            assert frac_rc <= 0.03, (name, frac_rc)
            assert frac_e <= 0.001, (name, frac_e)
            # the reference's own two precisions agree on everything decidable
            for k, ok in (("matches0", ~ur), ("matches1", ~uc)):
                assert np.array_equal(r32[k].numpy()[ok], r64[k].numpy()[ok]), (name, k)
            ok_a = ~ur[:, :, None] & ~uc[:, None, :]
            assert np.array_equal(r32["assignment"].numpy()[ok_a], r64["assignment"].numpy()[ok_a]), name
            assert np.array_equal(rw[~ue], r64["reward"].numpy()[~ue]), name
            perr = max(float((r32[k].double() - r64[k]).abs().max()) for k in ("proj_0to1", "proj_1to0"))
            out["und_rows"], out["und_cols"] = ur, uc
            out["und_reward_idx"] = np.argwhere(ue).astype(np.int32)
            out["proj_0to1_f64"], out["proj_1to0_f64"] = r64["proj_0to1"].numpy(), r64["proj_1to0"].numpy()
            meta.update({"e": e, "tau": tau, "proj_err": perr, "proj_tol": 4.0 * perr})
            print(f"{name}: e {e:.3e} tau {tau:.3e} proj_err {perr:.3e} undecidable rows+cols "
                  f"{int(ur.sum() + uc.sum())}/{ur.size + uc.size} reward {int(ue.sum())}/{ue.size} "
                  f"positives {len(out['assignment_idx'])} m0>-1 {(out['matches0'] > -1).sum()} "
                  f"m0==-1 {(out['matches0'] == -1).sum()} m0==-2 {(out['matches0'] == -2).sum()}")
        out["meta_json"] = np.array(json.dumps(meta))
        os.makedirs(gt_ref.HERE, exist_ok=True)
        path = os.path.join(gt_ref.HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"  wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
