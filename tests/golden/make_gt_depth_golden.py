#!/usr/bin/env python3
"""Generate the pose-and-depth ground-truth fixtures by running the REAL reference.

Run from the repo root where the reference checkout exists (it does not on the GPU box)::

    python tests/golden/make_gt_depth_golden.py

Imports the reference's ``gluefactory/geometry/gt_generation.py`` and ``wrappers.py`` through the shim
of make_gt_golden.py (synthetic package objects, stand-ins for ``omegaconf``, ``kornia`` and ``cv2``,
none of which ``gt_matches_from_pose_depth`` touches), runs it in fp32 and in fp64 on inputs from the
NumPy PCG64 recipes below and writes ``tests/golden/gt_depth/gtd_*.npz``: the inputs and, per variant
(a set of thresholds on the same inputs), the reference's fp32 outputs (``assignment`` as index
triples, ``reward`` as int8), the fp64 continuous outputs and the undecidable masks.

The exact case: every fp32 operation of the chain is exact, so the reference's fp32 and fp64 runs must
agree bit for bit in all twelve outputs (asserted; change the recipe, not the assertion).

The random cases are gated (tests/gt_depth_ref.py:margins).  Every tolerance is 4 x the largest
deviation between the fp32 and the fp64 run of the chain for that quantity
(tests/gt_depth_ref.py:tolerances -- the restatement, which is first asserted to reproduce the
reference's twelve outputs bit for bit in both precisions, because the reference does not hand out
its intermediates).  Asserted here (change a failing seed, not the cap): undecidable points <= 1 %,
undecidable rows + columns <= 3 %, undecidable reward entries <= 0.1 %, the reference's own fp32 and
fp64 runs agree on everything decidable, and the th_epi variants of the 300 x 257 cases have at least
5 labels that the epipolar step changes.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gt_depth_ref as R  # noqa: E402
from make_gt_golden import install_shim  # noqa: E402


def exact_case(seed, B, M, N):
    """512 x 512 pinhole cameras with f = c = 256, depth 4 except a dozen zero rectangles per map,
    R = I, t = (0.125, -0.0625, 0): a shift of (8, -4) px.  Keypoints at integer + 0.5 in [40, 440);
    image 1 is image 0 shifted plus integer offsets in [-3, 3]; the last quarter of each image
    duplicates its first quarter (tied minima)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    S = 512
    cam = np.tile(np.array([S, S, 256.0, 256.0, 256.0, 256.0]), (B, 1))
    T01 = np.tile(np.concatenate([np.eye(3).reshape(9), [0.125, -0.0625, 0.0]]), (B, 1))
    T10 = np.tile(np.concatenate([np.eye(3).reshape(9), [-0.125, 0.0625, 0.0]]), (B, 1))
    depth = np.full((2, B, S, S), 4.0)
    kp0 = rng.integers(40, 440, (B, M, 2)) + 0.5
    kp0[:, M - M // 4:] = kp0[:, : M // 4]
    kp1 = np.empty((B, N, 2))
    for b in range(B):
        src = rng.permutation(M)[:N]
        kp1[b] = kp0[b, src] + np.array([8.0, -4.0]) + rng.integers(-3, 4, (N, 2))
    kp1[:, N - N // 4:] = kp1[:, : N // 4]
    for k, kp in ((0, kp0), (1, kp1)):
        for b in range(B):
            for r in range(12):  # half of the rectangles sit on a keypoint, some with the point on their border
                hw, hh = rng.integers(6, 40, 2)
                if r % 2 == 0:
                    p = kp[b, rng.integers(0, kp.shape[1])].astype(int)
                    x0, y0 = p[0] - rng.integers(0, 2) * (hw - 1) - rng.integers(0, 2), p[1] - rng.integers(0, hh)
                else:
                    x0, y0 = rng.integers(0, S - hw), rng.integers(0, S - hh)
                x0, y0 = max(int(x0), 0), max(int(y0), 0)
                depth[k, b, y0:y0 + hh, x0:x0 + hw] = 0.0
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))  # noqa: E731
    return {"keypoints0": f32(kp0), "keypoints1": f32(kp1), "depth0": f32(depth[0]), "depth1": f32(depth[1]),
            "camera0": f32(cam), "camera1": f32(cam), "T_0to1": f32(T01), "T_1to0": f32(T10)}


def plane(n_dist, holes=12):
    def recipe(seed, B, M, N):
        return R.plane_scene(seed, B, M, N, n_dist=n_dist, width=256, height=192, holes=holes)
    return recipe


def V(prefix, pos=3.0, neg=5.0, epi=None, cc=None):
    return {"prefix": prefix, "th_positive": pos, "th_negative": neg, "th_epi": epi, "th_consistency": cc}


# th_epi with th_negative 3: with 5 the ignored set is so large that nearly every point without depth has
# an ignored point within 5 px of its epipolar line and the step relabels next to nothing (0 to 6 labels
# here, whatever the share of zero rectangles); with 3 it relabels 20 to 40
THREE = [V("plain_"), V("cc_", cc=4.0), V("ccepi_", neg=3.0, cc=4.0, epi=1.0)]
CASES = [
    # name, recipe, seed, B, M, N, variants, precomputed depths
    ("gtd_exact_b3_m64_n48", exact_case, 11, 3, 64, 48, [V("plain_"), V("cc_", cc=1.0), V("ccepi_", cc=1.0, epi=1.0)], False),
    ("gtd_rand_nd0_b2_m300_n257", plane(0, holes=12), 31, 2, 300, 257, THREE, False),
    ("gtd_rand_nd2_b2_m300_n257", plane(2, holes=12), 32, 2, 300, 257, THREE, False),
    ("gtd_rand_nd4_b2_m300_n257", plane(4, holes=12), 33, 2, 300, 257, THREE, False),
    ("gtd_rand_b1_m37_n1100", plane(0), 34, 1, 37, 1100, [V("plain_"), V("ccepi_", cc=4.0, epi=1.0)], False),
    ("gtd_rand_b1_m1100_n37", plane(2), 35, 1, 1100, 37, [V("plain_"), V("ccepi_", cc=4.0, epi=1.0)], False),
    ("gtd_th_b2_m128_n128", plane(0), 36, 2, 128, 128, [V("n2_", neg=2.0), V("n6_", neg=6.0)], False),
    ("gtd_pre_b2_m128_n128", plane(4), 37, 2, 128, 128, [V("plain_"), V("epi_", epi=1.0)], True),
]


def ref_data(W, g, dtype, maps):
    t = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    view0, view1 = {"camera": W.Camera(t(g["camera0"]))}, {"camera": W.Camera(t(g["camera1"]))}
    if maps:
        view0["depth"], view1["depth"] = t(g["depth0"]), t(g["depth1"])
    return {"view0": view0, "view1": view1, "T_0to1": W.Pose(t(g["T_0to1"])), "T_1to0": W.Pose(t(g["T_1to0"]))}


def same_bits(a, b):
    a, b = a.numpy(), b.numpy()
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def main():
    gen = install_shim()
    import importlib

    W = importlib.import_module("gluefactory.geometry.wrappers")
    os.makedirs(R.HERE, exist_ok=True)
    for name, recipe, seed, B, M, N, variants, pre in CASES:
        g = recipe(seed, B, M, N)
        exact = recipe is exact_case
        out = dict(g)
        kw_np = None
        if pre:  # the depths a data loader would have cached: sampled once in fp32, the maps dropped
            d0, v0 = R.sample_depth(torch.from_numpy(g["keypoints0"]), torch.from_numpy(g["depth0"]))
            d1, v1 = R.sample_depth(torch.from_numpy(g["keypoints1"]), torch.from_numpy(g["depth1"]))
            kw_np = {"in_depth_keypoints0": d0.numpy(), "in_depth_keypoints1": d1.numpy(), "in_valid0": v0.numpy(),
                     "in_valid1": v1.numpy()}
            out.update(kw_np)
            del out["depth0"], out["depth1"]
            g = {k: v for k, v in g.items() if not k.startswith("depth")}
        meta = {"B": B, "M": M, "N": N, "seed": seed, "exact": exact, "precomputed": pre, "variants": []}
        for v in variants:
            pos, neg, epi, cc = v["th_positive"], v["th_negative"], v["th_epi"], v["th_consistency"]
            runs, rest = {}, {}
            for dt in (torch.float32, torch.float64):
                kw = {}
                if pre:
                    kw = {"depth_keypoints0": torch.from_numpy(kw_np["in_depth_keypoints0"]).to(dt),
                          "depth_keypoints1": torch.from_numpy(kw_np["in_depth_keypoints1"]).to(dt),
                          "valid_depth_keypoints0": torch.from_numpy(kw_np["in_valid0"]),
                          "valid_depth_keypoints1": torch.from_numpy(kw_np["in_valid1"])}
                k0, k1 = torch.from_numpy(g["keypoints0"]).to(dt), torch.from_numpy(g["keypoints1"]).to(dt)
                runs[dt] = gen.gt_matches_from_pose_depth(k0, k1, ref_data(W, g, dt, not pre), pos_th=pos, neg_th=neg,
                                                          epi_th=epi, cc_th=cc, **kw)
                d = R.feed_of(g, dt)
                rest[dt] = R.gt_matches_from_pose_depth(k0, k1, d, pos, neg, epi, cc, **kw)
                assert list(runs[dt]) == R.KEYS
                for k in R.KEYS:  # the restatement is the reference, bit for bit
                    assert same_bits(runs[dt][k], rest[dt][k]), (name, v["prefix"], dt, k)
            r32, r64 = runs[torch.float32], runs[torch.float64]
            assert r32["reward"].dtype == torch.float32 and r32["matches0"].dtype == torch.int64
            assert r32["assignment"].dtype == torch.bool and r32["visible0"].dtype == torch.bool
            p = v["prefix"]
            for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "depth_keypoints0", "depth_keypoints1",
                      "proj_0to1", "proj_1to0", "visible0", "visible1"):
                out[p + k] = r32[k].numpy()
            out[p + "assignment_idx"] = np.argwhere(r32["assignment"].numpy()).astype(np.int32)
            rw = r32["reward"].numpy()
            assert np.isin(rw, (-1.0, 0.0, 1.0)).all()
            out[p + "reward_i8"] = rw.astype(np.int8)
            m0, m1 = r32["matches0"].numpy(), r32["matches1"].numpy()
            lab = np.concatenate([m0.ravel(), m1.ravel()])
            stats = (f"matched {(lab > -1).sum()} unmatched {(lab == -1).sum()} ignored {(lab == -2).sum()} "
                     f"NaN depths {int(np.isnan(out[p + 'depth_keypoints0']).sum() + np.isnan(out[p + 'depth_keypoints1']).sum())} "
                     f"visible {int(out[p + 'visible0'].sum() + out[p + 'visible1'].sum())} reward values {sorted(set(np.unique(rw)))}")
            vm = dict(v)
            if exact:
                for k in R.KEYS:
                    a = r32[k].to(r64[k].dtype)  # fp32 -> fp64 is exact (reward and the scores are fp32 in both)
                    assert same_bits(a, r64[k]), f"{name} {p}{k}: the reference's fp32 and fp64 runs differ"
                out[p + "und_reward_idx"] = np.zeros((0, 3), np.int32)
                print(f"{name} {p}: {stats}")
            else:
                kw_t = R.precomputed_kw(out, meta) if pre else None
                tol = R.tolerances(g, pos, neg, epi, cc, kw_t)
                mg = R.margins(g, pos, neg, epi, cc, tol, kw_t)
                up = mg["und_p0"].sum() + mg["und_p1"].sum()
                urc = mg["und_rows"].sum() + mg["und_cols"].sum()
                ue = mg["und_reward"]
                assert up / (B * (M + N)) <= 0.01, (name, p, "points", up)
                assert urc / (B * (M + N)) <= 0.03, (name, p, "rows + columns", urc)
                assert ue.sum() / ue.size <= 0.001, (name, p, "reward", ue.sum() / ue.size)
                want64 = {k: r64[k].numpy() for k in R.KEYS}
                got32 = {k: r32[k].numpy() for k in R.KEYS}
                R.compare(got32, want64, mg, tol, False)  # the reference's two precisions agree where decidable
                if epi is not None and M == 300:
                    k0, k1 = torch.from_numpy(g["keypoints0"]), torch.from_numpy(g["keypoints1"])
                    kwp = R.precomputed_kw(out, meta) if pre else {}
                    before = gen.gt_matches_from_pose_depth(k0, k1, ref_data(W, g, torch.float32, not pre), pos_th=pos,
                                                            neg_th=neg, epi_th=None, cc_th=cc, **kwp)
                    changed = int((before["matches0"] != r32["matches0"]).sum() + (before["matches1"] != r32["matches1"]).sum())
                    assert changed >= 5, (name, p, "labels the epipolar step changes", changed)
                    stats += f" epi-changed {changed}"
                for k in ("und_p0", "und_p1", "und_rows", "und_cols"):
                    out[p + k] = mg[k]
                out[p + "und_reward_idx"] = np.argwhere(ue).astype(np.int32)
                for k in ("depth_keypoints0", "depth_keypoints1", "proj_0to1", "proj_1to0"):
                    out[p + k + "_f64"] = r64[k].numpy()
                vm["tol"] = tol
                print(f"{name} {p}: {stats}\n    undecidable points {int(up)} rows+cols {int(urc)}/{B * (M + N)} "
                      f"reward {int(ue.sum())}/{ue.size}; tol " + " ".join(f"{k} {x:.2e}" for k, x in tol.items()))
            meta["variants"].append(vm)
        out["meta_json"] = np.array(json.dumps(meta))
        path = os.path.join(R.HERE, name + ".npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print(f"  wrote {path} ({size} bytes)")


if __name__ == "__main__":
    main()
