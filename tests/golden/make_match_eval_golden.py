"""Generate tests/golden/match_eval/match_eval.npz: inputs and expected outputs of the batched match evaluation
(lightglue_amd.match_eval), from the reference's own functions:

* ``sym_homography_error`` (gluefactory/geometry/homography.py:314-323),
* ``generalized_epi_dist(..., all=False, essential=True)`` (geometry/epipolar.py:75-85) on the
  reference's ``Camera`` / ``Pose`` wrappers (geometry/wrappers.py),
* for the DLT, this project's float-for-float restatement ``hpatches_metrics.eval_homography_dlt``
  (kornia is not installed), in fp32 and on fp64 copies of the fp32 inputs.

Run in the build container (the reference is at /root/reference; it is not needed at test time):
    python tests/golden/make_match_eval_golden.py
The geometry modules need only numpy and torch and are imported through synthetic ``gluefactory`` /
``gluefactory.geometry`` packages, as in make_metric_golden.py.

Every pair is a planar scene seen by two pinhole cameras, so one set of matches serves all three
metrics: H_0to1 = K1 (R + t n^T / d) K0^-1.  Keypoints are uniform in the image, matched partners are
warped by H_0to1 plus Gaussian noise of 0.3, 2 or 20 px, scores are uniform in [0.1, 1].

Two conditions are asserted (a case's seed is advanced until they hold):
* every live match's fp64 error is at least a relative 1e-3 away from every threshold it meets, so
  the fp32 and fp64 counts must agree and an exact comparison of counts is meaningful;
* the reference's fp32 counts equal the fp64 counts.
``dlt_rel_bar`` is the largest |fp32 - fp64| / fp64 of the host DLT error over the pairs with at least
4 matches: the bar for the kernel's ``H_error_dlt`` against the fp64 value.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "match_eval", "match_eval.npz")
sys.path.insert(0, ROOT)

HOM_T = (1.0, 3.0)
EPI_T = (1e-4, 5e-4, 1e-3)
MARGIN = 1e-3

# name -> pairs of (M, N, live matches, image size)
CASES = {
    "a": [(5, 7, 4, (640, 480))],
    "b": [(64, 64, 33, (640, 480))],
    "c": [(65, 130, 65, (640, 480))],
    "d": [(257, 300, 200, (640, 480))],
    "e": [(300, 257, 256, (640, 480))],
    "f": [(512, 512, 257, (640, 480))],
    "g": [(40, 50, 0, (640, 480))],
    "h": [(40, 50, 3, (640, 480))],
    "j": [(100, 120, 60, (640, 480)), (100, 120, 75, (512, 384))],
}
RAGGED = ("a", "b", "c")  # case i: these three padded to one capacity


def reference_modules():
    for name, path in [("gluefactory", "gluefactory"), ("gluefactory.geometry", "gluefactory/geometry")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join("/root/reference", path)]
        sys.modules.setdefault(name, m)
    hom = importlib.import_module("gluefactory.geometry.homography")
    epi = importlib.import_module("gluefactory.geometry.epipolar")
    wr = importlib.import_module("gluefactory.geometry.wrappers")
    return hom, epi, wr


def rotation(aa):
    th = np.linalg.norm(aa)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_pair(rng, M, N, live, size):
    W, Hh = size
    cams = []
    for _ in range(2):
        fx = rng.uniform(400, 600)
        fy = fx * rng.uniform(0.85, 1.15)
        cx, cy = W / 2 + rng.uniform(-20, 20), Hh / 2 + rng.uniform(-20, 20)
        cams.append([W, Hh, fx, fy, cx, cy])
    R = rotation(rng.normal(0, 0.08, 3))
    t = rng.normal(0, 0.4, 3)
    T = np.concatenate([R.reshape(-1), t]).astype(np.float32)
    # the plane z = 5 of camera 0; from the fp32 pose and cameras the tests will see
    R32, t32 = T[:9].astype(np.float64).reshape(3, 3), T[9:].astype(np.float64)
    cam = np.asarray(cams, dtype=np.float32)
    K0, K1 = [np.array([[c[2], 0, c[4]], [0, c[3], c[5]], [0, 0, 1]], dtype=np.float64) for c in cam]
    H = K1 @ (R32 + np.outer(t32, [0, 0, 1]) / 5.0) @ np.linalg.inv(K0)
    H = (H / H[2, 2]).astype(np.float32)
    k0 = (rng.uniform(0, 1, (M, 2)) * [W, Hh]).astype(np.float32)
    k1 = (rng.uniform(0, 1, (N, 2)) * [W, Hh]).astype(np.float32)
    m0 = np.full(M, -1, dtype=np.int64)
    sel, dst = rng.permutation(M)[:live], rng.permutation(N)[:live]
    q = np.concatenate([k0[sel].astype(np.float64), np.ones((live, 1))], 1) @ H.astype(np.float64).T
    sigma = rng.choice([0.3, 2.0, 20.0], size=(live, 1), p=[0.4, 0.3, 0.3])
    k1[dst] = (q[:, :2] / q[:, 2:] + rng.normal(0, 1, (live, 2)) * sigma).astype(np.float32)
    m0[sel] = dst
    s0 = rng.uniform(0.1, 1.0, M).astype(np.float32)
    return {"kpts0": k0, "kpts1": k1, "matches0": m0, "scores0": s0, "H": H.reshape(3, 3),
            "size0": np.asarray(size, dtype=np.float32), "cam0": cam[0], "cam1": cam[1], "T": T}


def reference_pair(mods, p):
    """The reference's per-match errors in fp32 and fp64, the counts of both, the host DLT of both."""
    import lgamd  # noqa: F401
    from lightglue_amd import hpatches_metrics as hm

    hom, epi, wr = mods
    t = {k: torch.from_numpy(v) for k, v in p.items()}
    M = t["kpts0"].shape[0]
    live = t["matches0"] > -1
    out = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        k0, k1, H = t["kpts0"].to(dt), t["kpts1"].to(dt), t["H"].to(dt)
        pts0, pts1, sc = hm.get_matches_scores(k0, k1, t["matches0"], t["scores0"])
        he = hom.sym_homography_error(pts0, pts1, H)
        ee = epi.generalized_epi_dist(pts0[None], pts1[None], wr.Camera(t["cam0"].to(dt)[None]),
                                      wr.Camera(t["cam1"].to(dt)[None]), wr.Pose(t["T"].to(dt)[None]), False,
                                      essential=True)[0]
        for key, e in (("hom", he), ("epi", ee)):
            full = torch.full((M,), float("nan"), dtype=torch.float64)
            full[live] = e.double()
            out[f"{key}_err{name}"] = full.numpy()
        n = int(live.sum())
        out[f"hom_counts{name}"] = np.array([n] + [int((he < th).sum()) for th in HOM_T], dtype=np.int32)
        out[f"epi_counts{name}"] = np.array([n] + [int((ee < th).sum()) for th in EPI_T], dtype=np.int32)
        data = {"H_0to1": H, "view0": {"image_size": t["size0"].to(dt)}}
        pred = {"keypoints0": k0, "keypoints1": k1, "matches0": t["matches0"], "matching_scores0": t["scores0"]}
        out[f"dlt_err{name}"] = np.float64(hm.eval_homography_dlt(data, pred)["H_error_dlt"])
        if name == "64":
            out["H_dlt64"] = (hm.find_homography_dlt(pts0[None], pts1[None], sc.to(dt)[None])[0].numpy() if n >= 4
                              else np.full((3, 3), np.inf))
    return out


def acceptable(ref):
    for key, ths in (("hom", HOM_T), ("epi", EPI_T)):
        e = ref[f"{key}_err64"]
        e = e[~np.isnan(e)]
        for th in ths:
            if e.size and np.abs(e - th).min() < MARGIN * th:
                return False
        if not np.array_equal(ref[f"{key}_counts32"], ref[f"{key}_counts64"]):
            return False
    return True


def main():
    mods = reference_modules()
    store, pairs, rel = {}, {}, []
    for ci, (name, specs) in enumerate(CASES.items()):
        got = []
        for pi, (M, N, live, size) in enumerate(specs):
            for attempt in range(500):
                seed = 100000 * (ci + 1) + 1000 * pi + attempt
                p = make_pair(np.random.default_rng(seed), M, N, live, size)
                ref = reference_pair(mods, p)
                if acceptable(ref):
                    break
            else:
                raise AssertionError(f"case {name}: no seed keeps every error {MARGIN} away from the thresholds")
            assert acceptable(ref)
            print(f"case {name}[{pi}]: seed {seed}, hom {ref['hom_counts64']}, epi {ref['epi_counts64']}, "
                  f"dlt {ref['dlt_err32']:.6g} / {ref['dlt_err64']:.6g}")
            if live >= 4:
                rel.append(abs(ref["dlt_err32"] - ref["dlt_err64"]) / ref["dlt_err64"])
            got.append((p, ref))
        pairs[name] = got
        for k in got[0][0]:
            store[f"{name}/{k}"] = np.stack([p[k] for p, _ in got])
        for k in ("hom_err32", "hom_err64", "epi_err32", "epi_err64", "dlt_err32", "dlt_err64", "H_dlt64"):
            store[f"{name}/{k}"] = np.stack([r[k] for _, r in got])
        store[f"{name}/hom_counts"] = np.stack([r["hom_counts64"] for _, r in got])
        store[f"{name}/epi_counts"] = np.stack([r["epi_counts64"] for _, r in got])

    # case i: a, b, c padded to one capacity; the padding holds arbitrary keypoints and scores and
    # stale, valid-looking match indices
    rng = np.random.default_rng(9)
    src = [pairs[n][0] for n in RAGGED]
    Mc, Nc = max(p["kpts0"].shape[0] for p, _ in src), max(p["kpts1"].shape[0] for p, _ in src)
    B = len(src)
    pad = {"kpts0": (rng.uniform(0, 480, (B, Mc, 2))).astype(np.float32),
           "kpts1": (rng.uniform(0, 480, (B, Nc, 2))).astype(np.float32),
           "matches0": rng.integers(0, Nc, (B, Mc)).astype(np.int64),
           "scores0": rng.uniform(0.1, 1.0, (B, Mc)).astype(np.float32)}
    num0, num1 = [], []
    for b, (p, _) in enumerate(src):
        m, n = p["kpts0"].shape[0], p["kpts1"].shape[0]
        pad["kpts0"][b, :m], pad["kpts1"][b, :n] = p["kpts0"], p["kpts1"]
        pad["matches0"][b, :m], pad["scores0"][b, :m] = p["matches0"], p["scores0"]
        num0.append(m), num1.append(n)
    for k, v in pad.items():
        store[f"i/{k}"] = v
    for k in ("H", "size0", "cam0", "cam1", "T"):
        store[f"i/{k}"] = np.stack([p[k] for p, _ in src])
    store["i/num0"], store["i/num1"] = np.asarray(num0, dtype=np.int32), np.asarray(num1, dtype=np.int32)
    for k in ("dlt_err32", "dlt_err64", "H_dlt64"):
        store[f"i/{k}"] = np.stack([r[k] for _, r in src])
    store["i/hom_counts"] = np.stack([r["hom_counts64"] for _, r in src])
    store["i/epi_counts"] = np.stack([r["epi_counts64"] for _, r in src])
    for k in ("hom_err64", "epi_err64"):
        full = np.full((B, Mc), np.nan)
        for b, (_, r) in enumerate(src):
            full[b, :r[k].shape[0]] = r[k]
        store[f"i/{k}"] = full

    store["dlt_rel_bar"] = np.float64(max(rel))
    store["margin"] = np.float64(MARGIN)
    print(f"dlt_rel_bar = {max(rel):.3e} over {len(rel)} pairs")
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
