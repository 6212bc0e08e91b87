"""ALIKED golden fixtures (tests/golden/aliked/*.npz, made by tests/golden/make_aliked_golden.py by
running the real reference): regenerate a case's inputs and weights from its recipe, load its
reference outputs, the error bars the fixtures' own fp32-vs-fp64 error sets, and the comparison.

Bars:

* scores (score map, sampled score): ``max(2e-6, 6 e_scores)``; descriptors: ``max(2e-5, 6 e_desc)``
  -- the project's floors for this arithmetic class, 6 the ratio measured in DESIGN.md §9b;
* keypoints in pixels: ``max(6 e_kpts, (4 radius / T) score_bar)``, T = 0.1: the second term is the
  soft-argmax's sensitivity to a score error (a window of weights exp(s / T) moves by at most
  radius * 2 * delta / T when every score moves by delta, doubled for the normalising sum);
* dispersity: the same form, ``max(6 e_disp, (4 radius / T) score_bar)`` (its terms are squared
  distances in units of the radius, each at most 4 and as sensitive).

``e_*`` come from the fixture (the reference's fp32 run against its fp64 run), never from the code
under test.
"""
import glob
import json
import os

import numpy as np

from lightglue_amd.aliked_weights import aliked_state_dict
from lightglue_amd.sp_weights import synthetic_images
from sp_golden_util import sha  # noqa: F401  (SHA-256 over a dict of arrays)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aliked")
SCORE_FLOOR, DESC_FLOOR, REF_ERR_FACTOR, TEMPERATURE = 2e-6, 2e-5, 6.0, 0.1
MATCH_TOL = 0.05  # pixels: two runs' keypoints are the same point when closer than this, one to one


def aliked_case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def aliked_load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    g = {k: z[k] for k in z.files if k != "meta_json"}
    g["meta"] = json.loads(str(z["meta_json"]))
    return g


def aliked_case_inputs(meta):
    """(conf, state dict, data) of a case."""
    sd = aliked_state_dict(meta["conf"]["model_name"], seed=meta["w_seed"])
    data = {"image": synthetic_images(meta["B"], 3, meta["H"], meta["W"], seed=meta["img_seed"])}
    if meta.get("image_size") is not None:
        data["image_size"] = np.asarray(meta["image_size"], np.float32)
    return dict(meta["conf"]), sd, data


def aliked_bars(e_scores, e_desc, e_kpts, e_disp, radius):
    score = max(SCORE_FLOOR, REF_ERR_FACTOR * e_scores)
    soft = 4.0 * radius / TEMPERATURE * score
    return {"score": score, "desc": max(DESC_FLOOR, REF_ERR_FACTOR * e_desc), "kpts": max(REF_ERR_FACTOR * e_kpts, soft),
            "disp": max(REF_ERR_FACTOR * e_disp, soft)}


def fixture_bars(meta):
    return aliked_bars(meta["e_scores"], meta["e_desc"], meta["e_kpts"], meta["e_disp"], int(meta["conf"].get("nms_radius", 2)))


def match_points(a, b):
    """Index into b of each point of a: the same set, one to one, each pair closer than MATCH_TOL."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, f"different keypoint counts: {a.shape} against {b.shape}"
    if len(a) == 0:
        return np.zeros(0, np.int64)
    d = np.abs(a[:, None] - b[None]).max(-1)
    idx = d.argmin(1)
    assert float(d[np.arange(len(a)), idx].max()) < MATCH_TOL, "different keypoint sets"
    assert len(set(idx.tolist())) == len(idx), "different keypoint sets (two points on one)"
    return idx


def compare(out, ref, bars, label=""):
    """out / ref: dicts of arrays (or per-image lists) under the reference's keys.  Same keypoint set
    per image; per keypoint the sub-pixel position, descriptor, keypoint_scores (the dispersity) and
    score_dispersity (the sampled score) within the bars; score_map within the score bar.  Inside
    the order, only keypoints whose sampled scores differ by less than the score bar may trade
    places.  Prints the maxima before asserting and returns them."""
    err = {"score_map": float(np.abs(np.asarray(out["score_map"], np.float64) - np.asarray(ref["score_map"], np.float64)).max()),
           "kpts": 0.0, "desc": 0.0, "disp": 0.0, "score": 0.0}
    swaps, bad_swaps = 0, 0
    B = len(ref["keypoints"])
    assert len(out["keypoints"]) == B
    matched = []
    for b in range(B):
        ok, rk = np.asarray(out["keypoints"][b], np.float64), np.asarray(ref["keypoints"][b], np.float64)
        idx = match_points(ok, rk)
        matched.append(idx)
        if not len(idx):
            continue
        err["kpts"] = max(err["kpts"], float(np.abs(ok - rk[idx]).max()))
        for key, e in (("descriptors", "desc"), ("keypoint_scores", "disp"), ("score_dispersity", "score")):
            o, r = np.asarray(out[key][b], np.float64), np.asarray(ref[key][b], np.float64)
            err[e] = max(err[e], float(np.abs(o - r[idx]).max()))
        moved = np.nonzero(idx != np.arange(len(idx)))[0]
        swaps += len(moved)
        # a moved keypoint sits where a reference keypoint of (nearly) the same NMS score sat; the
        # NMS score is the raw score at the pixel, within the score bar of the sampled maximum's
        # neighbourhood: compare the reference's values at the two positions
        if len(moved) and "order_scores" in ref:
            rs = np.asarray(ref["order_scores"][b], np.float64)
            bad_swaps += int(np.sum(np.abs(rs[idx[moved]] - rs[moved]) >= bars["score"]))
    print(f"{label}: score_map {err['score_map']:.3g} sampled score {err['score']:.3g} (bar {bars['score']:.3g}); "
          f"keypoints {err['kpts']:.3g} px (bar {bars['kpts']:.3g}); descriptors {err['desc']:.3g} (bar {bars['desc']:.3g}); "
          f"dispersity {err['disp']:.3g} (bar {bars['disp']:.3g}); {swaps} keypoints at other positions")
    assert err["score_map"] <= bars["score"], (err["score_map"], bars["score"])
    assert err["score"] <= bars["score"], (err["score"], bars["score"])
    assert err["kpts"] <= bars["kpts"], (err["kpts"], bars["kpts"])
    assert err["desc"] <= bars["desc"], (err["desc"], bars["desc"])
    assert err["disp"] <= bars["disp"], (err["disp"], bars["disp"])
    if "order_scores" in ref:
        assert bad_swaps == 0, f"{bad_swaps} keypoints moved past a score gap above the bar"
    else:
        assert swaps == 0, f"{swaps} keypoints at other positions"
    return err
