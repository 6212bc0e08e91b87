"""Open SuperPoint golden fixtures (tests/golden/sp_open/spo_*.npz, made by
tests/golden/make_sp_open_golden.py): regenerate a case's inputs and weights from its recipe, load
its reference outputs, and the error bars the fixtures' own fp32-vs-fp64 error sets."""
import glob
import json
import os

import numpy as np

from lightglue_amd.sp_weights import superpoint_open_state_dict, synthetic_images
from sp_golden_util import sha as sha_inputs  # noqa: F401  (SHA-256 over a dict of arrays)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp_open")
# The nonfree extractor's bars (tests/test_gpu_superpoint.py; the arithmetic is the same fp16x3), or
# six times the reference's own fp32-vs-fp64 error where that is larger: 6 is the ratio measured on
# the nonfree extractor (7.5e-7 GPU-vs-reference over 1.3e-7 reference-vs-fp64), rounded up.
SCORE_FLOOR, DESC_FLOOR, REF_ERR_FACTOR = 2e-6, 2e-5, 6.0


def spo_case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "spo_*.npz")))


def spo_load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    g = {k: z[k] for k in z.files if k != "meta_json"}
    g["meta"] = json.loads(str(z["meta_json"]))
    return g


def spo_case_inputs(meta):
    """(conf, state dict, data) of a case."""
    sd = superpoint_open_state_dict(seed=meta["w_seed"])
    image = synthetic_images(meta["B"], meta["C"], meta["H"], meta["W"], seed=meta["img_seed"])
    return dict(meta["conf"]), sd, {"image": image}


def spo_bars(meta):
    """(score bar, descriptor bar) of a fixture."""
    return max(SCORE_FLOOR, REF_ERR_FACTOR * meta["e_scores"]), max(DESC_FLOOR, REF_ERR_FACTOR * meta["e_desc"])


def assert_same_keypoints(out, ref_k, ref_s, ref_d, score_atol, desc_atol):
    """Same keypoint set per image, scores positionally within score_atol, descriptors per keypoint
    within desc_atol.  The sorted top-k order may differ only between keypoints whose scores are
    closer than the bar (the positional score check bounds that).  Returns the number of keypoints
    found at another position."""
    ok, os_, od = (np.asarray(out[k]) for k in ("keypoints", "keypoint_scores", "descriptors"))
    assert ok.shape == ref_k.shape
    err_s = float(np.abs(os_ - ref_s).max()) if os_.size else 0.0
    swaps, err_d = 0, 0.0
    for b in range(ok.shape[0]):
        where = {tuple(p): i for i, p in enumerate(ref_k[b])}
        idx = [where.get(tuple(p), -1) for p in ok[b]]
        assert -1 not in idx and sorted(idx) == list(range(len(idx))), "different keypoint sets"
        swaps += int(np.sum(np.asarray(idx) != np.arange(len(idx))))
        if len(idx):
            err_d = max(err_d, float(np.abs(od[b] - ref_d[b][idx]).max()))
    print(f"max score error {err_s:.3g} (bar {score_atol:.3g}), max descriptor error {err_d:.3g} (bar {desc_atol:.3g}), "
          f"{swaps} keypoints at other positions")
    assert err_s <= score_atol, (err_s, score_atol)
    assert err_d <= desc_atol, (err_d, desc_atol)
    return swaps
