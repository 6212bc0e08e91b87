#!/usr/bin/env python3
"""Golden vectors for the open SuperPoint extractor, made by running the REAL reference here.

Run from the repo root (needs ``/root/reference``, which does not exist on the GPU box)::

    python tests/golden/make_sp_open_golden.py

Harness only (nothing here ships), in the manner of ``make_superpoint_golden.py``:

* the ``omegaconf`` stand-in and synthetic package objects whose ``__path__`` points into
  ``/root/reference`` (plus ``gluefactory.models.extractors``), so the REAL
  ``gluefactory.models.extractors.superpoint_open`` loads without the training stack;
* ``torch.hub.load_state_dict_from_url`` (``superpoint_open.py:114``) is replaced by a function
  returning the recipe weights (``lightglue_amd.sp_weights.superpoint_open_state_dict``) BEFORE the
  reference's ``SuperPoint`` is constructed: the trained checkpoint is a download, nothing here
  reaches the network;
* ``SuperPoint(conf).eval()(data)`` runs in fp32 on the recipe images; the outputs go to
  ``tests/golden/sp_open/<case>.npz``.  Inputs and weights are regenerated from the recipe in the
  tests (their SHA-256 is stored);
* the same model runs again in fp64 (``sample_descriptors`` wrapped so the keypoints take the
  descriptor dtype; it fails on the dtype mismatch otherwise).  The meta stores ``e_scores`` /
  ``e_desc`` (max |fp32 - fp64| over matched keypoints, and over the dense map where stored), the
  per-image ``kth_gap`` (k-th minus (k+1)-th best candidate score), ``positive`` (candidates with a
  positive score) and ``thr_gap`` (smallest |score - threshold| over the non-border pixels the NMS
  kept), all from the fp64 run;
* decidability is asserted (pick other seeds if it fails): fp32 and fp64 keypoint sets identical,
  ``kth_gap`` and ``thr_gap`` above 4x the score bar ``max(2e-6, 6 e_scores)``, and with a negative
  threshold at least k positive candidates per image (no zero-score tie is selected).
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
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import lgamd  # noqa: E402,F401
from lightglue_amd.sp_weights import superpoint_open_state_dict, synthetic_images  # noqa: E402
from make_golden import _ADict, _merge  # noqa: E402
from make_superpoint_golden import sha  # noqa: E402

OUT = os.path.join(HERE, "sp_open")
CASES = {
    # name: (B, C, H, W, conf, img_seed, w_seed)
    "spo_gray_b1_100x132_k150": (1, 1, 100, 132, {"max_num_keypoints": 150}, 21, 1),
    "spo_rgb_b2_72x88_k64_thrneg": (2, 3, 72, 88, {"max_num_keypoints": 64, "detection_threshold": -1, "nms_radius": 3,
                                                  "force_num_keypoints": True}, 22, 2),
    "spo_dense_b1_64x80": (1, 1, 64, 80, {"max_num_keypoints": None, "dense_outputs": True}, 23, 3),
}


def install_shim():
    om = types.ModuleType("omegaconf")

    class OmegaConf:
        merge = staticmethod(_merge)
        create = staticmethod(lambda d=None: _merge(d or {}))
        to_container = staticmethod(lambda d: dict(d))
        set_struct = staticmethod(lambda *a, **k: None)
        set_readonly = staticmethod(lambda *a, **k: None)

    om.OmegaConf = OmegaConf
    om.DictConfig = _ADict
    sys.modules["omegaconf"] = om
    for name, path in [
        ("gluefactory", "gluefactory"),
        ("gluefactory.models", "gluefactory/models"),
        ("gluefactory.models.utils", "gluefactory/models/utils"),
        ("gluefactory.models.extractors", "gluefactory/models/extractors"),
    ]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("gluefactory.models.extractors.superpoint_open")


def candidate_map(mod, model, image):
    """The reference's own steps up to the threshold (superpoint_open.py:118-143) on its modules."""
    if image.shape[1] == 3:
        image = (image * image.new_tensor([0.299, 0.587, 0.114]).view(1, 3, 1, 1)).sum(1, keepdim=True)
    s = torch.nn.functional.softmax(model.detector(model.backbone(image)), 1)[:, :-1]
    b, _, h, w = s.shape
    s = s.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
    s = mod.batched_nms(s, model.conf.nms_radius)
    pad = model.conf.remove_borders
    inner = torch.zeros_like(s, dtype=torch.bool)
    inner[:, pad:s.shape[1] - pad, pad:s.shape[2] - pad] = True
    return torch.where(inner, s, -torch.ones_like(s)), inner


def run_case(mod, name, spec):
    B, C, H, W, conf, img_seed, w_seed = spec
    sd = superpoint_open_state_dict(seed=w_seed)
    image = synthetic_images(B, C, H, W, seed=img_seed)
    real_hub = torch.hub.load_state_dict_from_url
    torch.hub.load_state_dict_from_url = lambda *a, **k: {n: torch.from_numpy(np.array(v)) for n, v in sd.items()}
    try:
        model = mod.SuperPoint(dict(conf)).eval()
    finally:
        torch.hub.load_state_dict_from_url = real_hub
    ref_keys = list(model.state_dict())
    with torch.no_grad():
        pred = model({"image": torch.from_numpy(image)})
        # fp64: the same module, doubled; sample_descriptors takes float keypoints (:154)
        real_sample = mod.sample_descriptors
        mod.sample_descriptors = lambda k, d, s=8: real_sample(k.to(d.dtype), d, s)
        try:
            model64 = model.double()
            pred64 = model64({"image": torch.from_numpy(image).double()})
            cand, inner = candidate_map(mod, model64, torch.from_numpy(image).double())
        finally:
            mod.sample_descriptors = real_sample
    out = {f"out_{k}": v.numpy() for k, v in pred.items()}
    thr = float(model.conf.detection_threshold)
    k = conf.get("max_num_keypoints")
    e_scores = e_desc = 0.0
    for b in range(B):
        where = {tuple(p): i for i, p in enumerate(pred64["keypoints"][b].numpy())}
        idx = [where.get(tuple(p), -1) for p in pred["keypoints"][b].numpy()]
        assert -1 not in idx and sorted(idx) == list(range(len(idx))), f"{name}: fp32 and fp64 keypoint sets differ"
        e_scores = max(e_scores, float((pred["keypoint_scores"][b].double() - pred64["keypoint_scores"][b][idx]).abs().max()))
        e_desc = max(e_desc, float((pred["descriptors"][b].double() - pred64["descriptors"][b][idx]).abs().max()))
    if "dense_descriptors" in pred:
        e_desc = max(e_desc, float((pred["dense_descriptors"].double() - pred64["dense_descriptors"]).abs().max()))
    gaps, positive, thr_gap = [], [], []
    for b in range(B):
        c = cand[b][cand[b] > thr]
        v = torch.sort(c, descending=True).values
        gaps.append(float(v[k - 1] - v[k]) if k is not None and k < len(v) else float("inf"))
        positive.append(int((cand[b] > 0).sum()))
        kept = cand[b][inner[b] & (cand[b] > 0)]
        thr_gap.append(float((kept - thr).abs().min()))
    bar = max(2e-6, 6 * e_scores)
    assert min(gaps) > 4 * bar and min(thr_gap) > 4 * bar, (name, gaps, thr_gap, bar)
    if thr < 0:
        assert k is not None and min(positive) >= k, (name, positive)
    meta = {"B": B, "C": C, "H": H, "W": W, "conf": conf, "img_seed": img_seed, "w_seed": w_seed,
            "inputs_sha256": sha({"image": image}), "weights_sha256": sha(sd), "ref_state_dict_keys": ref_keys,
            "e_scores": e_scores, "e_desc": e_desc, "kth_gap": gaps, "positive": positive, "thr_gap": thr_gap,
            "counts": [int((cand[b] > thr).sum()) for b in range(B)]}
    out["meta_json"] = np.array(json.dumps(meta))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **out)
    print(name, {k_: v.shape for k_, v in out.items() if k_ != "meta_json"},
          {k_: meta[k_] for k_ in ("e_scores", "e_desc", "kth_gap", "positive", "thr_gap", "counts")},
          "scores", float(pred["keypoint_scores"].min()), float(pred["keypoint_scores"].max()))


def main():
    mod = install_shim()
    only = sys.argv[1:]
    for name, spec in CASES.items():
        if not only or name in only:
            run_case(mod, name, spec)


if __name__ == "__main__":
    main()
