#!/usr/bin/env python3
"""Golden vectors for the ALIKED extractor, made by running the REAL reference here.

Run from the repo root (needs ``/root/reference``, which does not exist on the GPU box)::

    python tests/golden/make_aliked_golden.py

Harness only (nothing here ships), in the manner of ``make_sp_open_golden.py``:

* the ``omegaconf`` stand-in and synthetic package objects whose ``__path__`` points into
  ``/root/reference``, so the REAL ``gluefactory.models.extractors.aliked`` loads without the
  training stack;
* a ``torchvision`` stand-in (torchvision is not installed): ``ops.deform_conv2d`` is the
  restatement's function (``tests/aliked_ref.py``, checked equal to ``F.conv2d`` at zero offsets
  before use), ``models.resnet.conv1x1`` / ``conv3x3`` are bias-free convolutions;
* ``torch.hub.load_state_dict_from_url`` (``aliked.py:727``) is replaced by a function returning the
  recipe weights (``lightglue_amd.aliked_weights.aliked_state_dict``) BEFORE the reference's
  ``ALIKED`` is constructed: the trained checkpoint is a download, nothing here reaches the network;
* ``ALIKED(conf).eval()(data)`` runs in fp32 and, doubled, in fp64 on the recipe images; the fp32
  outputs go to ``tests/golden/aliked/<case>.npz`` with a meta: SHA-256 of the regenerated inputs
  and weights, the reference's ``state_dict`` keys and shapes, ``e_scores`` / ``e_kpts`` / ``e_desc``
  / ``e_disp`` (max |fp32 - fp64|), the per-image ``kth_gap`` (k-th minus (k+1)-th NMS score),
  ``thr_gap`` (smallest |NMS score - threshold| over the positive candidates) and ``positive``;
* decidability is asserted, and the seeds move on until it holds: fp32 and fp64 keypoint sets
  identical, ``kth_gap`` and ``thr_gap`` above 4x the score bar ``max(2e-6, 6 e_scores)``, every
  image with at least k positive candidates, and ``e_desc`` below 1e-5 (a keypoint whose position
  truncates to another pixel in one precision shows up there).
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
sys.path.insert(0, os.path.dirname(HERE))
import lgamd  # noqa: E402,F401
import aliked_ref  # noqa: E402
from aliked_golden_util import MATCH_TOL, match_points  # noqa: E402
from lightglue_amd.aliked_weights import aliked_state_dict  # noqa: E402
from lightglue_amd.sp_weights import synthetic_images  # noqa: E402
from make_golden import _ADict, _merge  # noqa: E402
from make_superpoint_golden import sha  # noqa: E402

OUT = os.path.join(HERE, "aliked")
CASES = {
    # name: (B, H, W, conf, image_size, first img_seed, first w_seed); thr "auto": chosen below
    "aliked_n16_b2_72x100_k64": (2, 72, 100, {"model_name": "aliked-n16", "max_num_keypoints": 64,
                                              "detection_threshold": 0.0}, [[90, 60], [100, 72]], 31, 1),
    "aliked_t16_b1_30x70_k24": (1, 30, 70, {"model_name": "aliked-t16", "max_num_keypoints": 24,
                                            "detection_threshold": 0.0}, None, 32, 2),
    "aliked_n32_b1_64x96_k48": (1, 64, 96, {"model_name": "aliked-n32", "max_num_keypoints": 48,
                                            "detection_threshold": 0.0}, None, 33, 3),
    "aliked_n16_b1_64x96_thr": (1, 64, 96, {"model_name": "aliked-n16", "max_num_keypoints": -1,
                                            "detection_threshold": "auto"}, None, 34, 4),
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
    # torchvision stand-in
    x = torch.randn(2, 5, 7, 9, dtype=torch.float64)
    wt = torch.randn(6, 5, 3, 3, dtype=torch.float64)
    got = aliked_ref.deform_conv2d(x, torch.zeros(2, 18, 7, 9, dtype=torch.float64), wt, None, padding=(1, 1))
    assert float((got - torch.nn.functional.conv2d(x, wt, padding=1)).abs().max()) < 1e-12
    tv, ops, models, resnet = (types.ModuleType(n) for n in ("torchvision", "torchvision.ops", "torchvision.models",
                                                              "torchvision.models.resnet"))
    ops.deform_conv2d = lambda input, offset, weight, bias=None, padding=(0, 0), mask=None: aliked_ref.deform_conv2d(
        input, offset, weight, bias, padding=padding, mask=mask)
    resnet.conv1x1 = lambda i, o, stride=1: torch.nn.Conv2d(i, o, kernel_size=1, stride=stride, bias=False)
    resnet.conv3x3 = lambda i, o, stride=1: torch.nn.Conv2d(i, o, kernel_size=3, stride=stride, padding=1, bias=False)
    tv.ops, tv.models, models.resnet = ops, models, resnet
    for m in (tv, ops, models, resnet):
        sys.modules[m.__name__] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("gluefactory.models.extractors.aliked")


def nms_candidates(mod, score_map, radius, image_size):
    """DKD's candidate map (aliked.py:120-132) with the reference's own simple_nms."""
    nms = mod.simple_nms(score_map, radius).clone()
    B, _, H, W = nms.shape
    nms[:, :, :radius] = 0
    nms[:, :, :, :radius] = 0
    for b in range(B):
        w, h = (int(image_size[b][0]), int(image_size[b][1])) if image_size is not None else (W, H)
        nms[b, :, h - radius:] = 0
        nms[b, :, :, w - radius:] = 0
    return nms.reshape(B, -1)


def build(mod, conf, sd):
    real_hub = torch.hub.load_state_dict_from_url
    torch.hub.load_state_dict_from_url = lambda *a, **k: {n: torch.from_numpy(np.array(v)) for n, v in sd.items()}
    try:
        return mod.ALIKED(dict(conf)).eval()
    finally:
        torch.hub.load_state_dict_from_url = real_hub


def try_case(mod, name, spec, img_seed, w_seed):
    B, H, W, conf, isz, _, _ = spec
    conf = dict(conf)
    sd = aliked_state_dict(conf["model_name"], seed=w_seed)
    image = synthetic_images(B, 3, H, W, seed=img_seed)
    radius = 2
    if isz is not None:
        assert isz[-1] == [W, H], "the last image fills the tensor (aliked.py:127 rebinds w, h)"
    if conf["detection_threshold"] == "auto":
        probe = build(mod, dict(conf, detection_threshold=0.5), sd).double()
        with torch.no_grad():
            _, smap = probe.extract_dense_map(torch.from_numpy(image).double())
        v = torch.sort(nms_candidates(mod, smap, radius, isz)[0], descending=True).values
        v = v[v > 0]
        n = min(60, len(v) - 1)
        assert n >= 20, f"{name}: only {len(v)} candidates"
        conf["detection_threshold"] = round(float((v[n - 1] + v[n]) / 2), 4)
    data = {"image": torch.from_numpy(image)}
    data64 = {"image": torch.from_numpy(image).double()}
    if isz is not None:
        data["image_size"] = torch.tensor(isz, dtype=torch.float32)
        data64["image_size"] = torch.tensor(isz, dtype=torch.float64)
    model = build(mod, conf, sd)
    ref_keys = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    with torch.no_grad():
        pred = model(data)
        pred64 = build(mod, conf, sd).double()(data64)
    thr, k = float(conf["detection_threshold"]), int(conf["max_num_keypoints"])
    e = {"scores": float((pred["score_map"].double() - pred64["score_map"]).abs().max()), "kpts": 0.0, "desc": 0.0, "disp": 0.0}
    for b in range(B):
        try:
            idx = match_points(pred["keypoints"][b].numpy(), pred64["keypoints"][b].numpy())
        except AssertionError as err:
            return f"fp32 and fp64 keypoint sets differ ({err})"
        e["kpts"] = max(e["kpts"], float((pred["keypoints"][b].double() - pred64["keypoints"][b][idx]).abs().max()))
        e["desc"] = max(e["desc"], float((pred["descriptors"][b].double() - pred64["descriptors"][b][idx]).abs().max()))
        # the reference's swapped names: keypoint_scores is the dispersity, score_dispersity the sampled score
        e["disp"] = max(e["disp"], float((pred["keypoint_scores"][b].double() - pred64["keypoint_scores"][b][idx]).abs().max()))
        e["scores"] = max(e["scores"],
                          float((pred["score_dispersity"][b].double() - pred64["score_dispersity"][b][idx]).abs().max()))
    cand = nms_candidates(mod, pred64["score_map"], radius, isz)
    cand32 = nms_candidates(mod, pred["score_map"], radius, isz)
    gaps, positive, thr_gap, order = [], [], [], []
    for b in range(B):
        v = torch.sort(cand[b], descending=True).values
        positive.append(int((cand[b] > 0).sum()))
        if thr <= 0 and k > 0:
            gaps.append(float(v[k - 1] - v[k]))
            thr_gap.append(float("inf"))
            order.append(torch.sort(cand32[b], descending=True, stable=True).values[:k].numpy())
        else:
            gaps.append(float("inf"))
            thr_gap.append(float((cand[b][cand[b] > 0] - thr).abs().min()))
            order.append(cand32[b][cand32[b] > thr].numpy())
    bar = max(2e-6, 6 * e["scores"])
    n_kp = [len(p) for p in pred["keypoints"]]
    if min(gaps) <= 4 * bar or min(thr_gap) <= 4 * bar:
        return f"undecidable: kth_gap {gaps} thr_gap {thr_gap} bar {bar}"
    if thr <= 0 and min(positive) < k:
        return f"fewer than k positive candidates: {positive}"
    if e["desc"] >= 1e-5:
        return f"e_desc {e['desc']}: a position truncates differently in fp32 and fp64"
    if thr > 0 and not (20 <= min(n_kp) and max(n_kp) <= 200):
        return f"threshold mode keeps {n_kp} points"
    assert all(len(o) == n for o, n in zip(order, n_kp)), (name, [len(o) for o in order], n_kp)
    out = {f"out_{key}": np.stack([np.asarray(t) for t in v]) if not isinstance(v, torch.Tensor) else v.numpy()
           for key, v in pred.items()}
    out["out_order_scores"] = np.stack(order)
    meta = {"B": B, "H": H, "W": W, "conf": conf, "image_size": isz, "img_seed": img_seed, "w_seed": w_seed,
            "inputs_sha256": sha({"image": image}), "weights_sha256": sha(sd), "ref_state_dict": ref_keys,
            "e_scores": e["scores"], "e_kpts": e["kpts"], "e_desc": e["desc"], "e_disp": e["disp"], "kth_gap": gaps,
            "thr_gap": thr_gap, "positive": positive, "counts": n_kp, "match_tol": MATCH_TOL}
    out["meta_json"] = np.array(json.dumps(meta))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **out)
    print(name, {k_: v.shape for k_, v in out.items() if k_ != "meta_json"},
          {k_: meta[k_] for k_ in ("conf", "e_scores", "e_kpts", "e_desc", "e_disp", "kth_gap", "thr_gap", "positive", "counts")},
          "score map", float(pred["score_map"].min()), float(pred["score_map"].max()), float(pred["score_map"].std()))
    return None


def main():
    mod = install_shim()
    only = sys.argv[1:]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        for step in range(12):
            why = try_case(mod, name, spec, spec[5] + 100 * step, spec[6] + 100 * step)
            if why is None:
                break
            print(f"{name}: seeds +{100 * step} rejected: {why}")
        else:
            raise SystemExit(f"{name}: no decidable seeds")


if __name__ == "__main__":
    main()
