"""Shared inputs and oracle references of the ragged-batch tests (test_gpu_ragged.py,
test_ragged_host.py).

A ragged case is ``B`` pairs laid out at one capacity per image; pair ``b`` has ``counts[b] =
(n0, n1)`` real points, stored first.  Inputs and weights are ``homography_pairs`` /
``crafted_state_dict`` of test_gpu_hpatches_auc.py.  The reference of pair ``b`` is the CPU oracle
on that pair alone, sliced to its own counts -- one call per pair, computed once per process and
shared (never modified) by every test that needs it."""
import functools

import numpy as np
import torch

import lgamd  # noqa: F401
from test_gpu_hpatches_auc import crafted_state_dict, homography_pairs

CONF = {"filter_threshold": 0.1}

# name -> (capacity, per-pair (n0, n1), seed)
CASES = {
    # two 256-tiles per side, one partial; B not a multiple of 8 (the xcd_remap tile order)
    "b3": (320, ((320, 320), (257, 255), (17, 300)), 11),
    # B = 8: whole pairs per XCD
    "b8": (272, ((272, 272), (256, 272), (255, 17), (1, 40), (40, 1), (129, 130), (16, 16), (200, 271)), 12),
    # capacity not a multiple of 16: the unfused assignment
    "odd": (300, ((300, 299), (33, 7)), 11),
}

POINT_KEYS = ("keypoints0", "keypoints1", "descriptors0", "descriptors1")


@functools.lru_cache(maxsize=None)
def state_dict():
    return crafted_state_dict(CONF)


@functools.lru_cache(maxsize=None)
def case_data(name):
    cap, counts, seed = CASES[name]
    data, _ = homography_pairs(len(counts), cap, seed=seed)
    for v in data.values():
        v.setflags(write=False)
    return data


def pair_data(name, b, with_size=True):
    """Pair b of a case alone, at M = n0, N = n1 (numpy, batch of one)."""
    data = case_data(name)
    n0, n1 = CASES[name][1][b]
    out = {"keypoints0": data["keypoints0"][b:b + 1, :n0], "keypoints1": data["keypoints1"][b:b + 1, :n1],
           "descriptors0": data["descriptors0"][b:b + 1, :n0], "descriptors1": data["descriptors1"][b:b + 1, :n1]}
    if with_size:
        out["image_size0"] = data["image_size0"][b:b + 1]
        out["image_size1"] = data["image_size1"][b:b + 1]
    return {k: v.copy() for k, v in out.items()}  # the shared case data stays read-only


@functools.lru_cache(maxsize=None)
def oracle_pair(name, b, with_size=True):
    """The CPU oracle on pair b alone (default conf of the ragged tests)."""
    import oracle

    with torch.no_grad():
        ref = oracle.lightglue_forward(state_dict(), pair_data(name, b, with_size), CONF)
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in ref.items()}


def top2_margin(la):
    """Smallest top-1 / top-2 gap over the rows and the columns of a pair's real block (a
    direction with a single candidate has no runner-up and is left out)."""
    la = np.asarray(la, np.float64)
    gaps = []
    for axis in (1, 0):
        if la.shape[axis] < 2:
            continue
        s = np.sort(la, axis=axis)
        top = np.take(s, -1, axis=axis) - np.take(s, -2, axis=axis)
        gaps.append(float(top.min()))
    return min(gaps) if gaps else float("inf")


def feed(name, device, pad="zero", with_size=True, counts=True):
    """The case as a LightGlue input dict on ``device``; the padding rows of keypoints and
    descriptors are zero or NaN."""
    data = case_data(name)
    cap, cnts, _ = CASES[name]
    out = {}
    for k in POINT_KEYS:
        v = data[k].copy()
        side = int(k[-1])
        for b, c in enumerate(cnts):
            v[b, c[side]:] = 0.0 if pad == "zero" else np.nan
        out[k] = torch.from_numpy(v).to(device)
    if with_size:
        out["view0"] = {"image_size": torch.from_numpy(data["image_size0"].copy()).to(device)}
        out["view1"] = {"image_size": torch.from_numpy(data["image_size1"].copy()).to(device)}
    if counts:
        out["num_keypoints0"] = torch.tensor([c[0] for c in cnts], dtype=torch.int64)
        out["num_keypoints1"] = torch.tensor([c[1] for c in cnts], dtype=torch.int32, device=device)
    return out
