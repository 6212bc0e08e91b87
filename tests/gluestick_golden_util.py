"""GlueStick golden fixtures (tests/golden/gluestick/*.npz): the recipe -> inputs and weights, and
the comparison helpers the CPU and GPU tests share.  The generator
(tests/golden/make_gluestick_golden.py) builds its inputs through the same functions."""
import glob
import json
import os

import numpy as np
import torch

import lgamd  # noqa: F401
from lightglue_amd.gs_weights import gluestick_state_dict, wireframe_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gluestick")
REF_ERR_FACTOR = 6.0   # the project's factor on a reference's own fp32-vs-fp64 deviation
BAND = 1e-4            # decisions closer than this to a tie / the threshold may flip
FLOAT_KEYS = ("log_assignment", "matching_scores0", "matching_scores1", "line_log_assignment", "line_matching_scores0",
              "line_matching_scores1", "raw_line_scores", "gnn_descriptors0", "gnn_descriptors1")
MATCH_KEYS = ("matches0", "matches1", "line_matches0", "line_matches1")
INPUT_KEYS = ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "keypoint_scores0", "keypoint_scores1",
              "lines0", "lines1", "lines_junc_idx0", "lines_junc_idx1", "line_scores0", "line_scores1")
GT_KEYS = ("gt_matches0", "gt_matches1", "gt_assignment", "gt_line_matches0", "gt_line_matches1", "gt_line_assignment")


def case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta_json"]))


def recipe_inputs(recipe):
    """(weights state dict, wireframe pair incl. ground truth) of a recipe, as numpy arrays."""
    sd = gluestick_state_dict(recipe["conf"], seed=recipe["w_seed"], proj_gain=recipe["proj_gain"],
                              line_gain=recipe["line_gain"])
    pair = wireframe_pair(recipe["B"], recipe["junc"], recipe["pts"], recipe["lines"], seed=recipe["seed"],
                          pad_junc=recipe["pad_junc"], noise=recipe["noise"], width=recipe["image_wh"][0],
                          height=recipe["image_wh"][1])
    return sd, pair


def image_sizes(recipe):
    """[B, 2] (w, h) per view, or None when the case passes the image shape only."""
    if not recipe["image_size"]:
        return None
    return np.tile(np.asarray([recipe["image_wh"]], np.float32), (recipe["B"], 1))


def ref_data(recipe, pair):
    """The data dict of tests/gluestick_ref.gluestick_forward."""
    d = {k: pair[k] for k in INPUT_KEYS}
    isz = image_sizes(recipe)
    d["image_size0"] = d["image_size1"] = isz
    d["image_hw"] = (recipe["image_wh"][1], recipe["image_wh"][0])
    return d


def model_data(recipe, pair, device):
    """The data dict of the matcher modules (torch tensors on ``device``), ground truth included."""
    d = {k: torch.from_numpy(np.ascontiguousarray(pair[k])).to(device) for k in INPUT_KEYS + GT_KEYS}
    isz = image_sizes(recipe)
    w, h = recipe["image_wh"]
    for v in "01":
        view = {"image": torch.zeros(recipe["B"], 1, h, w, device=device)}
        if isz is not None:
            view["image_size"] = torch.from_numpy(isz).to(device)
        d["view" + v] = view
    return d


def margins(la, th):
    """Per row / column of la[:, :-1, :-1]: best minus second best, and |exp(best) - th|."""
    s = np.asarray(la)[:, :-1, :-1].astype(np.float64)
    r = np.sort(s, axis=2)
    c = np.sort(s, axis=1)
    gap_r = r[:, :, -1] - r[:, :, -2] if s.shape[2] > 1 else np.full(s.shape[:2], np.inf)
    gap_c = c[:, -1, :] - c[:, -2, :] if s.shape[1] > 1 else np.full((s.shape[0], s.shape[2]), np.inf)
    return {"row_gap": gap_r, "col_gap": gap_c, "row_th": np.abs(np.exp(r[:, :, -1]) - th),
            "col_th": np.abs(np.exp(c[:, -1, :]) - th)}


def decided(la, th, band=BAND, mg=None):
    """Masks of the rows / columns of a reference log assignment whose match decision cannot flip
    within ``band``: their own argmax and threshold margins exceed it, and so do those of the
    best column (row) whose argmax the mutual check reads.  ``mg``: a fixture's stored margins
    (default: computed from ``la``)."""
    mg = margins(la, th) if mg is None else mg
    s = np.asarray(la)[:, :-1, :-1]
    ok_r = (mg["row_gap"] > band) & (mg["row_th"] > band)
    ok_c = (mg["col_gap"] > band) & (mg["col_th"] > band)
    part_r = np.take_along_axis(ok_c, s.argmax(2), 1)
    part_c = np.take_along_axis(ok_r, s.argmax(1), 1)
    return ok_r & part_r, ok_c & part_c


def compare_matches(got, ref, mask, what):
    """Matches equal on ``mask``; returns the number of entries outside it."""
    got, ref = np.asarray(got), np.asarray(ref)
    bad = (got != ref) & mask
    assert not bad.any(), f"{what}: {int(bad.sum())} decided entries differ, first at {np.argwhere(bad)[0]}"
    return int((~mask).sum())
