"""Wireframe golden fixtures (tests/golden/wireframe/*.npz): the recipe -> inputs, and the helpers the
CPU and GPU tests share.  The generator (tests/golden/make_wireframe_golden.py) builds its inputs
through the same functions.

A fixture stores only outputs of the reference: the fp64-run values, ``e_<key>`` = max |fp32 run -
fp64 run|, labels, counts, the removed-keypoint mask and the reference's random rows
(``fill_junctions`` / ``fill_keypoints``, read back from its outputs).  Of ``descriptors`` only the
sampled rows are stored (``desc_rows`` at ``desc_index`` = (image, row)); every other row is a copy
of the point extractor's descriptor."""
import glob
import json
import os

import numpy as np

import lgamd  # noqa: F401
from lightglue_amd.gs_weights import wireframe_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wireframe")
REF_ERR_FACTOR = 6.0  # the project's factor on a reference's own fp32-vs-fp64 deviation
WIDTH, HEIGHT, S = 160, 120, 8
ULP32 = float(np.finfo(np.float32).eps)
# magnitude each float output is floored at (2 ulp of it): coordinates at the image size, the rest at 1
MAGNITUDE = {"keypoints": float(WIDTH), "lines": float(WIDTH), "keypoint_scores": 1.0, "line_scores": 1.0,
             "descriptors": 1.0}
FLOAT_KEYS = tuple(MAGNITUDE)


def case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta_json"]))


def recipe_inputs(recipe):
    return wireframe_inputs(recipe["B"], tuple(recipe["lines"]), recipe["K"], seed=recipe["seed"],
                            max_num_lines=recipe["max_num_lines"], dim=recipe["dim"], nms_radius=recipe["nms_radius"],
                            width=WIDTH, height=HEIGHT, s=S)


def wf_conf(recipe):
    """The flat settings tests/wireframe_ref.py takes."""
    return {"nms_radius": recipe["nms_radius"], "merge_points": recipe["merge_points"],
            "merge_line_endpoints": recipe["merge_line_endpoints"], "force_num_keypoints": recipe["forced"],
            "force_num_lines": recipe["forced"], "max_num_lines": recipe["max_num_lines"]}


def extractor_conf(recipe, point_name, line_name):
    """The nested config of WireframeExtractor (reference and ours)."""
    return {"point_extractor": {"name": point_name, "force_num_keypoints": recipe["forced"], "max_num_keypoints": recipe["K"]},
            "line_extractor": {"name": line_name, "force_num_lines": recipe["forced"], "max_num_lines": recipe["max_num_lines"]},
            "wireframe_params": {"merge_points": recipe["merge_points"], "merge_line_endpoints": recipe["merge_line_endpoints"],
                                 "nms_radius": recipe["nms_radius"]}}


def bar(z, key):
    """REF_ERR_FACTOR x the reference's own fp32 error, floored at 2 ulp of the value's magnitude."""
    return max(REF_ERR_FACTOR * float(z["e_" + key]), 2 * ULP32 * MAGNITUDE[key])


def check_against_fixture(z, recipe, inp, got, exact_ints=True):
    """``got``: the extractor's outputs as numpy arrays ([B, ...]).  Returns {key: max abs deviation}."""
    dev = {}
    np.testing.assert_array_equal(got["lines_junc_idx"], z["out_lines_junc_idx"])
    np.testing.assert_array_equal(np.asarray(got["num_junctions"]).ravel(), z["out_num_junctions"].ravel())
    np.testing.assert_array_equal(got["pl_associativity"], z["out_pl_associativity"])
    for k in ("keypoints", "keypoint_scores", "lines", "line_scores"):
        assert got[k].shape == z["out_" + k].shape, (k, got[k].shape, z["out_" + k].shape)
        dev[k] = float(np.abs(got[k].astype(np.float64) - z["out_" + k]).max()) if got[k].size else 0.0
        assert dev[k] <= bar(z, k), (k, dev[k], bar(z, k))
    np.testing.assert_array_equal(got["orig_lines"], inp["lines"])
    # descriptors: the sampled rows against the fixture, every other row a copy of the input row
    B, N, D = got["descriptors"].shape
    sampled = np.zeros((B, N), bool)
    idx = z["desc_index"]
    sampled[idx[:, 0], idx[:, 1]] = True
    rows = got["descriptors"][idx[:, 0], idx[:, 1]].astype(np.float64)
    dev["descriptors"] = float(np.abs(rows - z["desc_rows"]).max()) if rows.size else 0.0
    assert dev["descriptors"] <= bar(z, "descriptors"), (dev["descriptors"], bar(z, "descriptors"))
    removed = z["removed"].astype(bool)
    for b in range(B):
        src = inp["descriptors"][b] if recipe["forced"] or not recipe["merge_points"] else inp["descriptors"][b][~removed[b]]
        J = N - len(src)
        keep = ~sampled[b, J:]
        np.testing.assert_array_equal(got["descriptors"][b, J:][keep], src[keep])
    return dev
