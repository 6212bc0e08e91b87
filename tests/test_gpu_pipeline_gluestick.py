"""GlueStick behind the two-view pipeline -- needs an MI355X.  A TwoViewPipeline without an
extractor takes each view's cached features (two_view_pipeline.py:62-97), hands the point and the
line keys through to the matcher resolved as "matchers.gluestick", and returns what the matcher
returns when called directly."""
import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
from gluestick_golden_util import load_case, model_data, recipe_inputs

pytestmark = pytest.mark.gpu

PER_VIEW = ("keypoints", "descriptors", "keypoint_scores", "lines", "lines_junc_idx", "line_scores")


def test_pipeline_equals_matcher():
    from lightglue_amd import GlueStick, pipeline

    z, meta = load_case("gs_l4_b2_m77_n131")
    recipe = meta["recipe"]
    sd, pair = recipe_inputs(recipe)
    sd_t = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    pipe = pipeline.get_model("two_view_pipeline")(
        {"matcher": {"name": "matchers.gluestick", **recipe["conf"]}, "allow_no_extract": True}).eval().cuda()
    assert isinstance(pipe.matcher, GlueStick) and not hasattr(pipe, "extractor")
    pipe.matcher.load_state_dict(sd_t, strict=True)
    direct = GlueStick(recipe["conf"]).eval().cuda()
    direct.load_state_dict(sd_t, strict=True)
    data = model_data(recipe, pair, "cuda")
    batch = {f"view{v}": {**data[f"view{v}"], "cache": {k: data[k + v] for k in PER_VIEW}} for v in "01"}
    with torch.no_grad():
        pred = pipe(batch)
        want = direct(data)
    for k in PER_VIEW:  # the cached features come back under the matcher's key names
        assert pred[k + "0"] is batch["view0"]["cache"][k] and pred[k + "1"] is batch["view1"]["cache"][k]
    for k, v in want.items():
        assert torch.equal(pred[k], v), k
    np.testing.assert_array_equal(pred["line_matches0"].cpu().numpy(), z["out_line_matches0"])
    assert int((pred["line_matches0"] >= 0).sum()) > 0 and int((pred["matches0"] >= 0).sum()) > 0
