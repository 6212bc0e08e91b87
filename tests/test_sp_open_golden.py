"""The torch-CPU restatement of the open SuperPoint (tests/spo_ref.py) against the reference's own
outputs (tests/golden/sp_open/spo_*.npz, tests/golden/make_sp_open_golden.py): the GPU tests use the
restatement where no fixture exists, so it has to BE the reference."""
import numpy as np
import pytest

from spo_golden_util import assert_same_keypoints, sha_inputs, spo_bars, spo_case_inputs, spo_case_names, spo_load
from spo_ref import spo_forward


def test_three_fixtures_are_committed():
    assert len(spo_case_names()) == 3


@pytest.mark.parametrize("name", spo_case_names())
def test_restatement_reproduces_the_reference(name):
    g = spo_load(name)
    meta = g["meta"]
    conf, sd, data = spo_case_inputs(meta)
    assert sha_inputs({"image": data["image"]}) == meta["inputs_sha256"], "image recipe drifted"
    assert sha_inputs(sd) == meta["weights_sha256"], "weight recipe drifted"
    out = {k: v.numpy() for k, v in spo_forward(sd, data, conf).items()}
    # same torch, same arithmetic: within the reference's own fp32-vs-fp64 error (in practice equal)
    swaps = assert_same_keypoints(out, g["out_keypoints"], g["out_keypoint_scores"], g["out_descriptors"],
                                  max(meta["e_scores"], 1e-7), max(meta["e_desc"], 1e-7))
    assert swaps == 0
    np.testing.assert_array_equal(out["keypoints"], g["out_keypoints"])
    assert ("dense_descriptors" in out) == ("out_dense_descriptors" in g)
    if "out_dense_descriptors" in g:
        np.testing.assert_allclose(out["dense_descriptors"], g["out_dense_descriptors"], atol=max(meta["e_desc"], 1e-7), rtol=0)


@pytest.mark.parametrize("name", spo_case_names())
def test_fixture_is_decidable(name):
    """What make_sp_open_golden.py asserted when it wrote the fixture, re-read from the meta: the
    selection cannot be flipped by an error within the score bar."""
    meta = spo_load(name)["meta"]
    score_bar, _ = spo_bars(meta)
    assert min(meta["kth_gap"]) > 4 * score_bar
    assert min(meta["thr_gap"]) > 4 * score_bar
    conf = meta["conf"]
    if conf.get("detection_threshold", 0.005) < 0:  # no zero-score tie among the selected
        assert min(meta["positive"]) >= conf["max_num_keypoints"]
    assert len(meta["ref_state_dict_keys"]) == 84
