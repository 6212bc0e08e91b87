"""Pin the SuperPoint oracle (oracle/superpoint_ref.py) to the reference's own outputs
(tests/golden/sp_*.npz, made by tests/golden/make_superpoint_golden.py from the reference's
gluefactory_nonfree/superpoint.py).

The oracle is the same torch-CPU fp32 program as the reference, but torch's CPU convolution sums in
an order that depends on the host (instruction set, thread count), so its floats are reproducible
only up to fp32 summation order -- not bit for bit on every machine.  Bars, from the fixtures' own
fp32 error and the number format, not from the oracle's results:

* scores: the reference's own fp32 scores lie within 1.3e-7 of its float64 run (scores span
  7e-4 .. 0.15; tests/test_gpu_superpoint.py); two fp32 runs that differ only in summation order
  are each that far from float64, so they are held to SCORE_ATOL = 4 x 1.3e-7 = 5.2e-7 absolute
  (a quarter of the GPU path's 2e-6 bar).
* keypoints: integer pixels chosen by exact comparisons -- the same SET, compared exactly (every
  committed case has a top-k boundary gap, kth_gap, above 1e-6 > SCORE_ATOL); inside the sorted
  top-k only keypoints whose reference scores are closer than 2 x SCORE_ATOL may trade places.
  Refined (sub-pixel) keypoints are score-weighted means of pixel coordinates: within 4 ulp of the
  largest coordinate, 4 x 2^-23 x max(H, W) pixels.
* descriptors: 1e-6 (unit vectors), as before.
"""
import numpy as np
import pytest
import torch

from oracle.superpoint_ref import superpoint_forward
from sp_golden_util import sha, sp_case_inputs, sp_case_names, sp_load

SCORE_ATOL = 4 * 1.3e-7
DESC_ATOL = 1e-6


def assert_same_keypoints(out, ref_k, ref_s, ref_d, kp_atol):
    """Same keypoint set per image (exact pixels, or within kp_atol when refined), scores
    positionally within SCORE_ATOL, descriptors per keypoint within DESC_ATOL; a keypoint may sit
    at another position of the sorted order only if the reference scores of the two positions are
    closer than 2 x SCORE_ATOL."""
    ok, os_, od = out["keypoints"].numpy(), out["keypoint_scores"].numpy(), out["descriptors"].numpy()
    assert ok.shape == ref_k.shape
    np.testing.assert_allclose(os_, ref_s, atol=SCORE_ATOL, rtol=0)
    for b in range(ok.shape[0]):
        dist = np.abs(ok[b][:, None, :] - ref_k[b][None, :, :]).max(-1)
        idx = np.argmin(dist, axis=1)
        assert (dist[np.arange(len(idx)), idx] <= kp_atol).all(), "different keypoints"
        assert sorted(idx.tolist()) == list(range(len(idx))), "different keypoint sets"
        moved = idx != np.arange(len(idx))
        assert (np.abs(ref_s[b][idx[moved]] - ref_s[b][moved]) < 2 * SCORE_ATOL).all(), "order differs beyond near-ties"
        np.testing.assert_allclose(od[b], ref_d[b][idx], atol=DESC_ATOL, rtol=0)


@pytest.mark.parametrize("name", sp_case_names())
def test_superpoint_oracle_matches_reference(name):
    g = sp_load(name)
    meta = g["meta"]
    conf, sd, data = sp_case_inputs(meta)
    assert sha({"image": data["image"]}) == meta["inputs_sha256"], "image recipe drifted"
    assert sha(sd) == meta["weights_sha256"], "weight recipe drifted"
    conf = {k: v for k, v in conf.items() if k != "force_num_keypoints"}
    with torch.no_grad():
        out = superpoint_forward(sd, data, conf)
    if conf.get("sparse_outputs", True):
        assert min(meta["kth_gap"]) > 1e-6
        refined = conf.get("refinement_radius", 0) > 0
        kp_atol = 4 * 2.0 ** -23 * max(meta["H"], meta["W"]) if refined else 0.0
        assert_same_keypoints(out, g["out_keypoints"], g["out_keypoint_scores"], g["out_descriptors"], kp_atol)
    else:
        np.testing.assert_allclose(out["keypoint_scores"].numpy(), g["out_keypoint_scores"], atol=SCORE_ATOL, rtol=0)
        np.testing.assert_allclose(out["descriptors"].numpy(), g["out_descriptors"], atol=DESC_ATOL, rtol=0)
