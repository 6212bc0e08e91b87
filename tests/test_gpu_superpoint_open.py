"""The open SuperPoint on the GPU (lightglue_amd.SuperPointOpen -> sp_open_create / sp_forward of
liblightglue_mi355x.so) against the reference's own outputs (tests/golden/sp_open/spo_*.npz,
tests/golden/make_sp_open_golden.py) and against the CPU restatement (tests/spo_ref.py, held to the
same fixtures by tests/test_sp_open_golden.py) on further seeded cases.

Bars (tests/spo_golden_util.py): scores max(2e-6, 6 e_scores), descriptors max(2e-5, 6 e_desc) per
case, where e_* is the reference's own fp32-vs-fp64 error of that case (stored in the fixture; from
a float64 run of the restatement for the seeded cases).  2e-6 / 2e-5 are the nonfree extractor's
bars (the same fp16x3 arithmetic), 6 the GPU-vs-reference over reference-vs-fp64 ratio measured
there, rounded up.  Keypoints are integer pixels chosen by exact comparisons: the SET is asserted
identical (every case has its top-k and threshold gaps above 4x the score bar); inside the sorted
top-k, keypoints whose scores differ by less than the bar may trade places.  Each test prints its
measured maxima before it asserts (DESIGN.md §9b records them).
"""
import numpy as np
import pytest
import torch

from lightglue_amd.sp_weights import SPO_POOLED, superpoint_open_state_dict, synthetic_images
from spo_golden_util import DESC_FLOOR, assert_same_keypoints, spo_bars, spo_case_inputs, spo_case_names, spo_load
from spo_ref import DEFAULT_CONF, candidate_map, dense_maps, reference_with_margins, sample_descriptors, spo_forward

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def as_torch_sd(sd):
    return {k: torch.from_numpy(v.copy()) if v.ndim else torch.tensor(int(v)) for k, v in sd.items()}


def make_model(conf, sd):
    from lightglue_amd import SuperPointOpen

    m = SuperPointOpen(conf).eval().to(DEV)
    m.load_state_dict(as_torch_sd(sd), strict=True)
    return m


def run(m, data, **extra):
    d = {"image": torch.from_numpy(data["image"]).to(DEV), **extra}
    with torch.no_grad():
        out = m(d)
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}


def check_fixture(name):
    g = spo_load(name)
    meta = g["meta"]
    conf, sd, data = spo_case_inputs(meta)
    score_bar, desc_bar = spo_bars(meta)
    assert min(meta["kth_gap"]) > 4 * score_bar and min(meta["thr_gap"]) > 4 * score_bar
    out = run(make_model(conf, sd), data)
    print(name, end=": ")
    assert_same_keypoints(out, g["out_keypoints"], g["out_keypoint_scores"], g["out_descriptors"], score_bar, desc_bar)
    assert ("dense_descriptors" in out) == ("out_dense_descriptors" in g)
    if "out_dense_descriptors" in g:
        err = float(np.abs(out["dense_descriptors"].numpy() - g["out_dense_descriptors"]).max())
        print(f"{name}: max dense descriptor error {err:.3g} (bar {desc_bar:.3g})")
        assert out["dense_descriptors"].shape == g["out_dense_descriptors"].shape and err <= desc_bar


@pytest.mark.parametrize("name", spo_case_names())
def test_open_superpoint_matches_reference_golden(name):
    check_fixture(name)


def test_open_superpoint_gather_convolution_matches_reference(monkeypatch):
    """The per-tap gather convolution (LG_SP_CONV=gather) with the affine epilogue, same golden."""
    monkeypatch.setenv("LG_SP_CONV", "gather")
    check_fixture("spo_gray_b1_100x132_k150")


def seeded(B, C, H, W, seed, gamma_sign=None):
    """Recipe weights and images; gamma_sign -1: every gamma of the three pooled blocks negative (a
    max-only pool is then wrong at every pooled value); +1: every gamma of every block positive."""
    sd = superpoint_open_state_dict(seed=seed)
    for k in list(sd):
        if k.endswith("bn.weight"):
            if gamma_sign == -1 and k[:-len(".bn.weight")] in SPO_POOLED:
                sd[k] = -np.abs(sd[k])
            if gamma_sign == 1:
                sd[k] = np.abs(sd[k])
    return sd, {"image": synthetic_images(B, C, H, W, seed=100 + seed)}


@pytest.mark.parametrize(
    "B,C,H,W,conf,seed,gamma_sign",
    [
        (1, 1, 72, 88, {"max_num_keypoints": 50}, 31, -1),                          # pooled gammas all negative
        (1, 3, 83, 97, {"max_num_keypoints": 50}, 32, 1),                           # all positive; odd sizes, RGB
        (1, 1, 72, 88, {"max_num_keypoints": None, "remove_borders": 0}, 33, None),  # every keypoint, no borders
        (2, 1, 40, 56, {"max_num_keypoints": 20, "nms_radius": 0, "remove_borders": 2}, 34, None),  # B > 1 stacked
    ],
)
def test_open_superpoint_matches_restatement(B, C, H, W, conf, seed, gamma_sign):
    sd, data = seeded(B, C, H, W, seed, gamma_sign)
    ref, meta = reference_with_margins(sd, data, conf)
    score_bar, desc_bar = spo_bars(meta)
    assert min(meta["kth_gap"]) > 4 * score_bar and min(meta["thr_gap"]) > 4 * score_bar, meta
    out = run(make_model(conf, sd), data)
    assert_same_keypoints(out, ref["keypoints"].numpy(), ref["keypoint_scores"].numpy(), ref["descriptors"].numpy(),
                          score_bar, desc_bar)


def test_open_superpoint_negative_threshold_with_more_slots_than_positive_candidates():
    """detection_threshold -1 makes every NMS-suppressed pixel a candidate of score 0; with k above
    the number of positive candidates torch.topk leaves the choice among those ties open.  Asserted:
    every positive keypoint comes first, in score order; the rest have score 0 at non-border pixels."""
    conf = {"max_num_keypoints": 400, "detection_threshold": -1, "nms_radius": 3}
    sd, data = seeded(1, 1, 72, 88, 35)
    pos, meta = reference_with_margins(sd, data, dict(conf, max_num_keypoints=None, detection_threshold=0.0))
    score_bar, desc_bar = spo_bars(meta)
    P = pos["keypoints"].shape[1]
    assert 0 < P < 400
    out = run(make_model(conf, sd), data)
    assert out["keypoints"].shape == (1, 400, 2) and out["descriptors"].shape == (1, 400, 256)
    s = out["keypoint_scores"][0]
    assert (s[:-1] >= s[1:]).all() and (s[:P] > 0).all() and (s[P:] == 0).all()
    order = torch.argsort(pos["keypoint_scores"][0], descending=True, stable=True)
    head = {k: v[:, :P] for k, v in out.items()}
    assert_same_keypoints(head, pos["keypoints"][:, order].numpy(), pos["keypoint_scores"][:, order].numpy(),
                          pos["descriptors"][:, order].numpy(), score_bar, desc_bar)
    rest = out["keypoints"][0, P:] - 0.5
    assert (rest[:, 0] >= 4).all() and (rest[:, 0] < 88 - 4).all() and (rest[:, 1] >= 4).all() and (rest[:, 1] < 72 - 4).all()
    assert len({tuple(p) for p in out["keypoints"][0].tolist()}) == 400
    d = sample_descriptors(out["keypoints"][:, P:] - 0.5, dense_maps(sd, torch.from_numpy(data["image"]))[1])[0].T
    np.testing.assert_allclose(out["descriptors"][0, P:].numpy(), d.numpy(), atol=desc_bar, rtol=0)


def test_open_superpoint_force_num_keypoints_pads_like_the_reference():
    """pad_and_stack(mode="random_c"): real keypoints first, pads uniform within the per-axis
    [min, max] of the real ones, zero scores, descriptors sampled at the pads."""
    conf = {"max_num_keypoints": 400, "force_num_keypoints": True}
    sd, data = seeded(2, 1, 64, 80, 36)
    scores, dense = dense_maps(sd, torch.from_numpy(data["image"]))
    cand = candidate_map(scores.clone(), DEFAULT_CONF)
    counts = [int((cand[b] > 0.005).sum()) for b in range(2)]
    assert 0 < min(counts) and max(counts) < 400
    out = run(make_model(conf, sd), data)
    assert out["keypoints"].shape == (2, 400, 2) and out["descriptors"].shape == (2, 400, 256)
    for b in range(2):
        n = counts[b]
        real = out["keypoints"][b, :n] - 0.5
        pads = out["keypoints"][b, n:] - 0.5
        assert (out["keypoint_scores"][b, :n] > 0.005).all() and (out["keypoint_scores"][b, n:] == 0).all()
        assert (pads >= real.min(0).values).all() and (pads <= real.max(0).values).all()
        d = sample_descriptors(out["keypoints"][b:b + 1] - 0.5, dense[b:b + 1])[0].T
        np.testing.assert_allclose(out["descriptors"][b].numpy(), d.numpy(), atol=DESC_FLOOR, rtol=0)


def test_open_superpoint_unequal_counts_raise_or_come_back_ragged():
    conf = {"max_num_keypoints": None}
    sd, data = seeded(2, 1, 64, 80, 36)
    m = make_model(conf, sd)
    with pytest.raises(RuntimeError, match="equal size"):
        run(m, data)
    out = run(m, data, ragged_keypoints=True)
    n = out["num_keypoints"].tolist()
    assert n[0] != n[1] and out["keypoints"].shape == (2, max(n), 2)
    ref = spo_forward(sd, {"image": data["image"][:1]}, conf)
    np.testing.assert_array_equal(out["keypoints"][0, :n[0]].numpy(), ref["keypoints"][0].numpy())
    b = int(np.argmin(n))
    assert (out["keypoint_scores"][b, n[b]:] == 0).all() and (out["descriptors"][b, n[b]:] == 0).all()


@pytest.mark.parametrize("matcher", [{"name": "matchers.lightglue", "filter_threshold": 0.1},
                                     {"name": "matchers.nearest_neighbor_matcher"}])
def test_open_superpoint_feeds_the_matchers_through_the_pipeline(matcher):
    """TwoViewPipeline(extractor=superpoint_open, matcher=...): the superpoint-open+* configs' shape --
    the extractor's outputs are the matcher's inputs, all on the device."""
    from lightglue_amd.pipeline import TwoViewPipeline
    from lightglue_amd.weights import synthetic_state_dict

    conf = {"extractor": {"name": "extractors.superpoint_open", "max_num_keypoints": 128, "detection_threshold": -1,
                          "nms_radius": 3, "force_num_keypoints": True},
            "matcher": matcher}
    pipe = TwoViewPipeline(conf).eval().to(DEV)
    pipe.extractor.load_state_dict(as_torch_sd(superpoint_open_state_dict(seed=2)), strict=True)
    if matcher["name"] == "matchers.lightglue":
        pipe.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict({}, seed=0).items()})
    img = torch.from_numpy(synthetic_images(2, 1, 96, 128, seed=4)).to(DEV)
    view0 = {"image": img[:1], "image_size": torch.tensor([[128.0, 96.0]], device=DEV)}
    view1 = {"image": img[1:], "image_size": torch.tensor([[128.0, 96.0]], device=DEV)}
    with torch.no_grad():
        pred = pipe({"view0": view0, "view1": view1})
        direct = pipe.matcher({"keypoints0": pred["keypoints0"], "keypoints1": pred["keypoints1"],
                               "descriptors0": pred["descriptors0"], "descriptors1": pred["descriptors1"],
                               "view0": view0, "view1": view1})
    assert pred["keypoints0"].shape == (1, 128, 2) and pred["descriptors1"].shape == (1, 128, 256)
    assert pred["keypoint_scores0"].shape == (1, 128) and pred["matches0"].shape == (1, 128)
    assert not torch.equal(pred["keypoints0"], pred["keypoints1"])
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        torch.testing.assert_close(pred[k], direct[k], rtol=0, atol=0)
