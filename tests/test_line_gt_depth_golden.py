"""The torch-CPU restatement of the pose-and-depth line ground truth (tests/line_gt_depth_ref.py) against
the fixtures the reference produced (tests/golden/make_line_gt_depth_golden.py) -- no GPU needed.

The exact fixtures and every stage B bit for bit; stage A inside the recorded gating on the random ones
(it is the same fp32 arithmetic on the same machine class, so it is in fact equal, but only the gating is
asserted); the fixtures' own caps; the differences from the homography variant each on a small case."""
import numpy as np
import pytest
import torch

import line_gt_depth_ref as R
import line_gt_ref as LR

NAMES = R.fixture_names()


def _lines(g, dtype=torch.float32):
    return torch.from_numpy(g["lines0"]).to(dtype), torch.from_numpy(g["lines1"]).to(dtype)


def test_the_fixtures_are_the_ones_the_issue_names():
    assert NAMES == ["line_gtd_exact_b1_n48_n64", "line_gtd_exact_b3_n64_n48", "line_gtd_rand_b1_n128_n128_d4",
                     "line_gtd_rand_b2_n130_n96_d2", "line_gtd_rand_b2_n96_n130_d0", "line_gtd_rand_p7_b2_n96_n96"]
    for name in NAMES:
        g, meta = R.load_fixture(name)
        assert g["lines0"].shape == (meta["B"], meta["n0"], 4) and g["lines1"].shape == (meta["B"], meta["n1"], 4)
        assert g["camera0"].shape[1] == 6 + meta["n_dist"]
        assert meta["npts"] == (33 if meta["exact"] else 7 if "_p7_" in name else 50)
        ign = int(g["ignore_depth0"].sum() + g["ignore_depth1"].sum())
        out = int(g["out_of0"].sum() + g["out_of1"].sum())
        assert g["positive"].sum() >= 10 and ign >= 3 and out >= 3, (name, ign, out)
        if not meta["exact"]:
            for k, und in (("cnt0", "und0"), ("cnt1t", "und1t")):
                assert (g[und] > 0).sum() <= 0.03 * (g[k] > 0).sum(), (name, k)
            assert g["und_line0"].sum() + g["und_line1"].sum() <= 0.03 * meta["B"] * (meta["n0"] + meta["n1"]), name
            assert R.pair_decided(g, meta).sum() >= 1, name


@pytest.mark.parametrize("name", NAMES)
def test_stage_a_reproduces_the_fixture(name):
    g, meta = R.load_fixture(name)
    kw = R.call_kw(meta)
    a = R.stage_a(*_lines(g), R.feed_of(g, meta), kw["npts"], kw["dist_th"], kw["min_visibility_th"])
    R.check_stage_a({k: v.numpy() for k, v in a.items()}, g, meta)
    if meta["exact"]:  # every step exact: fp64 gives the same arrays
        a64 = R.stage_a(*_lines(g, torch.float64), R.feed_of(g, meta, torch.float64), kw["npts"], kw["dist_th"],
                        kw["min_visibility_th"])
        R.check_stage_a({k: v.numpy() for k, v in a64.items()}, g, meta)


@pytest.mark.parametrize("name", NAMES)
def test_stage_b_reproduces_the_fixture_bit_for_bit(name):
    g, meta = R.load_fixture(name)
    pos, m0, m1, cost, assignation = R.stage_b_of(g, g["valid_lines0"], g["valid_lines1"], meta["npts"], meta["overlap_th"])
    R.check_labels((pos.numpy(), m0.numpy(), m1.numpy()), g)
    np.testing.assert_array_equal(cost.numpy().astype(np.float64), g["cost"])
    np.testing.assert_array_equal(assignation.numpy(), g["assignation"])


@pytest.mark.parametrize("name", NAMES)
def test_the_full_function_reproduces_the_decided_pairs(name):
    g, meta = R.load_fixture(name)
    l0, l1 = _lines(g)
    got = R.gt_line_matches_from_pose_depth(l0, l1, torch.from_numpy(g["valid_lines0"]), torch.from_numpy(g["valid_lines1"]),
                                            R.feed_of(g, meta), **R.call_kw(meta))
    R.check_labels([t.numpy() for t in got], g, pairs=R.pair_decided(g, meta))


def _tiny(depth_hw=(40, 60), image_hw=None, B=1):
    h, w = depth_hw
    cam = torch.tensor([[float(w), float(h), 50.0, 50.0, w / 2, h / 2]]).repeat(B, 1)
    T = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]]).repeat(B, 1)
    view = lambda: {"camera": cam.clone(), "depth": torch.full((B, h, w), 3.0)}  # noqa: E731
    data = {"view0": view(), "view1": view(), "T_0to1": T, "T_1to0": T}
    if image_hw is not None:
        for v in ("view0", "view1"):
            data[v]["image"] = torch.zeros(B, 1, *image_hw)
    return data


def test_differences_from_the_homography_variant():
    # out_of is not part of mask_close: a line that is out still blocks through unmatched only
    cnt = torch.tensor([[[40, 0], [0, 40]]])
    f, t = torch.zeros(1, 2, dtype=torch.bool), torch.ones(1, 2, dtype=torch.bool)
    nv = torch.full((1, 2), 50)
    pos, m0, m1, _, _ = R.stage_b(cnt, cnt, f, f, f, f, nv, nv, t, t, 50, 0.2)
    assert pos[0, 0, 0] and pos[0, 1, 1] and m0.tolist() == [[0, 1]]
    out1 = torch.tensor([[True, False]])  # line 0 of image 0 leaves image 1
    pos, m0, m1, _, _ = R.stage_b(cnt, cnt, f, out1, f, f, nv, nv, t, t, 50, 0.2)
    assert not pos[0, 0].any() and m0.tolist() == [[-1, 1]] and m1.tolist() == [[-1, 1]]
    # a lower visible count lowers the line's threshold: 9 > 40 * 0.2 but not > 50 * 0.2
    cnt9 = torch.tensor([[[9]]])
    one, zero = torch.ones(1, 1, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)
    assert not R.stage_b(cnt9, cnt9, zero, zero, zero, zero, torch.tensor([[50]]), torch.tensor([[50]]), one, one)[0].any()
    assert R.stage_b(cnt9, cnt9, zero, zero, zero, zero, torch.tensor([[40]]), torch.tensor([[40]]), one, one)[0].all()
    # depth-ignored lines are ignored (-2), as invalid ones are
    assert R.stage_b(cnt9 * 5, cnt9 * 5, zero, zero, one, zero, nv[:, :1], nv[:, :1], one, one)[1].tolist() == [[-2]]
    # the empty side (:227-238): [B, n] of -1, not [B, 0]
    data = _tiny()
    pos, m0, m1 = R.gt_line_matches_from_pose_depth(torch.zeros(2, 0, 4), torch.zeros(2, 3, 4), torch.zeros(2, 0, dtype=torch.bool),
                                                    torch.ones(2, 3, dtype=torch.bool), data)
    assert tuple(pos.shape) == (2, 0, 3) and tuple(m0.shape) == (2, 0) and m1.tolist() == [[-1] * 3] * 2 and m1.dtype == torch.int64


def test_clamp_uses_the_depth_map_and_the_outside_test_the_image():
    lines = torch.tensor([[[10.0, 30.0, 58.0, 30.0], [5.0, 5.0, 100.0, 5.0]]])
    a = R.stage_a(lines, lines, _tiny(image_hw=(40, 30)), 50, 5, 0.5)  # the image is half as wide as the depth map
    assert a["out_of1"].tolist() == [[True, True]] and (a["num_visible0"] == 50).all()  # clamped to x <= 59, half of it past x = 30
    b = R.stage_a(lines, lines, _tiny(), 50, 5, 0.5)  # no image: the depth map's size
    assert b["out_of1"].tolist() == [[False, False]]
    assert torch.equal(b["cnt0"], R.stage_a(lines, lines, _tiny(image_hw=(40, 60)), 50, 5, 0.5)["cnt0"])
    # a sample on the first row mixes with the zero padding and stays valid; an all-zero map ignores every line
    top = torch.tensor([[[5.0, 0.0, 40.0, 0.0]]])
    assert not R.stage_a(top, top, _tiny(), 50, 5, 0.5)["ignore_depth0"].any()
    dark = _tiny()
    dark["view0"]["depth"].zero_()
    a = R.stage_a(top, top, dark, 50, 5, 0.5)
    assert a["ignore_depth0"].all() and not a["ignore_depth1"].any() and not a["out_of1"].any()  # NaN is not outside
    assert a["num_visible0"].sum() == 0 and a["cnt1t"].sum() == 0


def test_thresholds_restated():
    assert R.min_close_table(50, 0.2)[50] == LR.min_close_count(50, 0.2) == 11
    assert R.min_close_table(50, 0.2)[40] == 9 and R.min_close_table(50, 0.2)[0] == 1
    assert R.min_close_table(7, 1.0) == [1, 2, 3, 4, 5, 6, 7, 8]  # v = npts: no count qualifies
    assert R.min_valid_count(50, 0.5) == 25 and R.min_valid_count(7, 0.0) == 0 and R.min_valid_count(7, 1.0) == 7
