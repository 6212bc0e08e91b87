"""The line ground-truth fixtures the reference produced (tests/golden/make_line_gt_golden.py) against
the torch-CPU restatement and the NumPy port of SciPy's solver (tests/line_gt_ref.py) -- no GPU needed.

Bars: the exact fixtures bit for bit; the random fixtures' counts equal on decided entries and inside
the recorded bounds elsewhere; the labels from the fixture's own counts equal with no gating; the solver
port equal to the recorded ``assignation`` on every recorded cost matrix, and to SciPy where it imports;
the generator's caps re-read from the files."""
import numpy as np
import pytest
import torch

import line_gt_ref as R

NAMES = R.fixture_names()


def _t(g, *keys):
    return [torch.from_numpy(g[k]) for k in keys]


def test_all_fixtures_are_present():
    assert len(NAMES) == 8
    assert sum(R.load_fixture(n)[1]["exact"] for n in NAMES) == 2
    shapes = {(m["B"], m["n0"], m["n1"]) for m in (R.load_fixture(n)[1] for n in NAMES)}
    assert {(3, 64, 48), (1, 48, 64), (2, 128, 128), (2, 96, 130), (2, 130, 96), (1, 300, 257), (2, 250, 250)} <= shapes
    assert any(m["npts"] == 7 and m["overlap_th"] == 0.5 for m in (R.load_fixture(n)[1] for n in NAMES))


@pytest.mark.parametrize("name", NAMES)
def test_restated_counts_match_the_fixture(name):
    g, meta = R.load_fixture(name)
    l0, l1, H = _t(g, "lines0", "lines1", "H_0to1")
    cnt0, cnt1t, o0, o1 = R.stage_a(l0, l1, meta["shape"], meta["shape"], H, meta["npts"], meta["dist_th"],
                                    meta["min_visibility_th"])
    R.check_counts({"cnt0": cnt0.numpy(), "cnt1t": cnt1t.numpy(), "out_of0": o0.numpy(), "out_of1": o1.numpy()}, g, meta)


@pytest.mark.parametrize("name", NAMES)
def test_restated_labels_from_the_fixture_counts(name):
    g, meta = R.load_fixture(name)
    pos, m0, m1, cost, assignation = R.stage_b(*_t(g, "cnt0", "cnt1t", "out_of0", "out_of1", "valid_lines0", "valid_lines1"),
                                               meta["npts"], meta["overlap_th"])
    R.check_labels((pos.numpy(), m0.numpy(), m1.numpy()), g)
    np.testing.assert_array_equal(cost.numpy().astype(np.float64), g["cost"])
    np.testing.assert_array_equal(assignation.numpy(), g["assignation"])


@pytest.mark.parametrize("name", [n for n in NAMES if R.load_fixture(n)[1]["exact"]])
def test_restated_end_to_end_on_the_exact_fixtures(name):
    g, meta = R.load_fixture(name)
    for dtype in (torch.float32, torch.float64):
        l0, l1, H = (x.to(dtype) for x in _t(g, "lines0", "lines1", "H_0to1"))
        got = R.gt_line_matches_from_homography(l0, l1, *_t(g, "valid_lines0", "valid_lines1"), meta["shape"], meta["shape"],
                                                H, meta["npts"], meta["dist_th"], meta["overlap_th"],
                                                meta["min_visibility_th"])
        R.check_labels([x.numpy() for x in got], g)


@pytest.mark.parametrize("name", NAMES)
def test_solver_port_equals_the_recorded_assignation(name):
    g, meta = R.load_fixture(name)
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        linear_sum_assignment = None
    for b in range(meta["B"]):
        rows, cols = R.lsap(g["cost"][b])
        np.testing.assert_array_equal(np.stack([rows, cols]), g["assignation"][b])
        if linear_sum_assignment is not None:
            np.testing.assert_array_equal(np.stack(linear_sum_assignment(g["cost"][b])), g["assignation"][b])


def test_solver_port_on_small_and_tied_matrices():
    scipy_optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.Generator(np.random.PCG64(5))
    for shape in ((1, 1), (1, 5), (5, 1), (64, 64), (65, 63), (8, 2400)):
        for C in (np.zeros(shape), rng.integers(-3, 1, shape).astype(np.float64), rng.random(shape)):
            np.testing.assert_array_equal(np.stack(R.lsap(C)), np.stack(scipy_optimize.linear_sum_assignment(C)))


@pytest.mark.parametrize("name", [n for n in NAMES if not R.load_fixture(n)[1]["exact"]])
def test_caps_hold_in_the_files(name):
    g, meta = R.load_fixture(name)
    for cnt, und, lo in (("cnt0", "und0", "lo0"), ("cnt1t", "und1t", "lo1t")):
        share = (g[und] > 0).sum() / max((g[cnt] > 0).sum(), 1)
        assert share <= 0.03, (cnt, share)
        low = g[lo].astype(int)
        assert ((g[cnt] >= low) & (g[cnt] <= low + g[und])).all()
    und_flags = g["und_out_of0"].sum() + g["und_out_of1"].sum()
    assert und_flags / (meta["B"] * (meta["n0"] + meta["n1"])) <= 0.03
    assert (g["cnt0"] > 0).sum() > 50 and g["positive"].any()
