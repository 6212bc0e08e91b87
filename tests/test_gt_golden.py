"""tests/gt_ref.py (the torch-CPU restatement of gt_matches_from_homography) in fp32 against the
fixtures the reference itself produced (tests/golden/make_gt_golden.py): bit for bit on the exact
case, on every decidable item under the recorded near-tie gating on the others."""
import numpy as np
import pytest
import torch

import gt_ref


def test_fixtures_present():
    names = gt_ref.fixture_names()
    assert "gt_exact_b3_m64_n48" in names and len(names) >= 6


@pytest.mark.parametrize("name", gt_ref.fixture_names())
def test_restatement_matches_reference(name):
    g, meta = gt_ref.load_fixture(name)
    out = gt_ref.gt_matches_from_homography(torch.from_numpy(g["keypoints0"]), torch.from_numpy(g["keypoints1"]),
                                            torch.from_numpy(g["H_0to1"]), pos_th=meta["th_positive"],
                                            neg_th=meta["th_negative"])
    got = {k: v.numpy() for k, v in out.items()}
    assert got["assignment"].dtype == bool and got["matches0"].dtype == np.int64
    gt_ref.check_against_fixture(got, g, meta)


def test_fixture_gating_is_within_its_caps():
    """What the generator asserted, re-read from the files: undecidable rows + columns <= 3 %,
    undecidable reward entries <= 0.1 %, none at all in the exact case."""
    for name in gt_ref.fixture_names():
        g, meta = gt_ref.load_fixture(name)
        nrc = g["und_rows"].sum() + g["und_cols"].sum()
        if meta["exact"]:
            assert nrc == 0 and g["und_reward"].sum() == 0
            continue
        assert nrc <= 0.03 * (g["und_rows"].size + g["und_cols"].size), name
        assert g["und_reward"].sum() <= 0.001 * g["und_reward"].size, name
        assert meta["tau"] == 4.0 * meta["e"] and meta["proj_tol"] == 4.0 * meta["proj_err"]


def test_empty_side_returns_the_reference_tuple():
    a, m0, m1 = gt_ref.gt_matches_from_homography(torch.zeros(2, 0, 2), torch.zeros(2, 5, 2), torch.eye(3))
    assert a.shape == (2, 0, 5) and m0.shape == (2, 0) and (m1 == -1).all()
