"""The torch-CPU restatement of the pose-and-depth ground truth (tests/gt_depth_ref.py) against the
fixtures the reference itself produced (tests/golden/make_gt_depth_golden.py) -- no GPU needed.

The exact fixture bit for bit in all twelve outputs, NaN positions included, in fp32 and (cast) in
fp64; the random fixtures on every item the recorded margins decide, the continuous outputs within
the recorded tolerances.  (On the generating host the restatement gives the reference's bits in
every case -- the generator asserts it; another CPU's torch may round an fp32 matmul differently,
which is what the margins are for.)"""
import functools

import numpy as np
import pytest
import torch

import gt_depth_ref as R

NAMES = R.fixture_names()


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return R.load_fixture(name)


def _cases():
    return [(n, i) for n in NAMES for i in range(len(_fixture(n)[1]["variants"]))]


def _run(name, i, dtype):
    g, meta = _fixture(name)
    v = meta["variants"][i]
    d = R.feed_of(g, dtype)
    out = R.gt_matches_from_pose_depth(d["keypoints0"], d["keypoints1"], d, v["th_positive"], v["th_negative"], v["th_epi"],
                                       v["th_consistency"], **R.precomputed_kw(g, meta, dtype))
    return out, g, meta, v


def test_the_fixture_set_is_complete():
    assert len(NAMES) == 8 and "gtd_exact_b3_m64_n48" in NAMES
    flavours = {n: [v["prefix"] for v in _fixture(n)[1]["variants"]] for n in NAMES}
    assert flavours["gtd_exact_b3_m64_n48"] == ["plain_", "cc_", "ccepi_"]
    for nd in (0, 2, 4):
        g, meta = _fixture(f"gtd_rand_nd{nd}_b2_m300_n257")
        assert g["camera0"].shape == (2, 6 + nd) and flavours[f"gtd_rand_nd{nd}_b2_m300_n257"] == ["plain_", "cc_", "ccepi_"]
    assert _fixture("gtd_pre_b2_m128_n128")[1]["precomputed"] and "depth0" not in _fixture("gtd_pre_b2_m128_n128")[0]


@pytest.mark.parametrize("name,i", _cases())
def test_restatement_fp32_matches_the_reference_fixture(name, i):
    out, g, meta, v = _run(name, i, torch.float32)
    assert list(out) == R.KEYS
    assert out["assignment"].dtype == torch.bool and out["visible0"].dtype == torch.bool
    assert out["matches0"].dtype == torch.int64 and out["reward"].dtype == torch.float32
    R.check_against_fixture({k: t.numpy() for k, t in out.items()}, g, meta, v)


@pytest.mark.parametrize("name,i", _cases())
def test_restatement_fp64_matches_the_reference_fixture(name, i):
    out, g, meta, v = _run(name, i, torch.float64)
    got = {k: t.numpy() for k, t in out.items()}
    if meta["exact"]:  # every operation is exact: the fp64 run holds fp32 values
        for k in got:
            if got[k].dtype == np.float64:
                assert np.array_equal(got[k].astype(np.float32).astype(np.float64), got[k], equal_nan=True), k
                got[k] = got[k].astype(np.float32)
    R.check_against_fixture(got, g, meta, v)


def test_gating_caps_hold_in_every_random_fixture():
    for name in NAMES:
        g, meta = _fixture(name)
        if meta["exact"]:
            continue
        B, M, N = meta["B"], meta["M"], meta["N"]
        for v in meta["variants"]:
            p = v["prefix"]
            assert (g[p + "und_p0"].sum() + g[p + "und_p1"].sum()) <= 0.01 * B * (M + N), (name, p)
            assert (g[p + "und_rows"].sum() + g[p + "und_cols"].sum()) <= 0.03 * B * (M + N), (name, p)
            assert g[p + "und_reward"].sum() <= 0.001 * B * M * N, (name, p)
            assert set(v["tol"]) >= {"proj", "depth", "z", "bound", "r2", "tau", "epi"}


def test_exact_fixture_covers_what_it_is_for():
    g, meta = _fixture("gtd_exact_b3_m64_n48")
    m = np.concatenate([g["plain_matches0"].ravel(), g["plain_matches1"].ravel()])
    assert (m > -1).any() and (m == -1).any() and (m == -2).any()
    assert np.isnan(g["plain_depth_keypoints0"]).any() or np.isnan(g["plain_depth_keypoints1"]).any()
    assert set(np.unique(g["plain_reward"])) == {-1.0, 0.0, 1.0}
    lost = (g["plain_visible0"] & ~g["cc_visible0"]).sum() + (g["plain_visible1"] & ~g["cc_visible1"]).sum()
    assert lost >= 3  # the consistency check takes visibility away
    assert (g["ccepi_matches0"] != g["cc_matches0"]).sum() + (g["ccepi_matches1"] != g["cc_matches1"]).sum() >= 1
    # tied minima: duplicated points, and the lowest index wins
    assert np.array_equal(g["keypoints0"][:, -16:], g["keypoints0"][:, :16])
