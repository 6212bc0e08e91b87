"""tests/nn_ref.py (the torch-CPU restatement of the nearest-neighbour matcher) in fp32 against the
fixtures the reference itself produced (tests/golden/make_nn_golden.py): on every decidable item
under the recorded near-tie gating, and on the stored dense outputs of the exact fixture."""
import numpy as np
import pytest
import torch

import nn_ref

EXACT = "nn_exact_b3_m64_n48_d64"


def test_fixtures_present():
    names = nn_ref.fixture_names()
    assert EXACT in names and "nn_ragged_b3_m300_n257_d256" in names and len(names) >= 7


def _run(g, meta, ratio, dist, mutual):
    d0, d1 = torch.from_numpy(g["descriptors0"]), torch.from_numpy(g["descriptors1"])
    if meta["counts"] is not None:
        return nn_ref.nn_forward_ragged(d0, d1, meta["counts"][0], meta["counts"][1], ratio, dist, mutual)
    return nn_ref.nn_forward(d0, d1, ratio, dist, mutual)


@pytest.mark.parametrize("name", nn_ref.fixture_names())
def test_restatement_matches_reference(name):
    g, meta = nn_ref.load_fixture(name)
    for ratio, dist, mutual in nn_ref.FLAVOURS:
        got = {k: v.numpy() for k, v in _run(g, meta, ratio, dist, mutual).items()}
        assert got["matches0"].dtype == np.int64 and got["matching_scores0"].dtype == np.float32
        nn_ref.check_against_fixture(got, g, meta, ratio, dist, mutual)


def test_exact_fixture_dense_outputs():
    """The exact fixture's descriptors are multiples of 1/64 with |q| <= 127: every product and
    every partial sum of the similarity is exact in fp32, so any summation order gives the stored
    bits.  The log assignment goes through exp and log, whose vectorised CPU implementations may
    differ in the last place between hosts: 4 ulp of its largest magnitude."""
    g, meta = nn_ref.load_fixture(EXACT)
    assert meta["exact"] and meta["e"] == 0.0
    out = _run(g, meta, None, None, True)
    sim, la = out["similarity"].numpy(), out["log_assignment"].numpy()
    assert sim.dtype == np.float32 and la.dtype == np.float32
    np.testing.assert_array_equal(sim.view(np.uint32), g["similarity"].view(np.uint32))
    np.testing.assert_array_equal(sim.astype(np.float64), nn_ref.sim64(g["descriptors0"], g["descriptors1"]).numpy())
    assert (la[:, -1] == 0).all() and (la[:, :, -1] == 0).all()
    np.testing.assert_allclose(la, g["log_assignment"], rtol=0, atol=4 * 2.0**-23 * float(np.abs(la).max()))


def test_fixture_gating_is_within_its_caps():
    """What the generator asserted, re-read from the files: undecidable rows + columns <= 3 % per
    fixture and flavour, and tol = 4 max(e, 2.4e-7 S)."""
    for name in nn_ref.fixture_names():
        g, meta = nn_ref.load_fixture(name)
        assert meta["tol"] == 4.0 * max(meta["e"], nn_ref.H3_ERR * meta["S"])
        e, S, tol = nn_ref.tol_of(g["descriptors0"], g["descriptors1"])
        assert S == pytest.approx(meta["S"], rel=1e-12)
        for ratio, dist, mutual in nn_ref.FLAVOURS:
            k = nn_ref.flavour_key(ratio, dist, mutual)
            ur, uc = g[k + "/und_rows"], g[k + "/und_cols"]
            assert ur.sum() + uc.sum() <= 0.03 * (ur.size + uc.size), (name, k)
            c0, c1 = meta["counts"] if meta["counts"] is not None else (None, None)
            mg = nn_ref.margins(g["descriptors0"], g["descriptors1"], ratio, dist, mutual, meta["tol"], c0, c1)
            assert np.array_equal(mg["und_rows"], ur) and np.array_equal(mg["und_cols"], uc), (name, k)


def test_thresholds_exercise_both_branches():
    g, meta = nn_ref.load_fixture("nn_b2_m300_n257_d256")
    for ratio, dist, mutual in nn_ref.FLAVOURS:
        m0 = g[nn_ref.flavour_key(ratio, dist, mutual) + "/matches0"]
        if ratio or dist or mutual:
            assert 0 < (m0 > -1).sum() < m0.size
        else:
            assert (m0 > -1).all()
