"""The torch restatement of GlueStick (tests/gluestick_ref.py) against fixtures the REAL reference
produced (tests/golden/make_gluestick_golden.py): this pins the yardstick the GPU tests use."""
import numpy as np
import pytest
import torch

from gluestick_golden_util import (BAND, FLOAT_KEYS, MATCH_KEYS, REF_ERR_FACTOR, case_names, decided, load_case, margins,
                                   recipe_inputs, ref_data)
from gluestick_ref import gluestick_forward, nll

CASES = case_names()


def test_fixtures_present():
    assert len(CASES) >= 3


@pytest.fixture(scope="module", params=CASES)
def case(request):
    z, meta = load_case(request.param)
    sd, pair = recipe_inputs(meta["recipe"])
    data = ref_data(meta["recipe"], pair)
    with torch.no_grad():
        r64 = gluestick_forward(sd, data, meta["recipe"]["conf"], torch.float64)
        r32 = gluestick_forward(sd, data, meta["recipe"]["conf"], torch.float32)
    return z, meta, pair, r64, r32


def test_fp64_restatement_reproduces_reference(case):
    z, meta, _, r64, _ = case
    for k in FLOAT_KEYS:
        ref = z["out_" + k]
        assert ref.dtype == np.float64
        bar = REF_ERR_FACTOR * float(z["e_" + k])
        err = float(np.abs(r64[k].numpy() - ref).max())
        print(f"{k}: max err {err:.3e} (bar {bar:.3e})")
        assert err <= bar, k
    for k in MATCH_KEYS:
        np.testing.assert_array_equal(r64[k].numpy(), z["out_" + k], err_msg=k)


def test_fp32_restatement_matches_outside_band(case):
    z, meta, _, _, r32 = case
    th = meta["filter_threshold"]
    for head in ("", "line_"):
        ok0, ok1 = decided(z[f"out_{head}log_assignment"], th)
        for k, ok in ((f"{head}matches0", ok0), (f"{head}matches1", ok1)):
            got = r32[k].numpy()
            assert not ((got != z["out_" + k]) & ok).any(), k
            assert not ((got != z["m32_" + k]) & ok).any(), k


def test_fixture_conditions(case):
    z, meta, pair, r64, _ = case
    th = meta["filter_threshold"]
    for head in ("", "line_"):
        assert (z[f"out_{head}matches0"] >= 0).mean() >= 0.25
        mg = {k: z[f"margin_{head}{k}"] for k in ("row_gap", "col_gap", "row_th", "col_th")}
        for k, v in margins(r64[head + "log_assignment"].numpy(), th).items():  # the stored margins are the fp64 run's
            np.testing.assert_allclose(v, mg[k], atol=1e-7, err_msg=head + k)
        assert ((mg["row_gap"] > BAND) & (mg["row_th"] > BAND)).mean() >= 0.9
        assert ((mg["col_gap"] > BAND) & (mg["col_th"] > BAND)).mean() >= 0.9
    assert meta["line_effect"] >= 100 * 1e-4
    for v in "01":
        for b in range(meta["recipe"]["B"]):
            j = np.sort(pair["lines_junc_idx" + v][b], 1)
            assert (j[:, 0] != j[:, 1]).all()
            assert len({tuple(r) for r in j}) == len(j)
            deg = np.bincount(pair["lines_junc_idx" + v][b].ravel())
            assert deg.max() >= 5 and deg[deg > 0].min() == 1


def test_line_layers_matter(case):
    """line_effect, recomputed by the restatement: a forward without the line layers differs."""
    z, meta, pair, r64, _ = case
    conf = {**meta["recipe"]["conf"], "num_line_iterations": 0}
    sd, _ = recipe_inputs(meta["recipe"])
    with torch.no_grad():
        off = gluestick_forward(sd, ref_data(meta["recipe"], pair), conf, torch.float64)
    eff = max(float((r64[f"gnn_descriptors{v}"] - off[f"gnn_descriptors{v}"]).abs().max()) for v in "01")
    assert abs(eff - meta["line_effect"]) <= 1e-6
    assert len(r64["line_layer_x"]) == sum(k == "self" for k in meta["recipe"]["conf"].get("GNN_layers", ["self", "cross"] * 9))


def test_loss_values(case):
    z, meta, pair, r64, _ = case
    bal = 0.5
    total = 0
    for head in ("", "line_"):
        v, npos, nneg = nll(r64[head + "log_assignment"], torch.from_numpy(pair[f"gt_{head}assignment"]),
                            torch.from_numpy(pair[f"gt_{head}matches0"]), torch.from_numpy(pair[f"gt_{head}matches1"]), bal)
        np.testing.assert_allclose(v.numpy(), z[f"loss_{head}assignment_nll"], rtol=1e-9)
        np.testing.assert_allclose(npos.numpy(), z[f"loss_{head}num_matchable"])
        np.testing.assert_allclose(nneg.numpy(), z[f"loss_{head}num_unmatchable"])
        total = total + v
    np.testing.assert_allclose(total.numpy(), z["loss_total"], rtol=1e-9)
