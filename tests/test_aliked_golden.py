"""The CPU restatement of ALIKED (tests/aliked_ref.py) against the reference's own outputs
(tests/golden/aliked/*.npz, made by tests/golden/make_aliked_golden.py from the real reference on
recipe weights): identical keypoint sets, values within the bars of tests/aliked_golden_util.py.
This is what lets the GPU tests use the restatement (in fp64) as their reference on further seeded
cases."""
import numpy as np
import pytest
import torch

import aliked_ref
from aliked_golden_util import aliked_case_inputs, aliked_case_names, aliked_load, compare, fixture_bars, sha
from lightglue_amd.aliked_weights import ALIKED_CFGS, aliked_schema

CASES = aliked_case_names()


def test_fixtures_present():
    assert len(CASES) == 4, CASES
    models = {aliked_load(n)["meta"]["conf"]["model_name"] for n in CASES}
    assert models == {"aliked-n16", "aliked-t16", "aliked-n32"}


@pytest.mark.parametrize("name", CASES)
def test_recipe_regenerates_inputs(name):
    meta = aliked_load(name)["meta"]
    _, sd, data = aliked_case_inputs(meta)
    assert sha({"image": data["image"]}) == meta["inputs_sha256"]
    assert sha(sd) == meta["weights_sha256"]
    assert [(n, list(s)) for n, s in aliked_schema(meta["conf"]["model_name"])] == [tuple(x) for x in meta["ref_state_dict"]]
    k = meta["conf"]["max_num_keypoints"]
    bar = fixture_bars(meta)["score"]
    assert min(meta["kth_gap"]) > 4 * bar and min(meta["thr_gap"]) > 4 * bar
    if k > 0:
        assert min(meta["positive"]) >= k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(name, dtype):
    g = aliked_load(name)
    conf, sd, data = aliked_case_inputs(g["meta"])
    out = aliked_ref.aliked_forward(sd, data, conf, dtype)
    ref = {k[4:]: v for k, v in g.items() if k.startswith("out_")}
    compare({k: (np.asarray(v) if isinstance(v, torch.Tensor) else [np.asarray(t) for t in v])
             for k, v in out.items() if k in ref}, ref, fixture_bars(g["meta"]), f"{name} {dtype}")


def test_deform_conv_is_conv_at_zero_offsets():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 7, 9, dtype=torch.float64, generator=g)
    w = torch.randn(6, 5, 3, 3, dtype=torch.float64, generator=g)
    b = torch.randn(6, dtype=torch.float64, generator=g)
    got = aliked_ref.deform_conv2d(x, torch.zeros(2, 18, 7, 9, dtype=torch.float64), w, b, padding=1)
    assert float((got - torch.nn.functional.conv2d(x, w, b, padding=1)).abs().max()) < 1e-12


def test_deform_conv_limits():
    """One input pixel of value 1 at (0, 0), one tap active: positions just inside and just outside
    the -1 and H limits, and an exactly integer position."""
    x = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    x[0, 0, 0, 0] = 1.0
    x[0, 0, 2, 2] = 1.0
    w = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    w[0, 0, 1, 1] = 1.0  # the centre tap: samples (y + dy, x + dx)
    def at(y, x_, dy, dx):
        off = torch.zeros(1, 18, 3, 3, dtype=torch.float64)
        off[0, 8, y, x_], off[0, 9, y, x_] = dy, dx
        return float(aliked_ref.deform_conv2d(x, off, w, None, padding=1)[0, 0, y, x_])
    assert at(0, 0, 0.0, 0.0) == 1.0
    assert at(1, 1, -1.0, -1.0) == 1.0             # exactly integer
    assert abs(at(0, 0, -0.75, 0.0) - 0.25) < 1e-15  # y = -0.75: the row -1 corner contributes 0
    assert at(0, 0, -1.0, 0.0) == 0.0              # y = -1: outside
    assert abs(at(2, 2, 0.75, 0.0) - 0.25) < 1e-15   # y = 2.75 < H
    assert at(2, 2, 1.0, 0.0) == 0.0               # y = 3 = H: outside


def test_cfg_table():
    assert set(ALIKED_CFGS) == {"aliked-t16", "aliked-n16", "aliked-n16rot", "aliked-n32"}
