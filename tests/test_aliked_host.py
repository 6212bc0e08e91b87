"""Host-side checks of lightglue_amd.ALIKED: the module tree against the reference's state_dict
(as recorded in the fixtures), the recipe weights, the registry names, the exported symbols and the
config / input errors.  No GPU."""
import os
import re

import pytest
import torch

from aliked_golden_util import aliked_case_names, aliked_load
from lightglue_amd import _lib
from lightglue_amd.aliked_weights import ALIKED_CFGS, ALIKED_DEFAULT_CONF, aliked_schema, aliked_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sp_aliked_create", "sp_aliked_destroy", "sp_aliked_weight_count", "sp_aliked_weight_name",
           "sp_aliked_weight_numel", "sp_aliked_load_weights", "sp_aliked_workspace_bytes", "sp_aliked_forward",
           "sp_aliked_deform_conv", "sp_aliked_set_profile", "sp_aliked_stage_ms"]


def as_torch_sd(sd):
    return {k: torch.from_numpy(v.copy()) if v.ndim else torch.tensor(int(v)) for k, v in sd.items()}


@pytest.mark.parametrize("model_name", sorted(ALIKED_CFGS))
def test_state_dict_matches_reference(model_name):
    from lightglue_amd import ALIKED

    m = ALIKED({"model_name": model_name})
    got = [(k, list(v.shape)) for k, v in m.state_dict().items()]
    assert got == [(n, list(s)) for n, s in aliked_schema(model_name)]
    # the reference's own list, where a fixture of this architecture recorded it (n16rot = n16)
    arch = {"aliked-n16rot": "aliked-n16"}.get(model_name, model_name)
    recorded = [aliked_load(n)["meta"] for n in aliked_case_names()]
    recorded = [r for r in recorded if r["conf"]["model_name"] == arch]
    assert recorded, arch
    assert got == [tuple(x) for x in recorded[0]["ref_state_dict"]]
    m.load_state_dict(as_torch_sd(aliked_state_dict(model_name, seed=3)), strict=True)
    assert float(m.block3.conv1.offset_conv.bias.detach().abs().sum()) > 0


def test_default_conf_and_registry():
    from lightglue_amd import ALIKED
    from lightglue_amd.pipeline import get_model

    assert get_model("extractors.aliked") is ALIKED and get_model("aliked") is ALIKED
    for k, v in {"model_name": "aliked-n16", "max_num_keypoints": -1, "detection_threshold": 0.2,
                 "force_num_keypoints": False, "pretrained": True, "nms_radius": 2}.items():
        assert ALIKED_DEFAULT_CONF[k] == v
    m = ALIKED({})
    assert m.conf.model_name == "aliked-n16" and not m._topk
    assert ALIKED({"max_num_keypoints": 64, "detection_threshold": 0.0})._topk
    with pytest.raises(NotImplementedError):
        m.loss({}, {})


def test_symbols_and_abi():
    lib = _lib.load()
    assert lib.lg_abi_version() == 12 and _lib.ABI_VERSION == 12
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    with open(os.path.join(ROOT, "include", "aliked_mi355x.h")) as f:
        declared = set(re.findall(r"\b(sp_aliked_\w+)\s*\(", f.read()))
    assert declared == set(SYMBOLS)


def test_config_and_input_errors():
    from lightglue_amd import ALIKED

    with pytest.raises(ValueError, match="force_num_keypoints"):
        ALIKED({"force_num_keypoints": True})  # threshold mode
    with pytest.raises(ValueError, match="force_num_keypoints"):
        ALIKED({"force_num_keypoints": True, "detection_threshold": 0.0, "max_num_keypoints": -1})
    ALIKED({"force_num_keypoints": True, "detection_threshold": 0.0, "max_num_keypoints": 32})
    with pytest.raises(ValueError, match="model_name"):
        ALIKED({"model_name": "aliked-x64"})
    m = ALIKED({"max_num_keypoints": 16, "detection_threshold": 0.0})
    with pytest.raises(ValueError, match="3, H, W"):
        m({"image": torch.zeros(1, 1, 32, 32)})
    with pytest.raises(RuntimeError, match="HIP device"):
        m({"image": torch.zeros(1, 3, 32, 32)})
