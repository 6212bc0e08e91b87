"""Host-side contract of the open SuperPoint extractor (no GPU): registry names, the module's
parameter tree against the schema and the reference's recorded key list, config keys, the ctypes
mirror of sp_open_config_t, the exported symbol, and the configs and inputs that raise."""
import ctypes
import os
import subprocess

import pytest
import torch

from lightglue_amd import _lib, pipeline
from lightglue_amd.sp_weights import (SPO_DEFAULT_CONF, superpoint_open_schema, superpoint_open_state_dict)
from spo_golden_util import spo_case_names, spo_load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_resolves_the_reference_names():
    import lightglue_amd
    from lightglue_amd.superpoint_open import SuperPoint

    for name in ("extractors.superpoint_open", "superpoint_open"):
        assert pipeline.get_model(name) is SuperPoint
    assert lightglue_amd.SuperPointOpen is SuperPoint
    # the nonfree names still resolve to the nonfree module
    assert pipeline.get_model("extractors.superpoint") is lightglue_amd.SuperPoint
    assert lightglue_amd.SuperPoint is not SuperPoint


def test_state_dict_equals_the_schema_and_the_reference_key_list():
    from lightglue_amd.superpoint_open import SuperPoint

    m = SuperPoint({})
    sd = m.state_dict()
    schema = superpoint_open_schema()
    assert len(schema) == 84
    assert list(sd) == [n for n, _ in schema]
    for n, shape in schema:
        assert tuple(sd[n].shape) == tuple(shape), n
    assert sd["backbone.0.0.bn.num_batches_tracked"].dtype == torch.int64
    for name in spo_case_names():  # what the reference's module registered when the fixture was made
        assert list(sd) == spo_load(name)["meta"]["ref_state_dict_keys"]
    # the reference's tree: pools at the same indices, eps 1e-3
    assert [type(x).__name__ for x in m.backbone[0]] == ["VGGBlock", "VGGBlock", "MaxPool2d"]
    assert [type(x).__name__ for x in m.backbone[3]] == ["VGGBlock", "VGGBlock"]
    assert m.backbone[1][1].bn.eps == 0.001 and isinstance(m.detector[1].activation, torch.nn.Identity)
    # a checkpoint in the reference's format loads strictly
    rec = superpoint_open_state_dict(seed=0)
    res = m.load_state_dict({k: torch.from_numpy(v.copy()) if v.ndim else torch.tensor(int(v)) for k, v in rec.items()},
                            strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_recipe_has_mixed_sign_gamma():
    sd = superpoint_open_state_dict(seed=1)
    for blk in ("backbone.0.1", "backbone.1.1", "backbone.2.1"):  # the pooled blocks
        g = sd[f"{blk}.bn.weight"]
        assert 0.1 < (g < 0).mean() < 0.45 and 0.5 <= abs(g).min() and abs(g).max() <= 1.5
    assert sd["detector.1.bn.running_var"].min() >= 0.3 and sd["detector.1.bn.num_batches_tracked"].dtype.kind == "i"


def test_default_conf_keys_match_reference():
    # superpoint_open.py:77-87 + base_model.py:54-59
    assert set(SPO_DEFAULT_CONF) == {
        "name", "trainable", "freeze_batch_normalization", "timeit", "descriptor_dim", "nms_radius",
        "max_num_keypoints", "force_num_keypoints", "detection_threshold", "remove_borders", "channels", "dense_outputs",
    }
    assert SPO_DEFAULT_CONF["max_num_keypoints"] is None and SPO_DEFAULT_CONF["detection_threshold"] == 0.005
    assert SPO_DEFAULT_CONF["channels"] == [64, 64, 128, 128, 256]


def test_sp_open_config_layout_matches_the_header(tmp_path):
    py = _lib.SPOpenConfig
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "superpoint_mi355x.h")}"',
             "int main(void) {", 'printf("size %zu\\n", sizeof(sp_open_config_t));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(sp_open_config_t, {f}));')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(py)
    assert [f for f, _ in py._fields_] == ["descriptor_dim", "nms_radius", "remove_borders", "detection_threshold"]
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f


def test_sp_open_create_is_exported_and_checks_its_arguments():
    lib = _lib.load()
    assert "sp_open_create" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "sp_open_create")
    assert lib.lg_abi_version() == 12  # additive: the ABI version does not move
    h = ctypes.c_void_p()
    assert lib.sp_open_create(None, 0, ctypes.byref(h)) == _lib.LG_E_INVALID
    assert b"null" in lib.lg_last_error()
    cfg = _lib.SPOpenConfig(128, 4, 4, 0.005)
    assert lib.sp_open_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib.LG_E_INVALID
    assert b"descriptor_dim must be 256" in lib.lg_last_error()


def test_cpu_input_and_refused_configs_raise():
    from lightglue_amd.superpoint_open import SuperPoint

    m = SuperPoint({"max_num_keypoints": 10}).eval()
    with pytest.raises(RuntimeError, match="on the CPU"):
        m({"image": torch.zeros(1, 1, 32, 32)})
    with pytest.raises(AssertionError, match="Missing key image"):
        m({})
    with pytest.raises(ValueError, match="descriptor_dim"):
        SuperPoint({"descriptor_dim": 128})
    with pytest.raises(ValueError, match="channels"):
        SuperPoint({"channels": [32, 64, 128, 128, 256]})
    with pytest.raises(ValueError, match="max_num_keypoints"):
        SuperPoint({"max_num_keypoints": 0})
