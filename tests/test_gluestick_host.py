"""Host-side checks of the GlueStick binding (no GPU): module tree and registry, the C schema, the
refusals, the empty-keypoint outputs, checkpoint key rewriting, exports and struct layouts."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.gs_weights import GS_DEFAULT_CONF, gluestick_schema, gluestick_state_dict, wireframe_pair

from gluestick_golden_util import case_names, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sg_gluestick_create", "sg_gluestick_destroy", "sg_gluestick_weight_count", "sg_gluestick_weight_name",
           "sg_gluestick_weight_numel", "sg_gluestick_load_weights", "sg_gluestick_workspace_bytes",
           "sg_gluestick_forward", "sg_gluestick_line_update", "sg_gluestick_double_softmax", "sg_gluestick_line_scores"]


def _pair(B=1):
    p = wireframe_pair(B, (4, 5), (3, 3), (3, 4), seed=1)
    d = {k: torch.from_numpy(v) for k, v in p.items() if not k.startswith("gt_")}
    d["view0"] = d["view1"] = {"image_size": torch.tensor([[640.0, 480.0]] * B)}
    return d


def test_import_and_registry():
    from lightglue_amd import GlueStick
    from lightglue_amd.pipeline import get_model

    assert get_model("matchers.gluestick") is GlueStick
    assert get_model("gluestick") is GlueStick
    assert GlueStick.default_conf == GS_DEFAULT_CONF
    assert GlueStick.required_data_keys == [
        "view0", "view1", "keypoints0", "keypoints1", "descriptors0", "descriptors1", "keypoint_scores0",
        "keypoint_scores1", "lines0", "lines1", "lines_junc_idx0", "lines_junc_idx1", "line_scores0", "line_scores1"]


@pytest.mark.parametrize("name", case_names())
def test_state_dict_matches_reference(name):
    """Keys, order and shapes of the module's state dict equal the real reference's (fixture list)."""
    from lightglue_amd import GlueStick

    _, meta = load_case(name)
    conf = meta["recipe"]["conf"]
    sd = GlueStick(conf).state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["state_dict"]
    assert [[n, list(s)] for n, s, _ in gluestick_schema(conf)] == meta["state_dict"]
    # the recipe weights load strictly
    GlueStick(conf).load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                                     gluestick_state_dict(conf, seed=1).items()}, strict=True)


@pytest.mark.parametrize("conf", [{}, {"GNN_layers": ["self", "cross", "self"], "keypoint_encoder": [16, 32]}])
def test_c_schema_equals_module(conf):
    from lightglue_amd import GlueStick

    lib = _lib.load()
    m = GlueStick(conf)
    h = ctypes.c_void_p()
    _lib.check(lib.sg_gluestick_create(ctypes.byref(m._lib_config()), 0, ctypes.byref(h)), "create")
    try:
        want = [(k, v.numel()) for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")]
        n = lib.sg_gluestick_weight_count(h)
        got = [(lib.sg_gluestick_weight_name(h, i).decode(), lib.sg_gluestick_weight_numel(h, i)) for i in range(n)]
        assert got == want
        assert lib.sg_gluestick_weight_name(h, n) is None and lib.sg_gluestick_weight_numel(h, -1) == -1
    finally:
        lib.sg_gluestick_destroy(h)


def test_unsupported_configurations_raise():
    from lightglue_amd import GlueStick

    with pytest.raises(NotImplementedError):
        GlueStick({"line_attention": True})
    with pytest.raises(NotImplementedError):
        GlueStick({"inter_supervision": [2, 5]})
    with pytest.raises(ValueError):
        GlueStick({"descriptor_dim": 128})
    with pytest.raises(ValueError):
        GlueStick({"input_dim": 128})
    GlueStick({"skip_init": True, "checkpointed": True, "weights": "no_such_checkpoint"})  # accepted, inert
    m = GlueStick({"GNN_layers": ["self", "cross"]}).train()
    with pytest.raises(NotImplementedError):
        m(_pair())
    lib = _lib.load()
    cfg = GlueStick({})._lib_config()
    cfg.num_line_iterations = -1
    h = ctypes.c_void_p()
    assert lib.sg_gluestick_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib.LG_E_INVALID


def test_cpu_inputs_raise():
    from lightglue_amd import GlueStick

    m = GlueStick({"GNN_layers": ["self", "cross"]}).eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        m(_pair())
    d = _pair()
    del d["line_scores1"]
    with pytest.raises(AssertionError, match="Missing key line_scores1"):
        m(d)


def test_empty_keypoints_outputs():
    """gluestick.py:156-188 on the host, before any device check; line_matching_scores1 is sized by
    the lines (the reference sizes it by n_kpts1)."""
    from lightglue_amd import GlueStick

    m = GlueStick({"GNN_layers": ["self", "cross"]}).eval()
    B, N, L0, L1 = 2, 5, 3, 4
    d = {"keypoints0": torch.zeros(B, 0, 2), "keypoints1": torch.zeros(B, N, 2), "descriptors0": torch.zeros(B, 0, 256),
         "descriptors1": torch.zeros(B, N, 256), "keypoint_scores0": torch.zeros(B, 0), "keypoint_scores1": torch.zeros(B, N),
         "lines0": torch.zeros(B, L0, 2, 2), "lines1": torch.zeros(B, L1, 2, 2),
         "lines_junc_idx0": torch.zeros(B, L0, 2, dtype=torch.int64), "lines_junc_idx1": torch.zeros(B, L1, 2, dtype=torch.int64),
         "line_scores0": torch.zeros(B, L0), "line_scores1": torch.zeros(B, L1), "view0": {}, "view1": {}}
    p = m(d)
    want = {"log_assignment": ((B, 0, N), torch.float32), "matches0": ((B, 0), torch.int64), "matches1": ((B, N), torch.int64),
            "matching_scores0": ((B, 0), torch.float32), "matching_scores1": ((B, N), torch.float32),
            "line_log_assignment": ((B, L0, L1), torch.float32), "line_matches0": ((B, L0), torch.int64),
            "line_matches1": ((B, L1), torch.int64), "line_matching_scores0": ((B, L0), torch.float32),
            "line_matching_scores1": ((B, L1), torch.float32)}
    assert set(p) == set(want)
    for k, (shape, dtype) in want.items():
        assert tuple(p[k].shape) == shape and p[k].dtype == dtype, k
        assert bool((p[k] == (-1 if "matches" in k else 0)).all()), k


def test_state_dict_from_checkpoint(tmp_path):
    from lightglue_amd import GlueStick

    conf = {"GNN_layers": ["self", "cross"]}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in gluestick_state_dict(conf, seed=3).items()}
    ckpt = {"model": {**{"matcher.module." + k: v for k, v in sd.items()}, "extractor.conv.weight": torch.zeros(3)},
            "epoch": 7}
    got = GlueStick.state_dict_from_checkpoint(ckpt)
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert GlueStick.state_dict_from_checkpoint(sd) is sd  # already a state dict
    path = tmp_path / "ckpt.tar"
    torch.save(ckpt, path)
    m = GlueStick({**conf, "weights": str(path)})
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_exports_and_abi():
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {s for s in exported if s.startswith("sg_gluestick_")} == set(SYMBOLS)
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION


def test_ctypes_structs_match_header(tmp_path):
    structs = {"sg_gluestick_config_t": _lib.GSConfig, "sg_gluestick_inputs_t": _lib.GSInputs,
               "sg_gluestick_outputs_t": _lib.GSOutputs}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "gluestick_mi355x.h")}"',
             "int main(void) {", 'printf("iters x %d\\n", SG_GLUESTICK_MAX_LINE_ITERS);']
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        c, f, v = line.split()
        got[(c, f)] = int(v)
    assert got[("iters", "x")] == _lib.SG_GLUESTICK_MAX_LINE_ITERS
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)


def test_workspace_bytes():
    from lightglue_amd import GlueStick

    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.sg_gluestick_create(ctypes.byref(GlueStick({})._lib_config()), 0, ctypes.byref(h)), "create")
    try:
        def nbytes(*a):
            b = ctypes.c_size_t()
            rc = lib.sg_gluestick_workspace_bytes(h, *a, ctypes.byref(b))
            return rc, b.value

        base = (2, 100, 120, 30, 40)
        rc, b0 = nbytes(*base)
        assert rc == 0 and b0 > 0
        for i in range(5):
            grown = list(base)
            grown[i] += 64
            rc, b1 = nbytes(*grown)
            assert rc == 0 and b1 > b0, i
            neg = list(base)
            neg[i] = -1
            assert nbytes(*neg)[0] == _lib.LG_E_INVALID, i
        # either image without lines: no line buffers at all
        assert nbytes(2, 100, 120, 0, 40)[1] == nbytes(2, 100, 120, 0, 0)[1] < b0
        assert lib.sg_gluestick_workspace_bytes(h, 1, 1, 1, 1, 1, None) == _lib.LG_E_INVALID
    finally:
        lib.sg_gluestick_destroy(h)
