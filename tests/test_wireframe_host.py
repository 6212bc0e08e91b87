"""Host-side checks of the wireframe binding (no GPU): exports and ABI, struct layouts, registry
names, the refusals, and the LSD wrapper's post-processing with an injected detector."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.wireframe import MAX_LINES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lg_wireframe_workspace_bytes", "lg_wireframe_forward", "lg_wireframe_connectivity",
           "lg_sample_descriptors_corner"]


def test_exports_and_abi():
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {s for s in exported if s.startswith("lg_wireframe_") or s.startswith("lg_sample_descriptors")} == set(SYMBOLS)
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION


def test_ctypes_structs_match_header(tmp_path):
    structs = {"lg_wireframe_config_t": _lib.WFConfig, "lg_wireframe_inputs_t": _lib.WFInputs,
               "lg_wireframe_outputs_t": _lib.WFOutputs}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "wireframe_mi355x.h")}"',
             "int main(void) {", 'printf("max lines %d\\n", LG_WIREFRAME_MAX_LINES);',
             'printf("max dim %d\\n", LG_WIREFRAME_MAX_DIM);']
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
    assert got[("max", "lines")] == _lib.LG_WIREFRAME_MAX_LINES and got[("max", "dim")] == _lib.LG_WIREFRAME_MAX_DIM
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)


def test_registry_names():
    from lightglue_amd import LSD, WireframeExtractor
    from lightglue_amd.pipeline import get_model

    for name in ("lines.wireframe", "wireframe", "gluefactory.models.lines.wireframe"):
        assert get_model(name) is WireframeExtractor, name
    for name in ("lines.lsd", "lsd", "gluefactory.models.lines.lsd"):
        assert get_model(name) is LSD, name
    assert WireframeExtractor.required_data_keys == ["image"] and LSD.required_data_keys == ["image"]
    assert WireframeExtractor.default_conf == {
        "point_extractor": {"name": None, "trainable": False, "dense_outputs": True, "max_num_keypoints": None,
                            "force_num_keypoints": False},
        "line_extractor": {"name": None, "trainable": False, "max_num_lines": None, "force_num_lines": False,
                           "min_length": 15},
        "wireframe_params": {"merge_points": True, "merge_line_endpoints": True, "nms_radius": 3}}
    assert LSD.default_conf == {"min_length": 15, "max_num_lines": None, "force_num_lines": False, "n_jobs": 4}


class _Points(torch.nn.Module):
    def __init__(self, conf):
        super().__init__()


def _extractor(**point):
    from lightglue_amd import WireframeExtractor
    from lightglue_amd.pipeline import register_model

    register_model("test_wireframe_points", _Points)
    return WireframeExtractor({"point_extractor": {"name": "test_wireframe_points", **point}, "line_extractor": {"name": None}})


def test_configuration_and_shape_errors():
    from lightglue_amd import lines_to_wireframe, sample_descriptors_corner_conv

    m = _extractor()
    assert m.line_extractor is None and isinstance(m.point_extractor, _Points)
    with pytest.raises(AssertionError, match="Missing key image"):
        m({})
    with pytest.raises(AssertionError, match="batch size of 1"):  # B > 1 without both force flags
        m({"image": torch.zeros(2, 1, 120, 160)})
    with pytest.raises(AssertionError, match="batch size of 1"):
        _extractor(force_num_keypoints=True)({"image": torch.zeros(2, 1, 120, 160)})
    with pytest.raises(RuntimeError, match="HIP"):  # CPU inputs
        m({"image": torch.zeros(1, 1, 120, 160)})
    with pytest.raises(RuntimeError, match="HIP"):
        lines_to_wireframe(torch.zeros(1, 3, 2, 2), torch.zeros(1, 3), torch.zeros(1, 256, 15, 20), 8, 3, False, None)
    with pytest.raises(RuntimeError, match="HIP"):
        sample_descriptors_corner_conv(torch.zeros(1, 3, 2), torch.zeros(1, 256, 15, 20))
    with pytest.raises(AssertionError, match="max_num_lines"):
        from lightglue_amd import WireframeExtractor

        WireframeExtractor({"point_extractor": {"name": "test_wireframe_points"},
                            "line_extractor": {"name": None, "force_num_lines": True}})
    lib = _lib.load()
    nb = ctypes.c_size_t()
    # E over capacity
    assert MAX_LINES == _lib.LG_WIREFRAME_MAX_LINES == 2048
    assert lib.lg_wireframe_workspace_bytes(1, _lib.LG_WIREFRAME_MAX_LINES, 10, ctypes.byref(nb)) == 0 and nb.value > 0
    assert lib.lg_wireframe_workspace_bytes(1, _lib.LG_WIREFRAME_MAX_LINES + 1, 10, ctypes.byref(nb)) == _lib.LG_E_INVALID
    assert b"too many lines" in lib.lg_last_error()
    assert lib.lg_wireframe_workspace_bytes(1, -1, 10, ctypes.byref(nb)) == _lib.LG_E_INVALID
    assert lib.lg_wireframe_workspace_bytes(1, 1, 1, None) == _lib.LG_E_INVALID
    cfg = _lib.WFConfig(3.0, 1, 1, 0, 0, 8, 0)
    out = _lib.WFOutputs()
    over = _lib.WFInputs(1, _lib.LG_WIREFRAME_MAX_LINES + 1, 0, 2 * _lib.LG_WIREFRAME_MAX_LINES + 2, 256, 15, 20, 0)
    assert lib.lg_wireframe_forward(ctypes.byref(cfg), ctypes.byref(over), ctypes.byref(out), None, 0, None) == _lib.LG_E_INVALID
    assert b"too many lines" in lib.lg_last_error()
    # D not a multiple of 4, D over the limit, J inconsistent with L: refused before any pointer is read
    for D in (6, 255, 0, 1028):
        bad = _lib.WFInputs(1, 4, 0, 8, D, 15, 20, 0)
        assert lib.lg_wireframe_forward(ctypes.byref(cfg), ctypes.byref(bad), ctypes.byref(out), None, 0, None) == _lib.LG_E_INVALID
        assert b"multiple of 4" in lib.lg_last_error()
        assert lib.lg_sample_descriptors_corner(None, None, 1, 3, 15, 20, D, 8, None, None) == _lib.LG_E_INVALID
    bad = _lib.WFInputs(1, 4, 0, 6, 256, 15, 20, 0)
    assert lib.lg_wireframe_forward(ctypes.byref(cfg), ctypes.byref(bad), ctypes.byref(out), None, 0, None) == _lib.LG_E_INVALID
    ok = _lib.WFInputs(1, 4, 0, 8, 256, 15, 20, 0)  # null pointers are an error, not a crash
    assert lib.lg_wireframe_forward(ctypes.byref(cfg), ctypes.byref(ok), ctypes.byref(out), None, 0, None) == _lib.LG_E_INVALID
    assert lib.lg_wireframe_forward(None, None, None, None, 0, None) == _lib.LG_E_INVALID
    assert lib.lg_wireframe_connectivity(None, 1, 4, 8, 0, None, None) == _lib.LG_E_INVALID
    assert lib.lg_wireframe_connectivity(None, 1, 4, 0, 0, None, None) == 0  # nothing to write


def _segments(rng, n):
    p = rng.random((n, 2)) * 100
    ang, length = rng.random(n) * 2 * np.pi, rng.random(n) * 40
    q = p + np.stack([np.cos(ang), np.sin(ang)], 1) * length[:, None]
    return np.concatenate([p, q, np.ones((n, 1)), 1 + rng.permutation(n)[:, None].astype(np.float64)], 1)  # [n, 6], nfa last


@pytest.mark.parametrize("conf", [{}, {"max_num_lines": 10}, {"max_num_lines": 40, "force_num_lines": True},
                                  {"max_num_lines": 12, "force_num_lines": True, "min_length": 25}])
def test_lsd_postprocessing_with_injected_detector(conf):
    """lsd.py:24-85 stated in numpy: length filter, score = nfa * sqrt(length), the best max_num_lines
    in descending order (detector order without a limit, as in the reference), zero padding and
    valid_lines under force_num_lines."""
    from lightglue_amd import LSD

    rng = np.random.Generator(np.random.PCG64(5))
    per_image = [_segments(rng, 30), _segments(rng, 25)]
    B = 2 if conf.get("force_num_lines") else 1
    seen = []

    def detector(img):
        assert img.dtype == np.uint8 and img.shape == (24, 32)
        seen.append(img.copy())
        return per_image[len(seen) - 1]

    class Injected(LSD):
        pass

    Injected.detector = staticmethod(detector)
    image = torch.from_numpy(rng.random((B, 3, 24, 32)).astype(np.float32))
    out = Injected(conf)({"image": image})
    gray = (image * torch.tensor([0.299, 0.587, 0.114]).view(1, 3, 1, 1)).sum(1).numpy()
    for b in range(B):
        np.testing.assert_array_equal(seen[b], np.uint8(gray[b] * 255))
        segs = per_image[b]
        length = np.sqrt(((segs[:, 2:4] - segs[:, 0:2]) ** 2).sum(1))
        keep = length >= conf.get("min_length", 15)
        score = segs[keep, 5] * np.sqrt(length[keep])
        assert len(set(score.tolist())) == len(score)  # distinct: the order is defined
        # lsd.py:36-40 applies the descending order only together with the max_num_lines cut
        order = np.argsort(-score)[: conf["max_num_lines"]] if "max_num_lines" in conf else np.arange(len(score))
        n = len(order)
        total = conf["max_num_lines"] if conf.get("force_num_lines") else n
        assert out["lines"].shape == (B, total, 2, 2) and out["line_scores"].shape == (B, total)
        np.testing.assert_array_equal(out["lines"][b, :n].numpy(), segs[keep][order, :4].reshape(-1, 2, 2).astype(np.float32))
        np.testing.assert_array_equal(out["line_scores"][b, :n].numpy(), score[order].astype(np.float32))
        assert (out["lines"][b, n:] == 0).all() and (out["line_scores"][b, n:] == 0).all()
        np.testing.assert_array_equal(out["valid_lines"][b].numpy(), np.arange(total) < n)
    assert out["lines"].dtype == torch.float32 and out["valid_lines"].dtype == torch.bool


def test_lsd_without_pytlsd_raises_import_error(monkeypatch):
    from lightglue_amd import LSD

    monkeypatch.setitem(sys.modules, "pytlsd", None)  # import pytlsd -> ImportError, installed or not
    with pytest.raises(ImportError, match="pytlsd"):
        LSD({})({"image": torch.zeros(1, 1, 24, 32)})
    with pytest.raises(AssertionError, match="max_num_lines"):
        LSD({"force_num_lines": True})
