"""Host-side checks of the ragged-batch interface (no GPU): the ABI version, the layout of
lg_inputs_t against the C header, the input checks of LightGlue.forward, and the oracle-side facts
the GPU tests (test_gpu_ragged.py) rest on, so that a drift of the fixture shows on the CPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ragged_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_abi_is_12():
    """11 brought the ragged fields of lg_inputs_t, 12 lg_train_gemm_ex."""
    from lightglue_amd import _lib

    lib = _lib.load()
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_lginputs_layout_equals_the_header(tmp_path):
    from lightglue_amd import _lib

    fields = [name for name, _ in _lib.LGInputs._fields_]
    assert fields[-3:] == ["flags", "num_keypoints0", "num_keypoints1"]
    prints = "".join(f'  printf("%zu\\n", offsetof(lg_inputs_t, {f}));\n' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lightglue_mi355x.h"\n'
                   'int main(void) {\n  printf("%zu\\n", sizeof(lg_inputs_t));\n' + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.LGInputs)
    assert out[1:] == [getattr(_lib.LGInputs, f).offset for f in fields]
    z = _lib.LGInputs()  # a zeroed struct means "every slot full"
    assert not z.num_keypoints0 and not z.num_keypoints1


def _cpu_inputs(b=2, m=8, n=6):
    g = torch.Generator().manual_seed(0)
    return {"keypoints0": torch.rand(b, m, 2, generator=g), "keypoints1": torch.rand(b, n, 2, generator=g),
            "descriptors0": torch.rand(b, m, 256, generator=g), "descriptors1": torch.rand(b, n, 256, generator=g)}


@pytest.mark.parametrize("nk0,nk1,err", [
    (torch.tensor([8.0, 4.0]), torch.tensor([6, 3]), "integer dtype"),
    (torch.tensor([8, 4]), torch.tensor([True, False]), "integer dtype"),
    (torch.tensor([8, 4, 2]), torch.tensor([6, 3]), "shape"),
    (torch.tensor([[8, 4]]), torch.tensor([6, 3]), "shape"),
    (torch.tensor(8), torch.tensor([6, 3]), "shape"),
    (torch.tensor([8, 4]), None, "together"),
    (None, [6, 3], "together"),
])
def test_bad_counts_raise_value_error_before_any_device_work(nk0, nk1, err):
    from lightglue_amd import LightGlue

    model = LightGlue({}).eval()
    data = _cpu_inputs()
    if nk0 is not None:
        data["num_keypoints0"] = nk0
    if nk1 is not None:
        data["num_keypoints1"] = nk1
    # the inputs are on the CPU: the device check (a RuntimeError) would come next
    with pytest.raises(ValueError, match=err):
        model(data)
    data["num_keypoints0"], data["num_keypoints1"] = [8, 4], np.array([6, 3], np.int16)  # lists / numpy are fine
    with pytest.raises(RuntimeError, match="HIP"):
        model(data)


def test_counts_in_training_mode_with_gradients_are_not_implemented():
    from lightglue_amd import LightGlue

    model = LightGlue({}).train()
    data = dict(_cpu_inputs(), num_keypoints0=torch.tensor([8, 4]), num_keypoints1=torch.tensor([6, 3]))
    with pytest.raises(NotImplementedError, match="training"):
        model(data)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP"):  # without gradients: the eval kernels
        model(data)


def test_parallel_slice_carries_the_counts():
    from lightglue_amd.parallel import _slice

    data = dict(_cpu_inputs(b=4), num_keypoints0=torch.tensor([8, 4, 2, 1]), num_keypoints1=torch.tensor([6, 3, 2, 1]))
    part = _slice(data, 1, 3)
    assert part["num_keypoints0"].tolist() == [4, 2] and part["num_keypoints1"].tolist() == [3, 2]
    assert part["keypoints0"].shape[0] == 2


def test_export_writes_the_counts_per_pair():
    """export_predictions carries num_keypoints0/1 like any [B] tensor: one scalar per pair, not
    rescaled (only keys that START with "keypoints" are divided by the view's scales)."""
    from lightglue_amd import export

    class Echo(torch.nn.Module):
        def forward(self, data):
            return {"keypoints0": data["keypoints0"], "num_keypoints0": data["num_keypoints0"],
                    "num_keypoints1": data["num_keypoints1"]}

    batch = dict(_cpu_inputs(b=2), num_keypoints0=torch.tensor([8, 4], dtype=torch.int32),
                 num_keypoints1=torch.tensor([6, 3], dtype=torch.int32), name=["a/0", "a/1"],
                 view0={"scales": torch.full((2, 2), 2.0)}, view1={"scales": torch.full((2, 2), 2.0)})
    w = export.MemoryWriter()
    export.export_predictions([batch], Echo(), writer=w, device="cpu")
    assert [int(w.groups[n]["num_keypoints0"]) for n in ("a/0", "a/1")] == [8, 4]
    assert [int(w.groups[n]["num_keypoints1"]) for n in ("a/0", "a/1")] == [6, 3]
    np.testing.assert_allclose(w.groups["a/1"]["keypoints0"], batch["keypoints0"][1].numpy() / 2.0)


@pytest.mark.parametrize("name", sorted(ru.CASES))
def test_oracle_facts_of_the_ragged_cases(name):
    """What test_gpu_ragged.py asserts without near-tie exclusions: every pair's smallest row /
    column top-1 / top-2 margin of the log assignment is far above the 1e-4 near-tie bar, no
    score sits within 1e-4 of the filter threshold, and every pair has matches."""
    smallest = float("inf")
    for b, (n0, n1) in enumerate(ru.CASES[name][1]):
        ref = ru.oracle_pair(name, b)
        la = ref["log_assignment"][0]
        assert la.shape == (n0 + 1, n1 + 1)
        smallest = min(smallest, ru.top2_margin(la[:-1, :-1]))
        assert (ref["matches0"] > -1).sum() > 0, (name, b)
        assert np.abs(ref["matching_scores0"] - ru.CONF["filter_threshold"]).min() > 1e-4, (name, b)
    print(f"{name}: smallest top-1/top-2 margin {smallest:.3e}")
    assert smallest >= 1e-3
