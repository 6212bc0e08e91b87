"""``flash: true`` without a GPU: the flag's plumbing from the config key to the C struct, the
`lg_create` rejections (checked before the device is touched), and the CPU emulations of
flash_ref.py against float64 -- including the near-tie cap of the model-level GPU test
(test_gpu_flash_forward.py), which is a property of the emulations and the chosen seed alone."""
import ctypes

import pytest
import torch

import flash_ref as fr
import lgamd  # noqa: F401
from lightglue_amd import LightGlue, _lib
from test_gpu_attention import CASES, case

LG_E_INVALID = -1


def test_flag_constant_and_abi_version():
    assert _lib.PREC_ATTN_F16 == 0x100
    assert _lib.PRECISIONS == {"auto": 0, "bf16x6": 1}
    assert _lib.load().lg_abi_version() == 12
    assert ctypes.sizeof(_lib.LGConfig) == 56  # lg_config_t did not grow (5 int32, pad, 3 double, int32, pad)


@pytest.mark.parametrize("precision", [1 | 0x100, 2, 0x200, 0x100 | 0x2, -1])
def test_lg_create_rejects_bad_precision_without_a_device(precision):
    lib = _lib.load()
    cfg = LightGlue({})._lib_config()
    cfg.precision = precision
    h = ctypes.c_void_p()
    rc = lib.lg_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    assert rc == LG_E_INVALID and not h.value
    assert b"precision" in lib.lg_last_error()


def test_flash_with_bf16x6_raises_naming_both_keys():
    with pytest.raises(ValueError) as e:
        LightGlue({"flash": True, "precision": "bf16x6"})
    assert "flash" in str(e.value) and "precision" in str(e.value)


def test_flash_sets_the_flag_in_the_config_struct():
    assert LightGlue({"flash": True})._lib_config().precision == _lib.PREC_ATTN_F16
    assert LightGlue({"flash": False})._lib_config().precision == 0
    assert LightGlue({})._lib_config().precision == 0
    assert LightGlue({"precision": "bf16x6"})._lib_config().precision == 1


def test_pipeline_and_pretrained_wrapper_pass_the_key_through():
    from lightglue_amd.pipeline import TwoViewPipeline

    pipe = TwoViewPipeline({"matcher": {"name": "matchers.lightglue", "flash": True}})
    assert pipe.matcher._lib_config().precision == _lib.PREC_ATTN_F16


@pytest.mark.parametrize("name", CASES)
def test_emulations_satisfy_the_hard_cap(name):
    q, k, v, scale = case(name)
    ref = fr.ref64(q, k, v, scale)
    cap = fr.hard_cap(q, k, v, scale)
    for emu in (fr.emu_upstream, fr.emu_tiled):
        err = (emu(q, k, v, scale) - ref).abs().max().item()
        print(f"{name}/{emu.__name__}: max |d| = {err:.3e}, cap {cap:.3e}")
        assert err <= cap, (name, emu.__name__, err, cap)


def test_emulations_really_round():
    q, k, v, scale = case("random_ragged")
    ref = fr.ref64(q, k, v, scale)
    for emu in (fr.emu_upstream, fr.emu_tiled):
        assert (emu(q, k, v, scale) - ref).abs().max().item() > 1e-5, emu.__name__


def test_near_tie_cap_holds_for_the_model_case():
    """The rows test_gpu_flash_forward.py leaves out of its match comparison (F1 / F2 disagree, or
    F1's top-1 / top-2 margin below 4 d_la) are at most 5 % of all rows, on the CPU emulations
    alone; the flash oracles differ from the fp32 oracle (they really round) and keep matching."""
    _, _, A, F1, F2 = fr.model_case()
    d_s, d_la = fr.spreads(F1, F2)
    tie0, tie1 = fr.near_tie_masks(F1, F2)
    share = (tie0.sum().item() + tie1.sum().item()) / (tie0.numel() + tie1.numel())
    print(f"d_s = {d_s:.3e}, d_la = {d_la:.3e}, excluded rows {share:.4f}")
    assert share <= fr.NEAR_TIE_CAP
    fin = torch.isfinite(A["log_assignment"])
    assert (F1["log_assignment"][fin] - A["log_assignment"][fin]).abs().max().item() > 1e-5
    assert (F1["matches0"] > -1).sum().item() > 100
