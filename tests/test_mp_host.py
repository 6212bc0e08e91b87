"""``mp: true`` without a GPU: the key's way from the config to the C struct, the `lg_create` rejections
(checked before the device is touched), and the CPU emulation of the single-product fp16 GEMM (mp_ref.py)
against both of its references -- including the cap on the rows the model-level GPU test
(test_gpu_mp_forward.py) leaves out, which is a property of the CPU oracles and the chosen seed alone."""
import ctypes

import pytest
import torch

import flash_ref as fr
import lgamd  # noqa: F401
import linear_cases as lc
import mp_ref as mp
from lightglue_amd import LightGlue, _lib

LG_E_INVALID = -1
NAMES = [c["name"] for c in lc.CASES]


# ---------------------------------------------------------------- plumbing (fail without the feature)
def test_flag_constants():
    assert _lib.PREC_GEMM_F16 == 0x400
    assert _lib.PRECISION_NAMES[0x400] == "fp16gemm" and _lib.PRECISION_NAMES[0x500] == "fp16gemm+fp16attn"
    assert _lib.PRECISIONS == {"auto": 0, "bf16x6": 1}


def test_mp_sets_both_flags_in_the_config_struct():
    assert LightGlue({"mp": True})._lib_config().precision == 0x500
    assert LightGlue({"mp": True, "flash": True})._lib_config().precision == 0x500
    assert LightGlue({"mp": False})._lib_config().precision == 0
    assert LightGlue({"flash": True})._lib_config().precision == 0x100


def test_pipeline_passes_the_key_through():
    from lightglue_amd.pipeline import TwoViewPipeline

    pipe = TwoViewPipeline({"matcher": {"name": "matchers.lightglue", "mp": True}})
    assert pipe.matcher._lib_config().precision == 0x500


def test_mp_with_bf16x6_raises_naming_both_keys():
    with pytest.raises(ValueError) as e:
        LightGlue({"mp": True, "precision": "bf16x6"})
    assert '"mp"' in str(e.value) and '"precision"' in str(e.value)


@pytest.mark.parametrize("precision", [0x401, 0x501, 0x600])
def test_lg_create_rejects_bad_flag_combinations_without_a_device(precision):
    lib = _lib.load()
    cfg = LightGlue({})._lib_config()
    cfg.precision = precision
    h = ctypes.c_void_p()
    rc = lib.lg_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    assert rc == LG_E_INVALID and not h.value
    assert b"precision" in lib.lg_last_error()


def test_lg_linear_rejects_the_flag_with_bf16x6():
    """Argument checks come before the device is touched: 0x401 is "bad precision", 0x400 passes that check
    (and then fails on the null workspace)."""
    lib = _lib.load()
    x = torch.zeros(64, 32)
    w = torch.zeros(256, 32)
    y = torch.zeros(64, 256)
    a = _lib.LGLinearArgs()
    a.R, a.K0, a.K, a.Nout = 64, 32, 32, 256
    a.A0, a.lda0, a.W, a.Y, a.ldy = x.data_ptr(), 32, w.data_ptr(), y.data_ptr(), 256
    a.out_scale, a.epi = 1.0, _lib.LIN_EPI["store"]
    a.precision = 0x401
    assert lib.lg_linear(ctypes.byref(a), None, 0, None) == LG_E_INVALID
    assert b"bad precision" in lib.lg_last_error()
    a.precision = _lib.PREC_GEMM_F16
    assert lib.lg_linear(ctypes.byref(a), None, 0, None) == _lib.LG_E_WORKSPACE


# ---------------------------------------------------------------- the emulation against both bars
def _ksplits(case):
    return [ks for ks in (1, 2, 4) if ks == 1 or case["K"] >= ks * 32]


@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_below_half_of_both_bars(name):
    case, t, _, _ = mp.prepared(name)
    for ks in _ksplits(case):
        out, exps = mp.emulate(case, t, ksplit=ks)
        loose, tight, h3 = mp.check(name, out, exps)
        print(f"MP-EMU {name} ksplit={ks} loose " + " ".join(f"{k}={v:.3f}" for k, v in loose.items()) +
              " tight " + " ".join(f"{k}={v:.3f}" for k, v in tight.items()) + f" fp16x3-bar {max(h3.values()):.0f}")
        assert max(loose.values()) <= 0.5, (name, ks, loose)
        assert max(tight.values()) <= 0.5, (name, ks, tight)


# which case shows which mistake (every case runs the first two)
MISTAKES = [("keep_2^-11", "store_plain"), ("keep_2^-11", "qkv_rot"), ("low_plane", "store_plain"),
            ("low_plane", "ln_gelu"), ("no_seam_rescale", "cat_k_exponents[256|512,300000,1]"),
            ("no_seam_rescale", "cat_k_exponents[96|256,300000,5e+06]"), ("bias_neighbour_block", "store_plain"),
            ("bias_neighbour_block", "cross_qkv"), ("res_not_res2", "store_ffn3")]


@pytest.mark.parametrize("wrong,name", MISTAKES)
def test_deliberate_mistakes_miss_both_bars(wrong, name):
    assert wrong in mp.WRONG
    case, t, _, _ = mp.prepared(name)
    out, exps = mp.emulate(case, t, wrong=wrong)
    loose, tight, _ = mp.check(name, out, exps)
    print(f"MP-WRONG {wrong} {name}: loose {max(loose.values()):.3g}, tight {max(tight.values()):.3g}")
    assert max(loose.values()) > 1.0 and max(tight.values()) > 1.0


@pytest.mark.parametrize("name", ["store_plain", "cat_k[256|512]", "qkv_rot", "cross_qkv"])
def test_emulation_really_rounds(name):
    """Against the unrounded reference the H1 error is far above the fp16x3 bar."""
    case, t, _, _ = mp.prepared(name)
    out, exps = mp.emulate(case, t)
    _, _, h3 = mp.check(name, out, exps)
    assert max(h3.values()) > 10.0, h3


# ---------------------------------------------------------------- the model-level oracles
def test_excluded_row_cap_holds_for_the_model_case():
    """The rows test_gpu_mp_forward.py leaves out (F1 != F2, margin below 2 d_m, score within 2 d_s of the
    threshold) are at most 10 % of all rows; the oracles really round and keep matching."""
    _, _, A, F1, F2 = mp.model_case()
    d_s, d_m = mp.spreads(F1, F2)
    x0, x1 = mp.excluded_masks(F1, F2, fr.MODEL_CONF["filter_threshold"])
    share = mp.excluded_share(x0, x1)
    differ = (F1["matches0"] != F2["matches0"]).sum().item() + (F1["matches1"] != F2["matches1"]).sum().item()
    print(f"d_s = {d_s:.3e}, d_m = {d_m:.3e}, F1 != F2 on {differ} rows, excluded rows {share:.4f}")
    assert share <= mp.EXCLUDED_CAP
    fin = torch.isfinite(A["log_assignment"])
    for F in (F1, F2):
        assert (F["log_assignment"][fin] - A["log_assignment"][fin]).abs().max().item() > 1e-4
        assert (F["matches0"] > -1).sum().item() > 100
