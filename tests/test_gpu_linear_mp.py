"""The single-product fp16 GEMM (gemm_h3.hip H1, `mp: true`) in isolation, through `lg_linear` with
LG_PREC_GEMM_F16, against float64 -- needs an MI355X.

Every case of linear_cases.CASES runs under every launch shape the LG_GEMM_TILE / LG_GEMM_KSPLIT overrides
reach (256-, 128- and 64-row tiles, the latter with the k-tiles split over 1, 2 and 4 waves; LayerNorm +
GELU fused at 128 and 64 rows and as GEMM + row kernel), as in test_gpu_linear.py, and is held to both
bars of mp_ref.py over the live rows:
  loose  float64 of the unrounded operands; product bar 2^-10 (1 + 2^-12) S + sub + 2^-23 |ref|
  tight  float64 of the operands' decoded high pieces; linear_ref's fp16x3 bars unchanged
Sentinels in dead rows and unrequested outputs stay intact (test_gpu_linear.outputs), and the reported
range exponents equal the host rule.  test_mp_host.py shows the CPU emulation below half of both bars
and that five deliberate mistakes miss them.

Measured on an MI355X when the tests were added, worst err / bar over a case's outputs.  Columns: 256-row
tile | 128-row | 64-row k-split 1 | k-split 2 | k-split 4.  Against the loose bar the five agree to the
printed digits (the error is the operands' rounding, which no launch shape changes), so one figure is given;
the tight figures show the accumulation order.
  case                                   loose   tight
  store_plain                            0.13    0.21 0.21 0.21 0.14 0.09
  store_ffn3                             0.08    0.20 0.20 0.20 0.13 0.10
  store_planes_only                      0.12    0.16 0.16 0.16 0.14 0.14
  store_relu_res                         0.11    0.18 0.18 0.18 0.14 0.10
  cat_k[256|512]                         0.09    0.19 0.19 0.19 0.12 0.08
  cat_k[96|256]                          0.14    0.18 0.18 0.18 0.14 0.12
  single_ktile[32]                       0.31    0.16 0.16 0.16 0.16 0.16
  single_ktile[64]                       0.27    0.22 0.22 0.22 0.15 0.15
  row_mask                               0.09    0.19 0.19 0.19 0.12 0.10
  row_mask_sel                           0.08    0.19 0.19 0.19 0.11 0.10
  qkv_rot                                0.14    0.16 0.16 0.16 0.15 0.12
  qkv_plain                              0.14    0.19 0.19 0.19 0.15 0.14
  qkv_rot_big                            0.12    0.16 0.16 0.16 0.13 0.13
  qkv_rot_small_v                        0.01    0.23 0.23 0.23 0.23 0.23
  cross_qkv                              0.13    0.15 0.15 0.15 0.14 0.11
  cross_qkv_planes                       0.13    0.15 0.15 0.15 0.12 0.11
  cat_k_exponents[256|512,3e5,5e6]       0.12    0.17 0.17 0.17 0.17 0.13
  cat_k_exponents[256|512,3e5,1]         0.14    0.42 0.42 0.42 0.22 0.14
  cat_k_exponents[256|512,1,3e5]         0.13    0.20 0.20 0.20 0.20 0.11
  cat_k_exponents[96|256,3e5,5e6]        0.15    0.20 0.20 0.20 0.20 0.15
  cat_k_exponents[96|256,3e5,1]          0.21    0.35 0.35 0.35 0.24 0.23
  cat_k_exponents[96|256,1,3e5]          0.17    0.19 0.19 0.19 0.16 0.15
  ln_gelu, ln_gelu_mask (fused 128 rows | fused 64 rows | GEMM + row kernel): loose 0.02 0.02 0.02, tight 0.05 0.05 0.05
The tight figures equal test_gpu_linear.py's fp16x3 figures in kind (0.1 to 0.4 of the same bars): with the
operands rounded as the kernel rounds them, what is left is the fp32 accumulation.
"""
import pytest

import lgamd  # noqa: F401
import linear_cases as lc
import linear_ref as lr
import mp_ref as mp
import test_gpu_linear as tl
from lightglue_amd import _lib

pytestmark = pytest.mark.gpu


def check_case(name, ln_route=0):
    case, t, _, _ = mp.prepared(name)
    rc, a, b, x6 = tl.run_linear(case, t, "auto", ln_route, override={"precision": _lib.PREC_GEMM_F16})
    _lib.check(rc, "lg_linear")
    exps = {"a0": a.exp_a0, "a1": a.exp_a1, "out": a.exp_out, "out_v": a.exp_out_v}
    loose, tight, _ = mp.check(name, tl.outputs(case, a, b, x6), exps)
    print(f"LINEAR-MP {name} route={ln_route} loose " + " ".join(f"{k}={v:.3f}" for k, v in loose.items()) +
          " tight " + " ".join(f"{k}={v:.3f}" for k, v in tight.items()) + f" exps={exps}")
    e0 = lr.range_exponent(t["A0"].abs().max().item())
    e1 = lr.range_exponent(t["A1"].abs().max().item()) if t["A1"] is not None else e0
    assert (a.exp_a0, a.exp_a1) == (e0, e1), f"A exponents {exps} != {(e0, e1)}"
    _, host_exps = mp.emulate(case, t)
    assert (a.exp_out, a.exp_out_v) == (host_exps["out"], host_exps["out_v"]), f"output exponents {exps} != {host_exps}"
    if name.startswith("cat_k_exponents"):
        assert e0 != e1 and a.exp_out > 0
    assert max(loose.values()) <= 1.0, f"{name}: {loose} of the loose bar"
    assert max(tight.values()) <= 1.0, f"{name}: {tight} of the tight bar"


@pytest.mark.parametrize("tile,ksplit", lc.STORE_LAUNCHES)
@pytest.mark.parametrize("name", tl.STORE_NAMES)
def test_fp16_gemm_matches_float64(name, tile, ksplit, monkeypatch):
    monkeypatch.setenv("LG_GEMM_TILE", tile)
    if ksplit is None:
        monkeypatch.delenv("LG_GEMM_KSPLIT", raising=False)
    else:
        monkeypatch.setenv("LG_GEMM_KSPLIT", ksplit)
    check_case(name)


@pytest.mark.parametrize("tile,route", lc.LN_LAUNCHES)
@pytest.mark.parametrize("name", tl.LN_NAMES)
def test_fp16_gemm_layernorm_gelu_matches_float64(name, tile, route, monkeypatch):
    monkeypatch.setenv("LG_GEMM_TILE", tile)
    monkeypatch.delenv("LG_GEMM_KSPLIT", raising=False)
    check_case(name, route)


def test_flag_with_bf16x6_is_bad_precision():
    case, t, _, _ = mp.prepared("store_plain")
    rc, _, b, _ = tl.run_linear(case, t, "auto", override={"precision": _lib.PREC_GEMM_F16 | 1})
    assert rc == _lib.LG_E_INVALID and b"bad precision" in _lib.load().lg_last_error()
    tl._untouched(b)
