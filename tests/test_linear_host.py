"""CPU self-checks of the kernel-level linear tests (no GPU): the bars of linear_ref.py are reachable
by the kernels' arithmetic, they notice deliberate mistakes, every case still takes the kernel
instantiation it was written for, and the packed projection order is head_perm's."""
import functools
import os
import subprocess

import pytest
import torch

import lgamd  # noqa: F401
import linear_cases as lc
import linear_ref as lr
from lightglue_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in lc.CASES]


@functools.lru_cache(maxsize=None)
def prepared(name):
    case = lc.BY_NAME[name]
    t = lc.build_inputs(case)
    return case, t, lr.reference(case, t)


def worst(case, t, ref, **kw):
    out, exps = lr.emulate(case, t, **kw)
    return max(lr.check(case, t, ref, out, exps).values()), exps


# ---------------------------------------------------------------- 1. the bars are reachable
@pytest.mark.parametrize("fmt", ["h3", "x6"])
@pytest.mark.parametrize("name", NAMES)
def test_emulation_meets_the_bars(name, fmt):
    case, t, ref = prepared(name)
    for ks in ((1, 4) if fmt == "h3" and case["epi"] == "store" else (1,)):
        w, _ = worst(case, t, ref, fmt=fmt, ksplit=ks)
        assert w <= 0.5, f"{name}/{fmt}/ksplit {ks}: emulation at {w:.3f} of the bar"


def test_emulated_exponents_are_what_the_cases_claim():
    for name in NAMES:
        case, t, ref = prepared(name)
        _, e = lr.emulate(case, t, fmt="h3")
        if name.startswith("cat_k_exponents"):
            assert e["a0"] != e["a1"] and max(e["a0"], e["a1"]) > 0 and e["out"] > 0, (name, e)
            assert (e["a0"] > 0) == (case["a0_scale"] > 1) and (e["a1"] > 0) == (case["a1_scale"] > 1), (name, e)
        elif name == "qkv_rot_big":
            assert e["a0"] > 0 and e["out"] > 0 and e["out_v"] > 0, e
        elif name in ("qkv_rot", "qkv_rot_small_v"):
            assert e["out"] == 0 and e["out_v"] < (-10 if name == "qkv_rot_small_v" else 0), e
        elif case["epi"] in ("store", "ln_gelu"):
            assert e["a0"] == e["a1"] == e["out"] == 0, (name, e)


def test_ln_rows_are_what_the_case_claims():
    case, t, ref = prepared("ln_gelu")
    pre = torch.cat([t["A0"], t["A1"]], 1).double() @ t["W"].double().T + t["bias"].double()
    assert 2e-7 < pre[7].var(unbiased=False).item() < 5e-6  # below eps = 1e-5: eps decides the scale
    assert abs(pre[93, 100].item() - 1e4) < 1.0 and pre[93].abs().median().item() < 1e3


# ---------------------------------------------------------------- 2. the bars notice mistakes
SENSITIVITY = {
    "drop_low_high": [("store_plain", 1)],
    # in-loop under split-k, after-loop under split-k, in-loop without a split
    "no_seam_rescale": [(f"cat_k_exponents[96|256,{3e5:g},{5e6:g}]", 4), (f"cat_k_exponents[256|512,{3e5:g},1]", 4),
                        (f"cat_k_exponents[256|512,1,{3e5:g}]", 1)],
    "bias_neighbour_block": [("store_plain", 1), ("qkv_rot", 1)],
    "res_not_res2": [("store_ffn3", 1)],
    "no_eps": [("ln_gelu", 1)],
    "rotary_sign": [("qkv_rot", 1)],
}


@pytest.mark.parametrize("wrong", lr.WRONG)
def test_bars_notice_a_wrong_kernel(wrong):
    """Each wrong variant of the emulation misses the bar on every case listed for it."""
    assert set(SENSITIVITY) == set(lr.WRONG)
    for name, ks in SENSITIVITY[wrong]:
        case, t, ref = prepared(name)
        w, _ = worst(case, t, ref, fmt="h3", ksplit=ks, wrong=wrong)
        assert w > 1.0, f"{wrong} on {name}: {w:.3f} of the bar -- the suite would not notice"


# ---------------------------------------------------------------- 3. routes
def test_cases_reach_their_routes():
    p = lc.parsed()
    for c in lc.CASES:
        R, K0, K, Nout, name = c["R"], c["K0"], c["K"], c["Nout"], c["name"]
        assert R <= 600 and K <= 512 and Nout <= 768
        if c["epi"] == "ln_gelu":
            assert lc.ln_route(p, R, "big") == (128, False)
            assert lc.ln_route(p, R, "small") == (64, True)
            assert lc.ln_route(p, R) == (64, True)  # what the forward takes at this size: the split route
            assert c["mask"] or (R % 128 and R % 64), "partial last tile under both fused shapes"
        # the override matrix reaches five distinct instantiations whenever K allows
        got = {(tile, ks): lc.store_route(p, R, K, Nout, tile, ks) for tile, ks in lc.STORE_LAUNCHES}
        assert got[("big", None)] == (256, 1) and got[("medium", None)] == (128, 1)
        want_ks = {"1": 1, "2": 2 if K >= 64 else 1, "4": 4 if K >= 128 else 2 if K >= 64 else 1}
        for req, ks in want_ks.items():
            assert got[("small", req)] == (64, ks), (name, req)
        assert lc.store_route(p, R, K, Nout) == got[("small", "4")], f"{name}: the unforced route is no longer the small tile"
        if c["epi"] == "store" and not c["mask"]:
            assert R % 256 and R % 128 and R % 64, f"{name}: no partial last tile"
    # single k-tile: prologue only; K = 64 falls back to 2
    assert all(lc.store_route(p, 300, 32, 256, "small", r) == (64, 1) for r in "124")
    assert lc.store_route(p, 300, 64, 256, "small", "4") == (64, 2)
    # the seam under KSPLIT = 4: inside a group (in-loop rescale on a non-empty accumulator) for
    # K0 = 96, on a group boundary with A0-only groups before it (after-loop rescale) for K0 = 256
    groups, nk0 = lc.ksplit_groups(p, 96, 256, 4)
    assert groups[1] == (2, 4) and nk0 == 3 and any(kb < nk0 < ke for kb, ke in groups)
    assert any(ke <= nk0 for kb, ke in groups)
    groups, nk0 = lc.ksplit_groups(p, 256, 512, 4)
    assert nk0 == 8 and not any(kb < nk0 < ke for kb, ke in groups) and sum(ke <= nk0 for kb, ke in groups) == 2
    # the row mask: segment 1 (rows 160 .. 319) holds whole dead 64-row tiles; segment 2's tile is live
    live = lc.live_rows(lc.BY_NAME["row_mask"])
    tiles = live.view(-1, 64).any(1)
    assert (~tiles).sum() >= 2 and tiles[320 // 64] and live[320:325].all() and not live[325:448].any()
    assert int(live.sum()) == 160 + 5 + 128
    frozen = lc.live_rows(lc.BY_NAME["row_mask_sel"])
    assert int(frozen.sum()) == 160 + 5 and not frozen[160:320].any() and not frozen[448:].any()
    # ffn3: the res2 / Y2 switch is no multiple of a store group, an MFMA tile or a wave tile
    r0 = lc.BY_NAME["store_ffn3"]["res2_row0"]
    assert r0 % 8 and r0 % 32 and r0 % 64


# ---------------------------------------------------------------- 4. packed order
def test_packed_order_is_head_perm():
    """lightglue_api.cpp head_perm, H = 4: p[t*256 + h*64 + j] = h*192 + dim(j)*3 + t (Wqkv) and
    p[768 + h*64 + j] = h*64 + dim(j) (to_qk / to_v), dim(j) = 2j (j < 32), 2(j-32)+1 (j >= 32)."""
    dim = lambda j: 2 * j if j < 32 else 2 * (j - 32) + 1  # noqa: E731
    p = lc.packed_order("qkv_rot").tolist()
    assert sorted(p) == list(range(768))
    for t in range(3):
        for h in range(4):
            for j in range(64):
                assert p[t * 256 + h * 64 + j] == h * 192 + dim(j) * 3 + t
    assert p[0] == 0 and p[1] == 6 and p[32] == 3 and p[256] == 1 and p[64] == 192
    pc = lc.packed_order("cross_qkv").tolist()
    assert sorted(pc) == list(range(512))
    for t in range(2):
        for h in range(4):
            for j in range(64):
                assert pc[t * 256 + h * 64 + j] == t * 256 + h * 64 + dim(j)
    # the kernel's own statement of the order (gemm_h3.hip QKV epilogue) still reads that way
    lc._one(r"const int dim = c < 32 \? 2 \* c : 2 \* \(c - 32\) \+ 1;", lc._src("gemm_h3.hip"), "QKV dim order")
    # and _packed_to_natural inverts it
    x = torch.arange(768.0).repeat(2, 1)
    nat = lr._packed_to_natural(x, 3)
    assert nat[0, 1, 2, 5].item() == 1 * 256 + 2 * 64 + 32 + 2 and nat[0, 0, 0, 4].item() == 2


# ---------------------------------------------------------------- 5. the binding
def test_linear_args_struct_matches_the_header(tmp_path):
    hdr = os.path.join(ROOT, "include", "lightglue_mi355x.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{hdr}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(lg_linear_args_t));']
    lines += [f'printf("{f} %zu\\n", offsetof(lg_linear_args_t, {f}));' for f, _ in _lib.LGLinearArgs._fields_]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got.pop("size")) == __import__("ctypes").sizeof(_lib.LGLinearArgs)
    for f, _ in _lib.LGLinearArgs._fields_:
        assert int(got[f]) == getattr(_lib.LGLinearArgs, f).offset, f
    assert {"lg_linear", "lg_linear_workspace_bytes", "lg_plane_roundtrip"} <= set(_lib.EXPORTED_SYMBOLS)
    assert _lib.load().lg_abi_version() == 12  # additive: the ABI version does not move


def test_range_exponent_rule():
    assert lr.range_exponent(2.0 ** 15) == 0 and lr.range_exponent(float(torch.nextafter(torch.tensor(2.0 ** 15), torch.tensor(1e9)))) == 1
    assert lr.range_exponent(16.0, lshift=11) == 0 and lr.range_exponent(16.000002, lshift=11) == 1
    e = lr.range_exponent(1e-3, two_sided=True)
    assert e < 0 and 2.0 ** 14 < 1e-3 * 2.0 ** -e <= 2.0 ** 15
    assert lr.range_exponent(0.0, two_sided=True) == 0 and lr.range_exponent(0.0) == 0
