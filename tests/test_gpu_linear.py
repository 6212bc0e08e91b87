"""The inference linear GEMMs (gemm_h3: fp16x3 plane images, gemm_x6: bf16x6) and their epilogues in
isolation, through the C-ABI entry `lg_linear`, against float64 -- needs an MI355X.

The forward goldens see these kernels only through 9 to 18 layers, with bars two orders of magnitude
above the kernels' own error.  Here every case of linear_cases.CASES runs in both operand formats and,
for fp16x3, under every launch shape the LG_GEMM_TILE / LG_GEMM_KSPLIT overrides reach (256-, 128- and
64-row tiles, the latter with the k-tiles split over 1, 2 and 4 waves; LayerNorm + GELU fused at 128
and 64 rows and as GEMM + row kernel), so a failure names the kernel, the epilogue and the tile shape.
Bars (linear_ref.bars; none is taken from the kernel): per element against float64,
  2^-21 S + 2^-23 |ref|,  S = sum_k |a w| + |bias| (times |out_scale|, plus |res|)
-- 2^-21 is the worst-case fp16x3 operand error (the dropped x_l y_l term 2^-22, two 2^-23 piece
roundings), about twice what DESIGN.md §3 records as measured -- plus 2^-22 |ref| + 2^(E-35) for
plane outputs (2^(E-25) for value planes), 2^-22 (|x_e| + |x_o|) for rotated pairs, and for
LayerNorm + GELU the first-order propagation 2.26 d_r |g| (1 + |z|) / sigma of the row's product bar
d_r plus twice the spread of the same LayerNorm + GELU in plain fp32.  test_linear_host.py shows a CPU
emulation of the kernels' arithmetic stays below half of every bar and that six deliberate mistakes
miss them.

Measured on an MI355X when the tests were added, worst err / bar over a case's outputs.  fp16x3 columns:
256-row tile | 128-row | 64-row k-split 1 | k-split 2 | k-split 4 (the first three accumulate the
k-tiles in the same order and agree to the printed digits); last column bf16x6.
  store_plain          0.32 0.32 0.32 0.22 0.13 | 0.42      store_ffn3         0.28 0.28 0.28 0.16 0.12 | 0.44
  store_planes_only    0.27 0.27 0.27 0.18 0.12 | 0.37      store_relu_res     0.25 0.25 0.25 0.23 0.11 | 0.32
  cat_k[256|512]       0.33 0.33 0.33 0.20 0.13 | 0.52      cat_k[96|256]      0.32 0.32 0.32 0.20 0.13 | 0.41
  single_ktile[32]     0.23 0.23 0.23 0.23 0.23 | 0.33      single_ktile[64]   0.32 0.32 0.32 0.18 0.18 | 0.36
  row_mask             0.31 0.31 0.31 0.20 0.12 | 0.44      row_mask_sel       0.31 0.31 0.31 0.20 0.12 | 0.44
  qkv_rot              0.26 0.26 0.26 0.20 0.15 | 0.36      qkv_plain          0.30 0.30 0.30 0.20 0.15 | 0.41
  qkv_rot_big          0.28 0.28 0.28 0.19 0.13 | 0.35      qkv_rot_small_v    0.22 0.22 0.22 0.22 0.22 | 0.18
  cross_qkv            0.34 0.34 0.34 0.17 0.14 | 0.45      cross_qkv_planes   0.34 0.34 0.34 0.17 0.14 | 0.41
  cat_k_exponents[256|512]: (3e5, 5e6) 0.27 0.27 0.27 0.28 0.19 | 0.45   (3e5, 1) 0.42 0.42 0.42 0.31 0.22 | 0.54
                            (1, 3e5)   0.30 0.30 0.30 0.32 0.17 | 0.48
  cat_k_exponents[96|256]:  (3e5, 5e6) 0.28 0.28 0.28 0.28 0.16 | 0.42   (3e5, 1) 0.43 0.43 0.43 0.34 0.27 | 0.46
                            (1, 3e5)   0.31 0.31 0.31 0.26 0.18 | 0.39
  ln_gelu: fused 128 rows 0.04, fused 64 rows 0.04, GEMM + row kernel 0.03 | 0.06;  ln_gelu_mask 0.06 0.06 0.04 | 0.07
  exponents seen: E[a] = 6 / 10 for inputs at 3e5 / 5e6, E[out] = 10 / 14; qkv: E[v] = -9 (-14 with inputs
  at 1e-6), qkv_rot_big E[a] = 6, E[k] = E[v] = 10.
Above half a bar: bf16x6 on cat_k[256|512] (0.52) and cat_k_exponents[256|512, 3e5, 1] (0.54).  That is the
format, not these cases: DESIGN.md §3 records bf16x6's own maximum over random operands as 3.1e-7 S =
0.65 * 2^-21 S, and these are the K = 512 cases, whose fp32 accumulation over 32 k-steps of six products
adds the most rounding.  The bars stay as derived above.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import linear_cases as lc
import linear_ref as lr
from lightglue_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -123.456  # fp32 sentinel; planes: 0x5A5A (fp16 211.25, bf16 ~1.5e13: finite in both)
SENT16 = 0x5A5A
NAMES = [c["name"] for c in lc.CASES]


@functools.lru_cache(maxsize=None)
def prepared(name):
    case = lc.BY_NAME[name]
    t = lc.build_inputs(case)
    return case, t, lr.reference(case, t)


def _dev(x, dtype=None):
    return None if x is None else torch.as_tensor(x, dtype=dtype).contiguous().cuda()


def _ptr(x):
    return None if x is None else x.data_ptr()


def run_linear(case, t, precision, ln_route=0, override=None, ws_short=0):
    """One lg_linear call on pre-filled outputs.  Returns (rc, args, buffers)."""
    lib = _lib.load()
    R, K0, K, Nout = case["R"], case["K0"], case["K"], case["Nout"]
    RP = (R + 255) // 256 * 256
    x6 = precision == "bf16x6"
    d = {k: _dev(t.get(k)) for k in ("A0", "A1", "W", "bias", "res", "res2", "ln_g", "ln_b", "cos", "sin")}
    b = {}
    a = _lib.LGLinearArgs()
    a.R, a.K0, a.K, a.Nout = R, K0, K, Nout
    a.A0, a.lda0, a.A1, a.lda1 = _ptr(d["A0"]), K0, _ptr(d["A1"]), K - K0
    a.W, a.bias = _ptr(d["W"]), _ptr(d["bias"])
    a.res, a.res2, a.res2_row0, a.ldr = _ptr(d["res"]), _ptr(d["res2"]), case["res2_row0"] or 0, Nout
    a.out_scale, a.relu = case["out_scale"], case["relu"]
    a.precision, a.epi, a.ln_route = _lib.PRECISIONS[precision], _lib.LIN_EPI[case["epi"]], ln_route
    a.ln_g, a.ln_b = _ptr(d["ln_g"]), _ptr(d["ln_b"])
    if case["head"]:
        a.B, a.M, a.N = case["head"]
        a.H = 4
        a.cosb, a.sinb, a.qk_scale = _ptr(d["cos"]), _ptr(d["sin"]), case["qk_scale"]
        b["q"] = torch.full((R * 256,), SENT, device="cuda") if (case["q_given"] or case["epi"] == "qkv_rot") else None
        b["kp"] = torch.full((3, R * 256), SENT16, dtype=torch.int16, device="cuda")
        b["vp"] = torch.full((3, R * 256), SENT16, dtype=torch.int16, device="cuda")
        a.q, a.kp, a.vp, a.pstride = _ptr(b["q"]), _ptr(b["kp"]), _ptr(b["vp"]), R * 256
    m = case["mask"]
    if m:
        a.mask_B, a.mask_M0, a.mask_N0 = m["B"], m["M0"], m["N0"]
        d["cnt"], d["sel"] = _dev(m["cnt"], torch.int32), _dev(m["sel"], torch.int32)
        a.cnt, a.sel, a.sel_eq = _ptr(d["cnt"]), _ptr(d["sel"]), m["sel_eq"]
    a.poison, a.want_planes = case["poison"], int(case["planes"])
    if case["fp32"]:
        r0 = case["y2_row0"]
        b["Y"] = torch.full((R, Nout), SENT, device="cuda")
        a.Y, a.ldy = _ptr(b["Y"]), Nout
        if r0 is not None:  # Y2: an allocation of its own, 130 rows of neighbour behind it
            b["Y2"] = torch.full((R - r0 + 130, Nout), SENT, device="cuda")
            a.Y2, a.y2_row0 = _ptr(b["Y2"]), r0
    if case["planes"]:
        b["yp"] = torch.full((2, RP * Nout), SENT16, dtype=torch.int16, device="cuda")
        b["yp_rows"] = torch.full((R, Nout), SENT, device="cuda")
        a.yp, a.yp_rows = _ptr(b["yp"]), _ptr(b["yp_rows"])
    for k, v in (override or {}).items():
        setattr(a, k, v)
    nbytes = ctypes.c_size_t()
    _lib.check(lib.lg_linear_workspace_bytes(R, K0, K, Nout, ctypes.byref(nbytes)), "lg_linear_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.lg_linear(ctypes.byref(a), ws.data_ptr(), nbytes.value - ws_short, stream)
    torch.cuda.synchronize()
    b["_keep"] = (d, ws)
    return rc, a, b, x6


def _planes(buf, x6, E, values=False):
    """Decode raw operand planes on the host: fp16 h + l 2^-11 (values: h + l), bf16 h + m + l; times 2^E."""
    raw = buf.cpu()
    if x6:
        p = raw.view(torch.bfloat16).double()
        return p[0] + p[1] + p[2]
    p = raw.view(torch.float16).double()
    return (p[0] + p[1] * (1.0 if values else 2.0 ** -11)) * 2.0 ** E


def outputs(case, a, b, x6):
    """The call's results as linear_ref.check takes them, after the untouched-memory assertions."""
    R, Nout = case["R"], case["Nout"]
    live = lc.live_rows(case)
    dead = ~live
    sent = torch.tensor(SENT)
    out = {}
    if "Y" in b:
        Y = b["Y"].cpu()
        r0 = case["y2_row0"]
        if r0 is not None:
            Y2 = b["Y2"].cpu()
            assert (Y[r0:] == sent).all(), "Y written at or after y2_row0"
            assert (Y2[R - r0:] == sent).all(), "Y2's neighbour written"
            Y = torch.cat([Y[:r0], Y2[:R - r0]])
        assert (Y[dead] == sent).all(), "a dead row of Y / Y2 was written"
        out["y"] = Y
    if "yp" in b:
        raw = b["yp"].cpu()
        if x6:
            assert (raw == SENT16).all(), "bf16x6 has no plane image"
            if case["epi"] != "ln_gelu":  # the LayerNorm + GELU row kernel has no mask
                assert (b["yp_rows"].cpu()[dead] == sent).all(), "a dead row was written"
        else:
            RP = raw.shape[1] // Nout
            written = torch.zeros(RP, dtype=torch.bool)
            written[:R] = live if not (case["epi"] == "ln_gelu" and a.ln_route == 1) else True  # the row kernel has no mask
            rows = torch.arange(RP)[:, None].expand(RP, Nout)
            off = lr.plane_off(rows, torch.arange(Nout)[None, :].expand(RP, Nout), RP)
            for p in range(2):
                vals = raw[p][off]  # [RP][Nout]
                assert (vals[~written] == SENT16).all(), f"plane {p}: a dead or padding row was written"
                assert not (vals[written] == SENT16).all(1).any(), f"plane {p}: a live row was not written"
        out["yp"] = b["yp_rows"].cpu()
    if case["head"]:
        B, M, N = case["head"]
        if b["q"] is not None:
            out["q"] = lr.from_head_major(b["q"].cpu(), B, M, N)
        out["k"] = lr.from_head_major(_planes(b["kp"], x6, a.exp_out), B, M, N)
        out["v"] = lr.from_head_major(_planes(b["vp"], x6, a.exp_out_v, values=True), B, M, N)
        if not x6:
            assert (b["kp"].cpu()[2] == SENT16).all() and (b["vp"].cpu()[2] == SENT16).all()
    return out


def check_case(name, precision, ln_route=0):
    case, t, ref = prepared(name)
    rc, a, b, x6 = run_linear(case, t, precision, ln_route)
    _lib.check(rc, "lg_linear")
    exps = {"a0": a.exp_a0, "a1": a.exp_a1, "out": a.exp_out, "out_v": a.exp_out_v}
    ratios = lr.check(case, t, ref, outputs(case, a, b, x6), exps)
    print(f"LINEAR {name} {precision} route={ln_route} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()) + f" exps={exps}")
    if x6:
        assert set(exps.values()) == {0}
    else:  # the path the case was written for really ran
        e0 = lr.range_exponent(t["A0"].abs().max().item())
        e1 = lr.range_exponent(t["A1"].abs().max().item()) if t["A1"] is not None else e0
        assert (a.exp_a0, a.exp_a1) == (e0, e1), f"A exponents {exps} != {(e0, e1)}"
        if name.startswith("cat_k_exponents"):
            assert e0 != e1 and a.exp_out > 0
        if name == "qkv_rot_big":
            assert a.exp_out > 0 and a.exp_out_v > 0
        if name in ("qkv_rot", "qkv_rot_small_v"):
            assert a.exp_out_v < 0
        if case["epi"] == "ln_gelu":
            assert abs(a.bound_out - ref["ln_bound"]) <= 1e-5 * ref["ln_bound"]
            assert np.isfinite(a.max_out) and 0 < a.max_out <= a.bound_out, "M[out] outside the LayerNorm bound"
    worst = max(ratios.values())
    assert worst <= 1.0, f"{name}/{precision}: {ratios} of the bar"


STORE_NAMES = [n for n in NAMES if lc.BY_NAME[n]["epi"] != "ln_gelu"]
LN_NAMES = [n for n in NAMES if lc.BY_NAME[n]["epi"] == "ln_gelu"]


@pytest.mark.parametrize("tile,ksplit", lc.STORE_LAUNCHES)
@pytest.mark.parametrize("name", STORE_NAMES)
def test_fp16x3_matches_float64(name, tile, ksplit, monkeypatch):
    monkeypatch.setenv("LG_GEMM_TILE", tile)
    if ksplit is None:
        monkeypatch.delenv("LG_GEMM_KSPLIT", raising=False)
    else:
        monkeypatch.setenv("LG_GEMM_KSPLIT", ksplit)
    check_case(name, "auto")


@pytest.mark.parametrize("tile,route", lc.LN_LAUNCHES)
@pytest.mark.parametrize("name", LN_NAMES)
def test_fp16x3_layernorm_gelu_matches_float64(name, tile, route, monkeypatch):
    """Fused at 128 rows (big), fused at 64 rows (small), and the 64 x 64-tile GEMM + row kernel; each
    against float64, not against each other."""
    monkeypatch.setenv("LG_GEMM_TILE", tile)
    monkeypatch.delenv("LG_GEMM_KSPLIT", raising=False)
    check_case(name, "auto", route)


@pytest.mark.parametrize("name", NAMES)
def test_bf16x6_matches_float64(name):
    check_case(name, "bf16x6")


# ---------------------------------------------------------------- range edges
def roundtrip(x, lshift, two_sided):
    lib = _lib.load()
    xd = x.contiguous().cuda()
    out = torch.full_like(xd, SENT)
    E = ctypes.c_int32(99)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.lg_plane_roundtrip(xd.data_ptr(), x.shape[0], x.shape[1], lshift, int(two_sided), out.data_ptr(),
                                      ctypes.byref(E), stream), "lg_plane_roundtrip")
    return out.cpu(), E.value


def _up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


@pytest.mark.parametrize("peak,lshift,two_sided,want", [
    (2.0 ** 15, 0, False, 0), (_up(2.0 ** 15), 0, False, 1), (16.0, 11, False, 0), (_up(16.0), 11, False, 1),
    (1e-3, 0, True, None), (0.0, 0, False, 0), (0.0, 0, True, 0)])
def test_range_edges(peak, lshift, two_sided, want):
    """rows_to_planes -> image_to_rows: the exponent at the 2^15 (2^4 for "y" operands) edge, the
    two-sided rule, all-zero input; the decoded rows equal the input to the 22-bit split."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(70, 64, generator=g)
    x = x / x.abs().max() * (0.9 * peak)
    x[3, 5], x[69, 63] = peak, -peak
    assert x.abs().max().item() == float(np.float32(peak))
    got, E = roundtrip(x, lshift, two_sided)
    if want is None:  # two-sided: the bound lands in (lim / 2, lim]
        assert E < 0 and 2.0 ** 14 < float(np.float32(peak)) * 2.0 ** -E <= 2.0 ** 15
    else:
        assert E == want
    assert E == lr.range_exponent(peak, lshift, two_sided)
    err = (got.double() - x.double()).abs()
    assert (err <= 2.0 ** -22 * x.double().abs() + 2.0 ** (E - 35)).all(), err.max().item()


# ---------------------------------------------------------------- argument errors
def _untouched(b):
    for k in ("Y", "yp_rows", "q"):
        if b.get(k) is not None:
            assert (b[k].cpu() == torch.tensor(SENT)).all(), f"{k} written by a refused call"
    for k in ("yp", "kp", "vp"):
        if b.get(k) is not None:
            assert (b[k].cpu() == SENT16).all(), f"{k} written by a refused call"


@pytest.mark.parametrize("precision", ["auto", "bf16x6"])
@pytest.mark.parametrize("what,name,override,ws_short,code", [
    ("Nout = 128", "store_plain", {"Nout": 128}, 0, _lib.LG_E_INVALID),
    ("K = 40", "store_plain", {"K": 40, "K0": 40}, 0, _lib.LG_E_INVALID),
    ("K0 > K", "store_plain", {"K0": 288}, 0, _lib.LG_E_INVALID),
    ("A1 null with K0 < K", "cat_k[256|512]", {"A1": None}, 0, _lib.LG_E_INVALID),
    ("ln_gelu with Nout != 512", "ln_gelu", {"Nout": 256}, 0, _lib.LG_E_INVALID),
    ("workspace one byte short", "store_ffn3", {}, 1, _lib.LG_E_WORKSPACE)])
def test_linear_errors(what, name, override, ws_short, code, precision):
    case, t, _ = prepared(name)
    rc, a, b, _ = run_linear(case, t, precision, override=override, ws_short=ws_short)
    assert rc == code, f"{what}: rc = {rc}"
    _untouched(b)
    lib = _lib.load()
    n = ctypes.c_size_t()
    if what in ("Nout = 128", "K = 40", "K0 > K"):  # the shape rules are the workspace function's too
        assert lib.lg_linear_workspace_bytes(a.R, a.K0, a.K, a.Nout, ctypes.byref(n)) == _lib.LG_E_INVALID
