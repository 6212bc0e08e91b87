"""The SuperPoint convolution kernels (sp_conv1a_kernel, sp_conv3x3_halo_kernel, sp_conv3x3_kernel) and the
two dense-head kernels in isolation, through the C-ABI entries `sp_conv_layer`, `sp_head_scores` and
`sp_head_normalize`, against float64 -- needs an MI355X.

The forward goldens see the convolutions only through seven to eight layers, two 1x1 GEMMs and a softmax
or an L2 normalisation, with bars two to three orders of magnitude above the kernels' own error.  Here
every case of sp_conv_cases.CASES runs under both routes (LG_SP_CONV unset = halo tiles, `gather` = the
per-tap row gather), so a failure names the kernel, the template instantiation (BN from Cout, POOL, AFF)
and the shape.  The seam cases take their batch size from the device's CU count so that a workgroup of
the persistent halo kernel walks at least three tiles (asserted with the kernel's own formula).
Bars (sp_conv_ref; none is taken from the kernel): per element against float64
  d = 2^-21 S + 2^-23 |c|, S = conv2d(|x|, |w|) + |bias|; through the affine |s| d + 2^-23 (|s relu(c)| + |y|);
  through the pool the window's largest bar; + 2^-22 |ref| + 2^(E-35) for the plane image;
  conv1a: 13 * 2^-24 (sum |w| |gray| + |bias|) instead of d.
test_sp_conv_host.py shows a CPU emulation of the kernels' arithmetic stays below half of every bar and
that seven deliberate mistakes miss them.

Structure checked with every case: the output planes are pre-filled with a sentinel and the call is
made twice with two different sentinels.  A half that the kernel writes holds the same bits after both
calls (the call is deterministic: this is the bit-identity assertion), a half it does not write holds
each call's sentinel: so every half of the live rows [0, rout) must agree between the calls and every
half of the rows [rout, yrows_pad) must hold the sentinels.  The workspace is handed over filled with
0xFF bytes (fp16 NaNs): nothing stale may reach a result.

Measured on an MI355X (256 CUs: the seam cases ran with B = 37, 37 and 19, max T = 3) when the tests were
added: worst err / bar per case, halo route then gather route, then the exponents E[in] / E[out] the two
images were written with (the same under both routes).  With one channel block (Cin = 32) the two routes
accumulate the k-steps in the same order and agree to the printed digits.
  b1_1x1_32to64                    0.100 0.100  -13/0     b1_2x2_32to64                    0.109 0.109  -13/0
  b1_2x2_32to64+pool               0.105 0.105  -13/0     b2_17x33_64to64                  0.251 0.249  -12/0
  b2_17x33_64to64+pool             0.283 0.301  -12/0     b1_19x21_64to128                 0.313 0.271  -12/0
  b1_19x21_64to128+pool            0.265 0.224  -12/0     b3_16x16_32to64                  0.243 0.243  -12/0
  b3_16x16_32to64+pool             0.249 0.249  -12/0     b1_24x40_32to192                 0.341 0.341  -12/0
  b1_24x40_32to192+pool            0.309 0.309  -12/0     b1_24x40_128to256                0.337 0.292  -12/0
  b1_24x40_128to256+pool           0.338 0.301  -12/0     b1_24x40_64to128                 0.288 0.283  -12/0
  b1_24x40_64to128+pool            0.319 0.286  -12/0     b1_24x40_128to512                0.304 0.330  -12/0
  b1_24x40_128to512+pool           0.328 0.307  -12/0     b2_17x33_64to64_aff_mixed        0.294 0.307  -12/0
  b2_17x33_64to64_aff_mixed+pool   0.284 0.270  -12/0     b1_19x21_64to128_aff_mixed       0.267 0.244  -12/0
  b1_19x21_64to128_aff_mixed+pool  0.208 0.192  -12/0     b2_17x33_64to64_aff_neg          0.281 0.263  -12/0
  b2_17x33_64to64_aff_neg+pool     0.118 0.150  -12/0     b1_19x21_64to128_aff_neg         0.267 0.254  -12/0
  b1_19x21_64to128_aff_neg+pool    0.128 0.096  -12/0     b2_17x33_64to64_aff_zeros        0.281 0.281  -12/0
  b2_17x33_64to64_aff_zeros+pool   0.311 0.255  -12/0     b1_19x21_64to128_aff_zeros       0.309 0.309  -12/0
  b1_19x21_64to128_aff_zeros+pool  0.340 0.336  -13/0     b2_17x33_64to64_aff_wide         0.431 0.431  -12/2
  b2_17x33_64to64_aff_wide+pool    0.411 0.411  -12/2     b1_19x21_64to128_aff_wide        0.455 0.455  -12/2
  b1_19x21_64to128_aff_wide+pool   0.345 0.345  -12/2     b2_17x33_64to64_x3e5             0.247 0.241    6/10
  b2_17x33_64to64_x3e5+pool        0.225 0.257    6/10    b2_17x33_64to64_x1e-6            0.447 0.447  -32/0
  b2_17x33_64to64_x1e-6+pool       0.420 0.416  -32/0     b2_17x33_64to64_allzero          0.000 0.000  -12/0
  b2_17x33_64to64_allzero+pool     0.000 0.000  -12/0     b2_17x33_64to64_wchan1e4         0.291 0.341  -12/5
  b2_17x33_64to64_wchan1e4+pool    0.272 0.253  -12/5     seam_32to64                      0.389 0.389  -12/0
  seam_32to64+pool                 0.339 0.339  -12/0     seam_32to64_aff                  0.354 0.354  -12/0
  seam_32to128                     0.411 0.411  -12/0     seam_32to128+pool                0.375 0.375  -12/0
  seam_64to256_aff+pool            0.395 0.362  -12/0
  conv1a (C, then B_HxW or the 0 / 1 / 255 image; E[out] = 0):
    c1_b1_1x1 0.124, c1_b1_1x1_aff 0.278, c1_b2_17x33 0.223, c1_b2_17x33_aff 0.423, c1_b1_40x56 0.320, c1_b1_40x56_aff 0.396, c1_0_1_255 0.265,
    c3_b1_1x1 0.115, c3_b1_1x1_aff 0.198, c3_b2_17x33 0.216, c3_b2_17x33_aff 0.356, c3_b1_40x56 0.206, c3_b1_40x56_aff 0.387, c3_0_1_255 0.322
  dense heads: scores 1x1 0.487, 3x5 0.498, 9x7 0.492; normalize 0.206 (norms of the unit-scale rows 0.999999945 .. 1.000000047)
Nothing is above half a bar.  The largest, 0.455 on the scales spanning 1e-3 to 1e3 and 0.447 on the inputs
at 1e-6, are the plane image's absolute quantum and not the product: one exponent serves the whole image
(E[out] = 2 and 0), so the outputs of the channels scaled by 1e-3, and every output of the 1e-6 case,
have subnormal fp16 low pieces and are stored to 2^(E-36), half of the bar's 2^(E-35) term.  The CPU
emulation of test_sp_conv_host.py gives the same five figures to the printed digits.  The softmax sits at
0.49-0.50: its bar is dominated by the argument term |x - max| 2^-24 (up to 160 for logits spanning +-80),
the rounding of the one subtraction that an fp32 softmax cannot avoid, and so is its error.
"""
import ctypes
import functools
import os

import pytest
import torch

import lgamd  # noqa: F401
import linear_ref as lr
import sp_conv_cases as sc
import sp_conv_ref as sr
from lightglue_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -123.456  # fp32 sentinel of y_rows
SENT16 = (0x5A5A, 0x2B2B)  # plane sentinels of the two calls (fp16 211.25 and 0.0558: finite)
ROUTES = ("halo", "gather")
_results = {}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def prepared(name):
    c = sc.case(name, cus())
    t = sc.build_inputs(c)
    return c, t, sr.reference(c, t)


@functools.lru_cache(maxsize=None)
def _base_exp_in():
    """The input exponent of b2_17x33_64to64, which the scaled-input cases are compared with."""
    return lr.range_exponent(sc.build_inputs(sc.case("b2_17x33_64to64"))["x"].abs().max().item(), two_sided=True)


def _ptr(x):
    return None if x is None else x.data_ptr()


def call_layer(c, t, sent16=SENT16[0], ws_short=0, drop_shift=False):
    """One sp_conv_layer call on pre-filled outputs -> (rc, buffers)."""
    lib = _lib.load()
    d = {k: (v.cuda() if v is not None else None) for k, v in t.items()}
    Cout = c["Cout"]
    rout, rpy = ctypes.c_int64(), ctypes.c_int32()
    _lib.check(lib.sp_conv_layer_rows(c["B"], c["H"], c["W"], c["pool"], ctypes.byref(rout), ctypes.byref(rpy)), "rows")
    b = {"rout": rout.value, "rpy": rpy.value}
    b["y_rows"] = torch.full((max(rout.value, 1), Cout), SENT, device="cuda")
    b["planes"] = torch.full((2, rpy.value * Cout), sent16, dtype=torch.int16, device="cuda")
    e_in, e_out, m_out = ctypes.c_int32(-999), ctypes.c_int32(-999), ctypes.c_float(-1.0)
    a = _lib.SPConvLayerArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.pool, a.conv1a = c["B"], c["H"], c["W"], c["Cin"], Cout, c["pool"], c["conv1a"]
    a.x, a.w, a.bias = _ptr(d["x"]), _ptr(d["w"]), _ptr(d["bias"])
    a.post_scale, a.post_shift = _ptr(d["s"]), (None if drop_shift else _ptr(d["t"]))
    a.y_rows, a.y_planes = _ptr(b["y_rows"]), _ptr(b["planes"])
    a.exp_in, a.exp_out, a.max_out = ctypes.pointer(e_in), ctypes.pointer(e_out), ctypes.pointer(m_out)
    nbytes = ctypes.c_size_t(4096)
    rc = lib.sp_conv_layer_workspace_bytes(c["B"], c["H"], c["W"], c["Cin"], Cout, c["pool"], c["conv1a"], ctypes.byref(nbytes))
    if rc != _lib.LG_OK:  # an invalid shape: sp_conv_layer itself must refuse it too
        nbytes.value = 1 << 20
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    b["ws_rc"] = rc
    rc = lib.sp_conv_layer(ctypes.byref(a), ws.data_ptr(), nbytes.value - ws_short, stream)
    torch.cuda.synchronize()
    b.update(exp_in=e_in.value, exp_out=e_out.value, max_out=m_out.value, _keep=(d, ws))
    return rc, b


def _plane_values(b, Cout):
    """The raw halves of both planes as [2][yrows_pad][Cout] (int16), on the host."""
    rpy = b["rpy"]
    rows = torch.arange(rpy)[:, None].expand(rpy, Cout)
    off = lr.plane_off(rows, torch.arange(Cout)[None, :].expand(rpy, Cout), rpy)
    raw = b["planes"].cpu()
    return torch.stack([raw[0][off], raw[1][off]])


def run_case(name, route):
    """Two calls with different sentinels -> (y_rows fp32 on the host, exps); the structural assertions."""
    assert os.environ.get("LG_SP_CONV", "halo") == route
    key = (name, route)
    if key in _results:
        return _results[key]
    c, t, ref = prepared(name)
    Cout = c["Cout"]
    rc0, b0 = call_layer(c, t, SENT16[0])
    _lib.check(rc0, "sp_conv_layer")
    rc1, b1 = call_layer(c, t, SENT16[1])
    _lib.check(rc1, "sp_conv_layer")
    rout = b0["rout"]
    p0, p1 = _plane_values(b0, Cout), _plane_values(b1, Cout)
    for p in range(2):
        assert (p0[p][rout:] == SENT16[0]).all() and (p1[p][rout:] == SENT16[1]).all(), f"plane {p}: a row past rout was written"
        same = p0[p][:rout] == p1[p][:rout]
        if not same.all():
            r, ch = (~same).nonzero()[0].tolist()
            left = p0[p][r, ch].item() == SENT16[0] and p1[p][r, ch].item() == SENT16[1]
            raise AssertionError(f"plane {p}, row {r}, channel {ch}: " + ("never written" if left else "differs between two calls"))
    y0, y1 = b0["y_rows"].cpu()[:rout], b1["y_rows"].cpu()[:rout]
    assert torch.equal(y0, y1) and (b0["exp_in"], b0["exp_out"], b0["max_out"]) == (b1["exp_in"], b1["exp_out"], b1["max_out"])
    # y_rows is the plane image decoded with the committed exponent
    dec = (p0[0][:rout].view(torch.float16).double() + p0[1][:rout].view(torch.float16).double() * 2.0 ** -11) * 2.0 ** b0["exp_out"]
    assert torch.allclose(y0.double(), dec, rtol=2.0 ** -23, atol=0.0)
    # the recorded max|y| is taken before the split: the image's largest value is its plane rounding away
    assert abs(b0["max_out"] - y0.abs().max().item()) <= 2.0 ** -22 * b0["max_out"] + 2.0 ** (b0["exp_out"] - 35)
    _results[key] = (y0, {"in": b0["exp_in"], "out": b0["exp_out"]})
    return _results[key]


def _set_route(monkeypatch, route):
    if route == "gather":
        monkeypatch.setenv("LG_SP_CONV", "gather")
    else:
        monkeypatch.delenv("LG_SP_CONV", raising=False)


# ---------------------------------------------------------------- the 3x3 convolutions
@pytest.mark.parametrize("name", sc.CONV_NAMES)
@pytest.mark.parametrize("route", ROUTES)
def test_conv3x3(route, name, monkeypatch):
    _set_route(monkeypatch, route)
    c, t, ref = prepared(name)
    BN, num_n, ntiles = sc.halo_tiles(c)
    if c["seam"]:
        assert ntiles > 2 * cus() + 64 and max(sc.tile_counts(ntiles, cus())) >= 3
    got, e = run_case(name, route)
    r = sr.check(ref, got, e["out"])
    T = max(sc.tile_counts(ntiles, cus()))
    print(f"SPCONV {name} {route} BN={BN} POOL={c['pool']} AFF={int(c['aff'] is not None)} B={c['B']} T={T} "
          f"err/bar={r:.3f} exps={e}")
    assert e["in"] == lr.range_exponent(t["x"].abs().max().item(), two_sided=True)
    base = _base_exp_in()
    if "_x3e5" in name:  # log2(3e5) = 18.2
        assert e["in"] - base in (18, 19) and e["out"] > 0
    if "_x1e-6" in name:  # log2(1e-6) = -19.9
        assert e["in"] - base in (-20, -19) and e["out"] == 0
    if "_wchan1e4" in name:
        assert e["out"] > 0
    if "_allzero" in name:
        assert (ref["y"] == 0).all() and (got == 0).all() and e["out"] == 0, "every output is exactly 0 behind the ReLU"
    assert r <= 1.0, f"{name}/{route}: {r:.3f} of the bar"


@pytest.mark.parametrize("name", sc.CONV_NAMES)
def test_routes_agree(name, monkeypatch):
    """halo and gather within the sum of their bars (not bit for bit: the k-steps run in another order)."""
    c, t, ref = prepared(name)
    out = {}
    for route in ROUTES:
        _set_route(monkeypatch, route)
        out[route] = run_case(name, route)
    (yh, eh), (yg, eg) = out["halo"], out["gather"]
    assert eh == eg
    diff = (yh.double() - yg.double()).abs()
    assert (diff <= 2 * sr.bars(ref, eh["out"])).all()


# ---------------------------------------------------------------- conv1a
@pytest.mark.parametrize("name", sc.CONV1A_NAMES)
def test_conv1a(name, monkeypatch):
    _set_route(monkeypatch, "halo")
    c, t, ref = prepared(name)
    got, e = run_case(name, "halo")
    r = sr.check(ref, got, e["out"])
    print(f"SPCONV {name} AFF={int(c['aff'] is not None)} err/bar={r:.3f} exps={e}")
    assert e["in"] == 0
    assert r <= 1.0, f"{name}: {r:.3f} of the bar"


# ---------------------------------------------------------------- invalid arguments
def _untouched(b):
    return (b["y_rows"].cpu() == torch.tensor(SENT)).all() and (b["planes"].cpu() == SENT16[0]).all() and b["exp_out"] == -999


@pytest.mark.parametrize("what", ["Cin48", "Cout96", "pool_H1", "ws_short", "scale_without_shift"])
def test_invalid_arguments_launch_nothing(what):
    c = dict(sc.case("b2_17x33_64to64_aff_mixed"))
    kw = {}
    if what == "Cin48":
        c["Cin"] = 48
    elif what == "Cout96":
        c["Cout"] = 96
    elif what == "pool_H1":
        c.update(H=1, pool=1)
    elif what == "ws_short":
        kw["ws_short"] = 1
    else:
        kw["drop_shift"] = True
    c["name"] = "invalid_" + what
    rc, b = call_layer(c, sc.build_inputs(c), **kw)
    assert rc == (_lib.LG_E_WORKSPACE if what == "ws_short" else _lib.LG_E_INVALID), rc
    assert b["ws_rc"] == (_lib.LG_E_INVALID if what in ("Cin48", "Cout96", "pool_H1") else _lib.LG_OK)
    assert _untouched(b), "an invalid call wrote an output"


# ---------------------------------------------------------------- the dense heads
@pytest.mark.parametrize("Hc,Wc", [(1, 1), (3, 5), (9, 7)])
def test_detector_scores(Hc, Wc):
    lib = _lib.load()
    B, ld = 2, 80
    g = torch.Generator().manual_seed(100 * Hc + Wc)
    cells = B * Hc * Wc
    logits = torch.full((cells, ld), 1e30)  # columns past 65 are never read
    logits[:, :65] = (torch.rand(cells, 65, generator=g) * 2 - 1) * 80.0
    logits[cells // 2, 64] = logits[cells // 2, :64].max() + 100.0  # a dustbin that dominates by 100
    ref, bar = sr.scores_reference(logits, B, Hc, Wc)
    dl = logits.cuda()
    out = torch.full((B, 8 * Hc, 8 * Wc), SENT, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.sp_head_scores(dl.data_ptr(), ld, B, Hc, Wc, out.data_ptr(), stream), "sp_head_scores")
    torch.cuda.synchronize()
    got = out.cpu().double()
    r = ((got - ref).abs() / bar).max().item()
    print(f"SPHEAD scores {Hc}x{Wc} err/bar={r:.3f}")
    assert r <= 1.0
    # the unfold permutation, exactly: one-hot logits give exactly 1 at one pixel of each cell
    hot = torch.full((cells, ld), -1e4)
    ch = (torch.arange(cells) * 7 + 3) % 64
    hot[torch.arange(cells), ch] = 0.0
    want, _ = sr.scores_reference(hot, B, Hc, Wc)
    dl = hot.cuda()
    _lib.check(lib.sp_head_scores(dl.data_ptr(), ld, B, Hc, Wc, out.data_ptr(), stream), "sp_head_scores")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), want) and want.sum() == cells


def test_desc_normalize():
    lib = _lib.load()
    g = torch.Generator().manual_seed(7)
    x = torch.cat([(torch.rand(8, 256, generator=g) * 2 - 1) * m for m in (1e-20, 1.0, 1e18)] + [torch.zeros(1, 256)]).float()
    ref, bar = sr.normalize_reference(x)
    dx = x.cuda()
    out = torch.full((x.shape[0] + 1, 256), SENT, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.sp_head_normalize(dx.data_ptr(), x.shape[0], out.data_ptr(), stream), "sp_head_normalize")
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[-1] == torch.tensor(SENT)).all(), "a row past `rows` was written"
    got = got[:-1].double()
    assert (got[-1] == 0).all(), "the all-zero row: 0 / 1e-12"
    r = ((got - ref).abs() / bar).max().item()
    norms = got[8:24].norm(dim=-1)
    print(f"SPHEAD normalize err/bar={r:.3f} unit norms {norms.min().item():.9f}..{norms.max().item():.9f}")
    assert r <= 1.0
