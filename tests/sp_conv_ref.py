"""Float64 reference, error bars and a CPU emulation for the kernel-level SuperPoint convolution tests.

reference(c, t)   conv2d(padding 1) + bias, ReLU, the optional affine and max_pool2d(2) in float64 torch
                  from the same fp32 inputs, with the per-element bar (none taken from the kernel):
    product   d = 2^-21 S + 2^-23 |c|,  S = conv2d(|x|, |w|) + |bias|,  c the pre-activation
              (2^-21: the dropped x_l w_l term 2^-22 plus two 2^-23 piece roundings, as linear_ref.bars)
    ReLU      1-Lipschitz: carries d unchanged
    affine    |s| d + 2^-23 (|s relu(c)| + |y|)       (one fp32 fma on a value already off by d)
    pool      the maximum of the window's four bars (max is 1-Lipschitz in the sup norm; the kernel's
              min-pool of the accumulators under a negative scale computes the same function)
    conv1a    fp32 FMA arithmetic: d = n 2^-24 (sum |w| G + |bias|) with n = 13 and G the gray image's
              magnitude 0.299 |r| + 0.587 |g| + 0.114 |b|.  n: a gray value passes through three
              rounded operations (a product and two sums; the other two products feed a sum and are
              counted with it), the nine taps are nine fmaf, each one rounding of the running sum,
              and the bias is one rounded add: every term carries at most 13 factors (1 + delta),
              |delta| <= 2^-24, so the error is at most gamma_13 ~ 13 * 2^-24 of sum |terms|.
bars(ref, E)      + 2^-22 |ref| + 2^(E-35) for the plane image (E: the committed output exponent)
emulate(c, t)     the fp16x3 arithmetic of sp_conv3x3_halo_kernel / sp_conv3x3_kernel in torch: the
                  two-sided input exponent, hi / lo pieces of x 2^-E and of w 2^sw, the three products
                  per (channel block, tap) step accumulated in fp32, the epilogue, the output split;
                  with `wrong=...` one of WRONG's deliberate mistakes.
Rows are NHWC: [B * Ho * Wo][Cout].
"""
import torch
import torch.nn.functional as F

from linear_ref import f32, range_exponent, split2h, weight_shift

D = torch.float64
N_CONV1A = 13
GRAY = (0.299, 0.587, 0.114)
SENT_VALUE = 211.25 + 211.25 / 2048.0  # what a plane pair left at 0x5A5A decodes to (times 2^E)
WRONG = ["drop_low_in", "wrap_rows", "tile_border_tap", "swap_cblocks", "maxpool_neg_scale", "partial_tile_unwritten",
         "bias_after_affine"]


def _rows(y):
    """[B][C][H][W] -> [B*H*W][C]"""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def _gray64(img):
    """(gray, magnitude) of an fp32 image [B][C][H][W] in float64, the fp32 constants widened."""
    x = img.double()
    if x.shape[1] == 1:
        return x, x.abs()
    k = [float(torch.tensor(v, dtype=torch.float32)) for v in GRAY]
    return (sum(k[i] * x[:, i:i + 1] for i in range(3)), sum(k[i] * x[:, i:i + 1].abs() for i in range(3)))


def reference(c, t):
    w, b = t["w"].double(), t["bias"].double()[None, :, None, None]
    if c["conv1a"]:
        x, mag = _gray64(t["x"])
        pre = F.conv2d(x, w, padding=1) + b
        d = N_CONV1A * 2.0 ** -24 * (F.conv2d(mag, w.abs(), padding=1) + b.abs())
    else:
        x = t["x"].double().permute(0, 3, 1, 2)
        pre = F.conv2d(x, w, padding=1) + b
        d = 2.0 ** -21 * (F.conv2d(x.abs(), w.abs(), padding=1) + b.abs()) + 2.0 ** -23 * pre.abs()
    y = pre.clamp_min(0)
    if t["s"] is not None:
        s, sh = t["s"].double()[None, :, None, None], t["t"].double()[None, :, None, None]
        r, y = y, y * s + sh
        d = s.abs() * d + 2.0 ** -23 * ((s * r).abs() + y.abs())
    if c["pool"]:
        y, d = F.max_pool2d(y, 2), F.max_pool2d(d, 2)
    return {"y": _rows(y).contiguous(), "bar": _rows(d).contiguous()}


def bars(ref, E):
    return ref["bar"] + 2.0 ** -22 * ref["y"].abs() + 2.0 ** (E - 35)


def check(ref, got, E):
    """max err / bar; every compared value must be finite."""
    e = (got.double() - ref["y"]).abs()
    assert torch.isfinite(e).all(), "non-finite output"
    return (e / bars(ref, E)).max().item() if e.numel() else 0.0


# ---------------------------------------------------------------------------------- emulation
def _shift(x, dy, dx, wrap=False):
    """x [B][H][W][C] read at (y + dy, x + dx): zero outside the image; wrap: the flat-row neighbour."""
    B, H, W, C = x.shape
    if wrap:  # row index p + dy W + dx of the flat pixel list, zero only outside the list
        flat = x.reshape(B * H * W, C)
        idx = torch.arange(B * H * W) + dy * W + dx
        ok = (idx >= 0) & (idx < B * H * W)
        return (flat[idx.clamp(0, B * H * W - 1)] * ok[:, None]).reshape(B, H, W, C)
    out = torch.zeros_like(x)
    ys, xs_ = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
    yd, xd = slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx))
    out[:, ys, xs_] = x[:, yd, xd]
    return out


def _codec(v, E):
    h, lo = split2h(f32(v * 2.0 ** -E))
    return (h + lo * 2.0 ** -11) * 2.0 ** E


def emulate(c, t, order="halo", wrong=None):
    """(rows [rout][Cout] as decoded from the planes, {"in": E_in, "out": E_out})."""
    assert not c["conv1a"]
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    x, w = t["x"].double(), t["w"].double()
    M = t["x"].abs().max().item()
    e_in = range_exponent(M, two_sided=True)
    wrep = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)  # k = (3 ky + kx) Cin + ci
    sw = weight_shift(wrep)
    wh, wl = split2h(wrep * 2.0 ** sw)
    xh, xl = split2h(f32(x * 2.0 ** -e_in))
    if wrong == "swap_cblocks":
        perm = torch.arange(Cin)
        perm[:32], perm[32:64] = torch.arange(32, 64), torch.arange(32)
        xh, xl = xh[..., perm], xl[..., perm]
    CB = Cin // 32
    steps = [(cb, tap) for cb in range(CB) for tap in range(9)] if order == "halo" else \
            [(cb, tap) for tap in range(9) for cb in range(CB)]
    acc = torch.zeros(B * H * W, Cout, dtype=D)
    border = (torch.arange(W) % 16 == 15)[None, None, :, None]
    for cb, tap in steps:
        ky, kx = tap // 3, tap % 3
        cs = slice(cb * 32, cb * 32 + 32)
        ks = slice(tap * Cin + cb * 32, tap * Cin + cb * 32 + 32)

        def tapped(p):
            a = _shift(p[..., cs], ky - 1, kx - 1, wrap=wrong == "wrap_rows")
            if wrong == "tile_border_tap" and tap == 5:  # tap (1, 2) reads x + 2 at a tile's last column
                a = torch.where(border, _shift(p[..., cs], 0, 2), a)
            return a.reshape(B * H * W, 32)
        ah, al = tapped(xh), tapped(xl)
        if wrong != "drop_low_in":
            acc = f32(acc + al @ wh[:, ks].T)
        acc = f32(acc + ah @ wl[:, ks].T)
        acc = f32(acc + ah @ (wh[:, ks] * 2048.0).T)
    accs = 2.0 ** (-(11 + sw) + e_in)
    bias = t["bias"].double()
    aff = t["s"] is not None
    if wrong == "bias_after_affine" and aff:
        v = f32(f32(acc * accs).clamp_min(0) * t["s"].double() + t["t"].double()) + bias
    else:
        v = f32(acc * accs + bias).clamp_min(0)  # one fma
        if aff:
            v = f32(v * t["s"].double() + t["t"].double())  # one fma
    v = v.reshape(B, H, W, Cout).permute(0, 3, 1, 2)
    g = wrep.abs().sum(1).max().item()
    smax, tmax = (t["s"].abs().max().item(), t["t"].abs().max().item()) if aff else (1.0, 0.0)
    e_out = range_exponent(smax * g * M + smax * bias.abs().max().item() + tmax)
    if c["pool"]:
        pooled = F.max_pool2d(v, 2)
        if aff and wrong == "maxpool_neg_scale":  # the largest accumulator's tail: the window's minimum for s < 0
            pooled = torch.where((t["s"] < 0)[None, :, None, None], -F.max_pool2d(-v, 2), pooled)
        v = pooled
    v = _codec(v, e_out)
    if wrong == "partial_tile_unwritten":
        Ho, Wo = v.shape[2], v.shape[3]
        if H % 16:
            v[:, :, Ho - 1, :] = SENT_VALUE * 2.0 ** e_out
        if W % 16:
            v[:, :, :, Wo - 1] = SENT_VALUE * 2.0 ** e_out
    return _rows(v).contiguous(), {"in": e_in, "out": e_out}


def emulate_conv1a(c, t):
    """sp_conv1a_kernel's arithmetic: gray by rounded fp32 operations, nine fmaf, the bias add, ReLU,
    the affine as one fma, the output split."""
    img = t["x"].double()
    if c["Cin"] == 3:
        k = [float(torch.tensor(v, dtype=torch.float32)) for v in GRAY]
        g = f32(f32(f32(img[:, 0] * k[0]) + f32(img[:, 1] * k[1])) + f32(img[:, 2] * k[2]))
    else:
        g = img[:, 0]
    g = g[..., None]  # [B][H][W][1]
    w = t["w"].double().reshape(64, 9)
    a = torch.zeros(*g.shape[:3], 64, dtype=D)
    for tap in range(9):
        a = f32(_shift(g, tap // 3 - 1, tap % 3 - 1) * w[:, tap] + a)
    v = f32(a + t["bias"].double()).clamp_min(0)
    aff = t["s"] is not None
    if aff:
        v = f32(v * t["s"].double() + t["t"].double())
    smax, tmax = (t["s"].abs().max().item(), t["t"].abs().max().item()) if aff else (1.0, 0.0)
    bound = smax * w.abs().sum(1).max().item() * t["x"].abs().max().item() + smax * t["bias"].abs().max().item() + tmax
    e_out = range_exponent(bound)
    return _codec(v, e_out).reshape(-1, 64), {"in": 0, "out": e_out}


# ---------------------------------------------------------------------------------- dense heads
# fp32 softmax over 65 (sp_scores_kernel), u = 2^-24, a_j = x_j - max, got_c = fl(e_c / sum_j e_j):
#   a_j        one subtraction, relative error u: through exp an error |a_j| u of e_j
#   e_j        expf, at most 1 ulp = 2 u (the bound the HIP device library documents for expf)
#   the sum    64 additions of non-negative terms: at most 64 u on top of the terms' own errors,
#              which enter weighted by p_j: sum_j p_j (|a_j| + 2) u
#   the quotient  one correctly rounded division, u
# so k_c = (|a_c| + 2) + (sum_j p_j |a_j| + 2 + 64) + 1 = 69 + |a_c| + sum_j p_j |a_j|, which is 69 for
# the cell's largest logit and grows with the distance below it, as the error of any fp32 softmax does.
# Below fp32's smallest normal number a result may be rounded as a subnormal or flushed: 2^-126 absolute.
K_SOFTMAX = 69


def scores_reference(logits, B, Hc, Wc):
    """softmax over 65 without the dustbin, unfolded to [B][8 Hc][8 Wc], and its bar."""
    l64 = logits[:, :65].double()
    p = torch.softmax(l64, -1)
    arg = (l64 - l64.amax(-1, keepdim=True)).abs()
    k = K_SOFTMAX + arg + (p * arg).sum(-1, keepdim=True)
    bar = k * 2.0 ** -24 * p + 2.0 ** -126
    unfold = lambda a: a[:, :64].reshape(B, Hc, Wc, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, 8 * Hc, 8 * Wc)  # noqa: E731
    return unfold(p), unfold(bar)


# L2 normalisation of a row of 256 (sp_desc_norm_kernel), u = 2^-24: a lane squares and sums four values
# (each term through at most 4 roundings), the wave sum adds six levels: the sum of squares is off by
# at most 10 u, its root by 5 u, + sqrtf (1 ulp = 2 u, the documented bound) + the correctly rounded
# division (u) + the clamp constant 1e-12f against the reference's double 1e-12 (u): k = 9.
K_NORMALIZE = 9


def normalize_reference(x):
    x64 = x.double()
    y = x64 / x64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return y, K_NORMALIZE * 2.0 ** -24 * y.abs() + 2.0 ** -126
