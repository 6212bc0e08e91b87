"""Float64 references, error bars and CPU emulations for the kernel-level linear tests.

reference(case, t)      the operation in float64 torch from the same fp32 inputs, rounded nowhere
bars(case, t, ref, E)   the per-element bars of the issue (none taken from the kernel under test)
emulate(case, t, fmt)   the fp16x3 / bf16x6 arithmetic of gemm_h3.hip / gemm.hip in torch: operands split
                        into their pieces, the partial products accumulated in fp32 per k-tile in the
                        kernels' order, the documented epilogue order, the output split.  It shows the
                        bars are reachable (test_linear_host.py) and, with `wrong=...`, that the bars notice
                        each of a list of deliberate mistakes.
check(...)              max err / bar per output over the live rows
Outputs are dicts: y (fp32 rows), yp (plane image decoded), q / k / v [R][H][64] in natural dim order.
"""
import math

import numpy as np
import torch

D = torch.float64
H = 4
WRONG = ["drop_low_high", "no_seam_rescale", "bias_neighbour_block", "res_not_res2", "no_eps", "rotary_sign"]


def f32(x):
    """Round a float64 tensor to fp32 once (kept as float64)."""
    return x.float().double()


def range_exponent(b, lshift=0, two_sided=False):
    """common.h range_exponent on a bound b."""
    b = float(np.float32(b))
    lim = 2.0 ** (15 - lshift)
    if not b <= 3.0e38:
        return 0
    if two_sided:
        return max(math.frexp(b / lim)[1], -64) if b > 0 else 0
    return math.frexp(b / lim)[1] if b > lim else 0


def weight_shift(W):
    """lightglue_api.cpp's sw = 4 - E rule: max|W 2^sw| in [8, 16)."""
    mx = W.abs().max().item()
    return min(max(4 - math.frexp(mx)[1], -100), 100) if mx > 0 and math.isfinite(mx) else 0


# ---------------------------------------------------------------------------------- layouts
def plane_off(rows, cols, rows_pad):
    """common.h plane_off for index tensors: element offset of (row, k) inside one plane."""
    swz = (0x78 >> (((rows >> 2) & 3) * 2)) & 3
    return ((cols >> 5) * rows_pad + rows) * 32 + ((((cols >> 3) & 3) ^ swz) << 3) + (cols & 7)


def from_head_major(flat, B, M, N):
    """[set][b][h][n][64] -> [R][H][64], rows in GEMM order (image 0 rows first)."""
    n0 = B * H * M * 64
    a = flat[:n0].view(B, H, M, 64).permute(0, 2, 1, 3).reshape(B * M, H, 64)
    b = flat[n0:n0 + B * H * N * 64].view(B, H, N, 64).permute(0, 2, 1, 3).reshape(B * N, H, 64)
    return torch.cat([a, b])


def head_major_index(B, M, N):
    """[R][H] element offset (of dim 0) of each row / head in the head-major layout."""
    i0 = (torch.arange(B)[:, None, None] * H * M + torch.arange(H)[None, None, :] * M + torch.arange(M)[None, :, None]) * 64
    i1 = (torch.arange(B)[:, None, None] * H * N + torch.arange(H)[None, None, :] * N + torch.arange(N)[None, :, None]) * 64
    return torch.cat([i0.reshape(B * M, H), B * H * M * 64 + i1.reshape(B * N, H)])


def _packed_to_natural(x, T):
    """[R][T*256] in packed column order c' = t*256 + h*64 + j -> [R][T][H][64] by dim."""
    dims = torch.tensor([2 * j if j < 32 else 2 * (j - 32) + 1 for j in range(64)])
    out = torch.empty(x.shape[0], T, H, 64, dtype=x.dtype)
    out[..., dims] = x.view(x.shape[0], T, H, 64)
    return out


# ---------------------------------------------------------------------------------- reference
def _cat_a(t):
    return torch.cat([t["A0"], t["A1"]], 1).double() if t["A1"] is not None else t["A0"].double()


def _res_full(t):
    return (torch.cat([t["res"], t["res2"]]) if t.get("res2") is not None else t["res"]).double()


def _rotate(x, S, cos, sin):
    """lightglue.py:36-43 on [R][H][64] with [R][32] tables; S propagated as |c| S_e + |s| S_o."""
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    xe, xo, Se, So = x[..., 0::2], x[..., 1::2], S[..., 0::2], S[..., 1::2]
    y, Sy, extra = torch.empty_like(x), torch.empty_like(S), torch.empty_like(x)
    y[..., 0::2], y[..., 1::2] = xe * c - xo * s, xo * c + xe * s
    Sy[..., 0::2], Sy[..., 1::2] = Se * c.abs() + So * s.abs(), So * c.abs() + Se * s.abs()
    extra[..., 0::2] = extra[..., 1::2] = 2.0 ** -22 * (xe.abs() + xo.abs())
    return y, Sy, extra


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def reference(case, t):
    A = _cat_a(t)
    epi = case["epi"]
    if case["head"]:
        W, b = t["W_nat"].double(), t["bias_nat"].double()
    else:
        W, b = t["W"].double(), (t["bias"].double() if t["bias"] is not None else torch.zeros(case["Nout"], dtype=D))
    pre, S = A @ W.T + b, A.abs() @ W.abs().T + b.abs()
    r = {}
    if epi == "store":
        s = case["out_scale"]
        y, S = pre * s, S * abs(s)
        if case["res"]:
            y, S = y + _res_full(t), S + _res_full(t).abs()
        r["y"], r["S"] = (y.clamp_min(0) if case["relu"] else y), S
    elif epi == "ln_gelu":
        g, be = t["ln_g"].double(), t["ln_b"].double()
        mu, var = pre.mean(-1, keepdim=True), pre.var(-1, unbiased=False, keepdim=True)
        sig = (var + 1e-5).sqrt()
        z = (pre - mu) / sig
        r["y"] = gelu64(z * g + be)
        d = (2.0 ** -21 * S + 2.0 ** -23 * pre.abs()).amax(-1, keepdim=True)
        p32 = pre.float()
        y32 = torch.nn.functional.gelu(torch.nn.functional.layer_norm(p32, (512,), t["ln_g"], t["ln_b"], 1e-5))
        r["ln_bar"] = 1.13 * 2 * d * g.abs() * (1 + z.abs()) / sig + 2 * (y32.double() - r["y"]).abs()
        r["ln_bound"] = (t["ln_g"].abs() * math.sqrt(511.0) + t["ln_b"].abs()).max().item()
    elif epi == "qkv_rot":
        x, S = pre.view(-1, H, 64, 3), S.view(-1, H, 64, 3)
        for i, n in enumerate("qkv"):
            r[n], r["S" + n], r["x" + n] = x[..., i], S[..., i], torch.zeros_like(x[..., i])
        if case["rotary"]:
            for n in "qk":
                r[n], r["S" + n], r["x" + n] = _rotate(r[n], r["S" + n], t["cos"], t["sin"])
    else:
        sc = case["qk_scale"]
        qk, Sq = pre[:, :256].reshape(-1, H, 64) * sc, S[:, :256].reshape(-1, H, 64) * sc
        r["q"] = r["k"] = qk
        r["Sq"] = r["Sk"] = Sq
        r["xq"] = r["xk"] = 2.0 ** -22 * qk.abs()
        r["v"], r["Sv"], r["xv"] = pre[:, 256:].reshape(-1, H, 64), S[:, 256:].reshape(-1, H, 64), torch.zeros_like(qk)
    return r


def bars(case, ref, exps):
    """Per-element bars.  exps: the range exponents the planes were written with (out, out_v)."""
    Eo, Ev = exps.get("out", 0), exps.get("out_v", 0)
    prod = lambda S, y: 2.0 ** -21 * S + 2.0 ** -23 * y.abs()  # noqa: E731
    b = {}
    if case["epi"] == "store":
        b["y"] = prod(ref["S"], ref["y"])
        b["yp"] = b["y"] + 2.0 ** -22 * ref["y"].abs() + 2.0 ** (Eo - 35)
    elif case["epi"] == "ln_gelu":
        b["yp"] = ref["ln_bar"] + 2.0 ** -22 * ref["y"].abs() + 2.0 ** (Eo - 35)
    else:
        b["q"] = prod(ref["Sq"], ref["q"]) + ref["xq"]
        b["k"] = prod(ref["Sk"], ref["k"]) + ref["xk"] + 2.0 ** -22 * ref["k"].abs() + 2.0 ** (Eo - 35)
        b["v"] = prod(ref["Sv"], ref["v"]) + 2.0 ** -22 * ref["v"].abs() + 2.0 ** (Ev - 25)
    return b


def check(case, t, ref, out, exps):
    """{output: max err / bar over the live rows}; every compared value must be finite."""
    bar = bars(case, ref, exps)
    live = t["live"]
    ratios = {}
    for k, got in out.items():
        if got is None:
            continue
        want = ref["y"] if k == "yp" else ref[k]
        e = (got.double() - want)[live].abs()
        assert torch.isfinite(e).all(), f"{case['name']}: non-finite {k}"
        ratios[k] = (e / bar[k][live]).max().item() if e.numel() else 0.0
    return ratios


# ---------------------------------------------------------------------------------- emulation
def split2h(x, scaled=True):
    """common.h split2h / split2h_v of fp32 values held in float64: (h, l) as float64."""
    x32 = x.float()
    h = x32.half()
    lo = ((x32 - h.float()) * (2048.0 if scaled else 1.0)).half()
    return h.double(), lo.double()


def split3(x):
    x32 = x.float()
    h = x32.bfloat16()
    r = x32 - h.float()
    m = r.bfloat16()
    return h.double(), m.double(), (r - m.float()).bfloat16().double()


def _planes_codec(v, fmt, E, values=False):
    """What a consumer decodes from the planes written for fp32 values v."""
    if fmt == "x6":
        h, m, lo = split3(v)
        return h + m + lo
    h, lo = split2h(f32(v * 2.0 ** -E), scaled=not values)
    return (h + lo * (1.0 if values else 2.0 ** -11)) * 2.0 ** E


def _acc_h3(t, K0, K, ksplit, wrong):
    """The fp16x3 accumulator after the k-loop (and the split-k sum): (acc, accs, E0, E1)."""
    A0, A1, W = t["A0"], t["A1"], t["W"]
    e0 = range_exponent(A0.abs().max().item())
    e1 = range_exponent(A1.abs().max().item()) if A1 is not None else e0
    sw = weight_shift(W)
    wh, wl = split2h(W.double() * 2.0 ** sw)
    ah0, al0 = split2h(f32(A0.double() * 2.0 ** -e0))
    ah1, al1 = split2h(f32(A1.double() * 2.0 ** -e1)) if A1 is not None else (None, None)
    nk, nk0 = K // 32, K0 // 32
    seam = e0 != e1 and wrong != "no_seam_rescale"
    total = None
    for s in range(ksplit):
        kb, ke = (s * nk) // ksplit, ((s + 1) * nk) // ksplit
        acc = torch.zeros(A0.shape[0], W.shape[0], dtype=D)
        for kt in range(kb, ke):
            if kt == nk0 and seam:
                acc = acc * 2.0 ** (e0 - e1)
            ks = slice(kt * 32, kt * 32 + 32)
            ka = ks if kt < nk0 else slice((kt - nk0) * 32, (kt - nk0) * 32 + 32)
            ah, al = (ah0[:, ka], al0[:, ka]) if kt < nk0 else (ah1[:, ka], al1[:, ka])
            if wrong != "drop_low_high":
                acc = f32(acc + al @ wh[:, ks].T)
            acc = f32(acc + ah @ wl[:, ks].T)
            acc = f32(acc + ah @ (wh[:, ks] * 2048.0).T)
        if ksplit > 1 and ke <= nk0 and seam:
            acc = acc * 2.0 ** (e0 - e1)
        total = acc if total is None else f32(total + acc)
    return total, 2.0 ** (-(11 + sw) + e1), e0, e1


def _acc_x6(t, K):
    A, W = _cat_a(t), t["W"].double()
    a, w = split3(A), split3(W)
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=D)
    for k0 in range(0, K, 16):
        ks = slice(k0, k0 + 16)
        for i, j in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):  # common.h mfma_x6, smallest terms first
            acc = f32(acc + a[i][:, ks] @ w[j][:, ks].T)
    return acc


def emulate(case, t, fmt="h3", ksplit=1, wrong=None):
    """(outputs, exps) of the kernels' arithmetic on the CPU."""
    epi, R, K0, K, Nout = case["epi"], case["R"], case["K0"], case["K"], case["Nout"]
    bias = t["bias"].double() if t["bias"] is not None else torch.zeros(Nout, dtype=D)
    if wrong == "bias_neighbour_block":
        bias = bias.roll(-32)
    exps = {"a0": 0, "a1": 0, "out": 0, "out_v": 0}
    if fmt == "h3":
        acc, accs, exps["a0"], exps["a1"] = _acc_h3(t, K0, K, ksplit, wrong)
        x = f32(acc * accs + bias)  # one fma
        Ma = (t["A0"].abs().max().item(), t["A1"].abs().max().item() if t["A1"] is not None else 0.0)
    else:
        x = f32(_acc_x6(t, K) + bias)
        Ma = (0.0, 0.0)
    out = {}
    h3 = fmt == "h3"
    if epi == "store":
        v = f32(x * case["out_scale"])
        if case["res"]:
            res = _res_full(t)
            if wrong == "res_not_res2" and case["res2_row0"] is not None:
                r0 = case["res2_row0"]
                res = torch.cat([res[:r0], res[torch.arange(r0, R) % r0]])
            v = f32(res + v)
        if case["relu"]:
            v = v.clamp_min(0)
        out["y"] = v if case["fp32"] else None
        if case["planes"]:
            if h3:
                os_ = abs(case["out_scale"])
                l1 = t["W"].double().abs().sum(1).max().item() * os_
                bound = l1 * (Ma[0] + Ma[1]) + bias.abs().max().item() * os_
                bound += _res_full(t).abs().max().item() if case["res"] else 0.0
                exps["out"] = range_exponent(bound)
            out["yp"] = _planes_codec(v, fmt, exps["out"])
    elif epi == "ln_gelu":
        x32 = x.float()
        mean = x32.sum(-1, keepdim=True) * (1.0 / 512.0)
        d = x32 - mean
        var = (d * d).sum(-1, keepdim=True) * (1.0 / 512.0)
        rstd = 1.0 / torch.sqrt(var + (0.0 if wrong == "no_eps" else 1e-5))
        y = torch.nn.functional.gelu(d * rstd * t["ln_g"] + t["ln_b"]).double()
        if h3:
            exps["out"] = range_exponent((t["ln_g"].abs() * math.sqrt(511.0) + t["ln_b"].abs()).max().item())
        out["yp"] = _planes_codec(y, fmt, exps["out"]) if h3 else y
    else:
        rot = epi == "qkv_rot"
        xn = _packed_to_natural(x, 3 if rot else 2)  # [R][T][H][64]
        sc = 1.0 if rot else float(np.float32(case["qk_scale"]))
        q, k, v = (xn[:, 0], xn[:, 1], xn[:, 2]) if rot else (f32(xn[:, 0] * sc), None, xn[:, 1])
        if rot and case["rotary"]:
            c, s = t["cos"].double()[:, None, :], t["sin"].double()[:, None, :]
            if wrong == "rotary_sign":
                s = -s

            def rotf(a):
                e, o = a[..., 0::2], a[..., 1::2]
                y = torch.empty_like(a)
                y[..., 0::2] = f32(f32(e * c) + f32(-o * s))
                y[..., 1::2] = f32(f32(o * c) + f32(e * s))
                return y
            q, k = rotf(q), rotf(k)
        if not rot:
            k = q
        if h3:
            Wn = t["W"].double().abs().sum(1)
            bn = t["bias"].double().abs()
            ksl, vsl = (slice(256, 512), slice(512, 768)) if rot else (slice(0, 256), slice(256, 512))
            kf = 1.5 if rot else abs(sc)
            exps["out"] = range_exponent(Wn[ksl].max().item() * kf * Ma[0] + bn[ksl].max().item() * kf)
            exps["out_v"] = range_exponent(Wn[vsl].max().item() * Ma[0] + bn[vsl].max().item(), two_sided=True)
        out["q"] = q if (rot or case["q_given"]) else None
        out["k"] = _planes_codec(k, fmt, exps["out"])
        out["v"] = _planes_codec(v, fmt, exps["out_v"], values=True)
    return out, exps
