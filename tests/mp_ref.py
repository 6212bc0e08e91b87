"""CPU references for ``mp: true`` (single-product fp16 GEMMs, gemm_h3.hip H1): the helper of
test_mp_host.py, test_gpu_linear_mp.py and test_gpu_mp_forward.py.

Kernel level (the cases of linear_cases.py, the epilogue emulation of linear_ref.py):

* ``acc_h1`` / ``emulate``: the H1 accumulator -- the high pieces A_h = fp16(a 2^-E), W_h = fp16(w 2^sw)
  only, fp32 accumulation per 32-wide k-tile, the 2^(e0-e1) seam rescale, accumulator scale 2^(e1-sw)
  -- followed by linear_ref's emulation of the (unchanged) epilogues.
* two references per case.  *Loose*: ``linear_ref.reference``, float64 from the unrounded operands, with
  the product bar  2^-10 (1 + 2^-12) S + sub + 2^-23 |ref|  in place of linear_ref's 2^-21 S + 2^-23 |ref|:
  one relative 2^-11 rounding per operand ((1 + 2^-11)^2 - 1 = 2^-10 (1 + 2^-12)), and
  sub = sum_k 2^(E_k - 25) |w_ck| + 2^(-sw - 25) sum_k |a_rk| for pieces that land in the fp16 subnormal
  range, where the rounding error is absolute (half the subnormal spacing 2^-24, in plane units).  The
  plane, rotary and LayerNorm terms stay linear_ref's.  *Tight*: ``linear_ref.reference`` on inputs whose
  A0, A1 and W are replaced by their decoded high pieces, held to ``linear_ref.bars`` unchanged: with the
  operands rounded as the kernel rounds them, H1 must be as close to float64 as fp16x3 is.

Model level (the case of flash_ref.model_case): the CPU oracle run with fp16 linears,

* F1, the upstream form (autocast): input, weight, bias and output of every linear with >= 256 outputs
  rounded to fp16, flash_ref's upstream attention;
* F2, the library form: operands rounded where the library rounds them -- the activations' and weights'
  high pieces, out_proj / to_out folded into ffn.0 BEFORE the weight is rounded, so the message is never
  formed or rounded -- outputs, bias, residual stream and final_proj in fp32, flash_ref's tiled attention;
* A, the fp32 oracle.
"""
import contextlib
import functools
import math

import torch

import flash_ref as fr
import lgamd  # noqa: F401
import linear_ref as lr
import oracle.lightglue_ref as ref_mod

D = torch.float64
WRONG = ["keep_2^-11", "low_plane", "no_seam_rescale", "bias_neighbour_block", "res_not_res2"]
REL = 2.0 ** -10 * (1 + 2.0 ** -12)


# ---------------------------------------------------------------------------------- kernel level
def _exps(t):
    e0 = lr.range_exponent(t["A0"].abs().max().item())
    e1 = lr.range_exponent(t["A1"].abs().max().item()) if t["A1"] is not None else e0
    return e0, e1, lr.weight_shift(t["W"])


def acc_h1(t, K0, K, ksplit, wrong):
    """The H1 accumulator after the k-loop (and the split-k sum): (acc, accs, E0, E1); the counterpart of
    linear_ref._acc_h3."""
    A0, A1, W = t["A0"], t["A1"], t["W"]
    e0, e1, sw = _exps(t)
    piece = 1 if wrong == "low_plane" else 0
    wh = lr.split2h(W.double() * 2.0 ** sw)[0]
    a0 = lr.split2h(lr.f32(A0.double() * 2.0 ** -e0))[piece]
    a1 = lr.split2h(lr.f32(A1.double() * 2.0 ** -e1))[piece] if A1 is not None else None
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
            ah = a0[:, ks] if kt < nk0 else a1[:, (kt - nk0) * 32:(kt - nk0) * 32 + 32]
            acc = lr.f32(acc + ah @ wh[:, ks].T)
        if ksplit > 1 and ke <= nk0 and seam:
            acc = acc * 2.0 ** (e0 - e1)
        total = acc if total is None else lr.f32(total + acc)
    return total, 2.0 ** ((-11 if wrong == "keep_2^-11" else 0) - sw + e1), e0, e1


def emulate(case, t, ksplit=1, wrong=None):
    """(outputs, exps) of the H1 kernel's arithmetic on the CPU: acc_h1, then linear_ref's epilogues."""
    saved = lr._acc_h3
    lr._acc_h3 = acc_h1
    try:
        return lr.emulate(case, t, "h3", ksplit, wrong)
    finally:
        lr._acc_h3 = saved


def rounded_inputs(case, t):
    """The case's inputs with A0, A1 and W replaced by their decoded high pieces (the tight reference's)."""
    e0, e1, sw = _exps(t)
    hi = lambda x, s: (lr.split2h(lr.f32(x.double() * 2.0 ** s))[0] * 2.0 ** -s).float()  # noqa: E731
    r = dict(t)
    r["A0"] = hi(t["A0"], -e0)
    r["A1"] = hi(t["A1"], -e1) if t["A1"] is not None else None
    r["W"] = hi(t["W"], sw)
    if "W_nat" in t:
        r["W_nat"] = hi(t["W_nat"], sw)
    return r


def _sub(case, t):
    """sub of the loose bar, taken through the epilogue the way linear_ref.reference takes S."""
    e0, e1, sw = _exps(t)
    K0, K = case["K0"], case["K"]
    A = lr._cat_a(t)
    W = (t["W_nat"] if case["head"] else t["W"]).double()
    ek = torch.cat([torch.full((K0,), 2.0 ** (e0 - 25), dtype=D), torch.full((K - K0,), 2.0 ** (e1 - 25), dtype=D)])
    sub = (W.abs() @ ek)[None, :] + 2.0 ** (-sw - 25) * A.abs().sum(1, keepdim=True)
    epi = case["epi"]
    if epi == "store":
        return {"y": sub * abs(case["out_scale"])}
    if epi == "ln_gelu":
        return {"pre": sub}
    if epi == "qkv_rot":
        x = sub.view(-1, lr.H, 64, 3)
        out = {n: x[..., i] for i, n in enumerate("qkv")}
        if case["rotary"]:
            c, s = t["cos"].double()[:, None, :].abs(), t["sin"].double()[:, None, :].abs()
            for n in "qk":
                e, o = out[n][..., 0::2], out[n][..., 1::2]
                y = torch.empty_like(out[n])
                y[..., 0::2], y[..., 1::2] = e * c + o * s, o * c + e * s
                out[n] = y
        return out
    qk = sub[:, :256].reshape(-1, lr.H, 64) * case["qk_scale"]
    return {"q": qk, "k": qk, "v": sub[:, 256:].reshape(-1, lr.H, 64)}


def bars_loose(case, t, ref, exps):
    """linear_ref.bars with the H1 product bar against the unrounded reference."""
    Eo, Ev = exps.get("out", 0), exps.get("out_v", 0)
    sub = _sub(case, t)
    prod = lambda S, y, sb: REL * S + sb + 2.0 ** -23 * y.abs()  # noqa: E731
    b = {}
    if case["epi"] == "store":
        b["y"] = prod(ref["S"], ref["y"], sub["y"])
        b["yp"] = b["y"] + 2.0 ** -22 * ref["y"].abs() + 2.0 ** (Eo - 35)
    elif case["epi"] == "ln_gelu":
        # linear_ref.reference's first-order propagation with the new row bar d
        A = lr._cat_a(t)
        W, bias = t["W"].double(), t["bias"].double()
        pre, S = A @ W.T + bias, A.abs() @ W.abs().T + bias.abs()
        g = t["ln_g"].double()
        mu, var = pre.mean(-1, keepdim=True), pre.var(-1, unbiased=False, keepdim=True)
        sig = (var + 1e-5).sqrt()
        z = (pre - mu) / sig
        d = prod(S, pre, sub["pre"]).amax(-1, keepdim=True)
        y32 = torch.nn.functional.gelu(torch.nn.functional.layer_norm(pre.float(), (512,), t["ln_g"], t["ln_b"], 1e-5))
        ln_bar = 1.13 * 2 * d * g.abs() * (1 + z.abs()) / sig + 2 * (y32.double() - ref["y"]).abs()
        b["yp"] = ln_bar + 2.0 ** -22 * ref["y"].abs() + 2.0 ** (Eo - 35)
    else:
        b["q"] = prod(ref["Sq"], ref["q"], sub["q"]) + ref["xq"]
        b["k"] = prod(ref["Sk"], ref["k"], sub["k"]) + ref["xk"] + 2.0 ** -22 * ref["k"].abs() + 2.0 ** (Eo - 35)
        b["v"] = prod(ref["Sv"], ref["v"], sub["v"]) + 2.0 ** -22 * ref["v"].abs() + 2.0 ** (Ev - 25)
    return b


def _ratios(case, t, ref, out, bar):
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


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(case, inputs, loose reference, tight reference) of a linear_cases case, computed once and shared."""
    import linear_cases as lc

    case = lc.BY_NAME[name]
    t = lc.build_inputs(case)
    return case, t, lr.reference(case, t), lr.reference(case, rounded_inputs(case, t))


def check(name, out, exps):
    """({output: err / loose bar}, {output: err / tight bar}, {output: err / fp16x3 bar vs the loose reference})
    over the live rows."""
    case, t, loose, tight = prepared(name)
    return (_ratios(case, t, loose, out, bars_loose(case, t, loose, exps)),
            _ratios(case, t, tight, out, lr.bars(case, tight, exps)),
            _ratios(case, t, loose, out, lr.bars(case, loose, exps)))


# ---------------------------------------------------------------------------------- model level
def _h(x):
    return x.half().float()


def _hi_w(w):
    """The weight's high piece fp16(w 2^sw) 2^-sw (lightglue_api.cpp's per-matrix shift)."""
    sw = lr.weight_shift(w)
    return (w * 2.0 ** sw).half().float() * 2.0 ** -sw


def _hi_a(x):
    """An activation's high piece fp16(x 2^-E) 2^E, E from the tensor's maximum (the library derives E from a
    bound >= the maximum; both are 0 below 2^15, which holds for the model case throughout)."""
    e = lr.range_exponent(x.abs().max().item())
    return (x * 2.0 ** -e).half().float() * 2.0 ** e


def _lin_lib(x, w, b):
    return torch.nn.functional.linear(_hi_a(x), _hi_w(w), b)


@contextlib.contextmanager
def _mp_oracle(variant):
    """ref_mod with fp16 linears: "upstream" (F1) or "library" (F2)."""
    plain = ref_mod._linear
    names = ("_linear", "_ffn", "self_block", "cross_block", "_softmax_attention")
    saved = {n: getattr(ref_mod, n) for n in names}
    if variant == "upstream":
        def linear(x, w, b):
            if w.shape[0] < 256:  # matchability / token heads: GEMVs, fp32 in the library too
                return plain(x, w, b)
            return _h(plain(_h(x), _h(w), _h(b) if b is not None else None))

        ref_mod._linear = linear
        inner = fr._flash_oracle("upstream")  # captures the patched _linear for its cross block
    else:
        def linear(x, w, b):
            if w.shape[0] == 256 and w.shape[1] != 256:  # input_proj (input_dim != 256); final_proj stays fp32
                return _lin_lib(x, w, b)
            return plain(x, w, b)

        def ffn_folded(x, ctx, W, p, o):
            """ffn.0 on [x | ctx] with out_proj / to_out (`o`) folded into its message half, then LN, GELU,
            ffn.3 and the fp32 residual."""
            W0, b0 = W[p + ".ffn.0.weight"].double(), W[p + ".ffn.0.bias"].double()
            Wo, bo = W[p + o + ".weight"].double(), W[p + o + ".bias"].double()
            Wf = torch.cat([W0[:, :256], W0[:, 256:] @ Wo], 1).float()
            bf = (b0 + W0[:, 256:] @ bo).float()
            h = torch.nn.functional.linear(torch.cat([_hi_a(x), _hi_a(ctx)], -1), _hi_w(Wf), bf)
            h = torch.nn.functional.layer_norm(h, (512,), W[p + ".ffn.1.weight"], W[p + ".ffn.1.bias"], eps=1e-5)
            return x + _lin_lib(torch.nn.functional.gelu(h), W[p + ".ffn.3.weight"], W[p + ".ffn.3.bias"])

        def self_block(x, cos, sin, W, p, H):
            qkv = _lin_lib(x, W[p + ".Wqkv.weight"], W[p + ".Wqkv.bias"]).unflatten(-1, (H, -1, 3)).transpose(1, 2)
            q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
            q, k = ref_mod._rotary(q, cos, sin), ref_mod._rotary(k, cos, sin)
            ctx = fr.emu_tiled_heads(q, k, v, (x.shape[-1] // H) ** -0.5)
            return ffn_folded(x, ctx.transpose(1, 2).flatten(-2), W, p, ".out_proj")

        def cross_block(x0, x1, W, p, H):
            def heads(t):
                return t.unflatten(-1, (H, -1)).transpose(1, 2)

            # to_qk and to_v are one 512-output GEMM in the library: one weight shift for both
            Wc = torch.cat([W[p + ".to_qk.weight"], W[p + ".to_v.weight"]])
            bc = torch.cat([W[p + ".to_qk.bias"], W[p + ".to_v.bias"]])
            y0, y1 = _lin_lib(x0, Wc, bc), _lin_lib(x1, Wc, bc)
            s = (x0.shape[-1] // H) ** -0.5
            qk0, qk1 = heads(y0[..., :256]) * s ** 0.5, heads(y1[..., :256]) * s ** 0.5
            v0, v1 = heads(y0[..., 256:]), heads(y1[..., 256:])
            m0, m1 = fr.emu_tiled_heads(qk0, qk1, v1, 1.0), fr.emu_tiled_heads(qk1, qk0, v0, 1.0)
            return (ffn_folded(x0, m0.transpose(1, 2).flatten(-2), W, p, ".to_out"),
                    ffn_folded(x1, m1.transpose(1, 2).flatten(-2), W, p, ".to_out"))

        ref_mod._linear, ref_mod.self_block, ref_mod.cross_block = linear, self_block, cross_block
        inner = contextlib.nullcontext()
    try:
        with inner:
            yield
    finally:
        for n, v in saved.items():
            setattr(ref_mod, n, v)


def lightglue_forward_mp(W, data, conf, variant):
    with _mp_oracle(variant), torch.no_grad():
        return ref_mod.lightglue_forward(W, data, conf)


EXCLUDED_CAP = 0.10
MODEL_SEED = fr.MODEL_SEED  # the pair seed of flash_ref.model_case


@functools.lru_cache(maxsize=None)
def model_case():
    """(weights, data, A, F1, F2) on flash_ref.model_case's weights and pair, computed once and shared."""
    sd, data, A, _, _ = fr.model_case()
    return sd, data, A, lightglue_forward_mp(sd, data, fr.MODEL_CONF, "upstream"), lightglue_forward_mp(
        sd, data, fr.MODEL_CONF, "library")


def _margins(la, idx=None):
    """top-1 minus top-2 along the last dim (dustbin column included), at `idx` ([..., 2]) when given."""
    if idx is None:
        idx = la.topk(2, dim=-1).indices
    v = la.gather(-1, idx)
    return v[..., 0] - v[..., 1], idx


def spreads(F1, F2):
    """(d_s, d_m): the F1-F2 spread of the matching scores, and of the decision margin -- top-1 minus top-2
    of F1's log-assignment row / column, evaluated at F1's indices in both."""
    d_s = max((F1[k] - F2[k]).abs().max().item() for k in ("matching_scores0", "matching_scores1"))
    d_m = 0.0
    for sel in (lambda la: la[:, :-1, :], lambda la: la[:, :, :-1].transpose(1, 2)):
        m1, idx = _margins(sel(F1["log_assignment"].double()))
        m2, _ = _margins(sel(F2["log_assignment"].double()), idx)
        d_m = max(d_m, (m1 - m2).abs().max().item())
    return d_s, d_m


def excluded_masks(F1, F2, th):
    """Boolean [B, M] / [B, N]: rows left out of the match comparison -- F1 != F2 on the row, F1's margin
    below 2 d_m, or the row's best non-dustbin score within 2 d_s of the filter threshold."""
    d_s, d_m = spreads(F1, F2)
    la = F1["log_assignment"].double()
    out = []
    for side, rows in (("0", la[:, :-1, :]), ("1", la[:, :, :-1].transpose(1, 2))):
        margin, _ = _margins(rows)
        best = rows[..., :-1].amax(-1).exp()
        out.append((F1["matches" + side] != F2["matches" + side]) | (margin < 2 * d_m) | ((best - th).abs() < 2 * d_s))
    return out[0], out[1]


def excluded_share(m0, m1):
    return (m0.sum().item() + m1.sum().item()) / (m0.numel() + m1.numel())
