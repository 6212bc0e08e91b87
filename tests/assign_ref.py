"""Float64 reference, error bars and CPU emulations for the kernel-level assignment tests.

reference(case, t, src)      la / matches of every pair in float64 from the fp32 inputs (a counted pair: the
                             reference run alone at Mb x Nb), placed into the layout of the contract, with the
                             per-element bars and the rows / columns whose matches float64 decides
emulate(case, t, src, ...)   the kernels' arithmetic in torch: recomputed = plane split at the measured
                             exponent, three fp16 products per k-tile accumulated in fp32, per-tile (max, sum)
                             partials merged in tile order, fp32 score_at, per-tile first argmax merged with >;
                             materialised = fp32 score_at on the given (or bf16x6) sim with CCH-row column
                             partials.  `wrong=...` runs one of WRONG's deliberate mistakes.
check(case, t, ref, got)     the exact checks (assert) and {output: worst err / bar}

Bars (none is taken from a kernel).  Similarity, per element, S = |md0| |md1|^T:
  recomputed            d = 2^-20 S + 2^-23 |sim| + floor
  materialised from md  d = 2^-21 S + 2^-23 |sim|        (linear_ref's product bar, bf16x6)
  materialised on sim   d = 0                            (the kernels read the reference's own input)
2^-20 S is linear_ref's 2^-21 S plus 2 * 2^-22 S: there one operand is a plane image and the other a weight
image split on the host; here both are run-time plane images, each element carrying the relative error
2^-22 of its low piece's rounding.
floor: a plane image stores x' = x 2^-E as h = fp16(x') and l = fp16((x' - h) 2^11).  Beside the relative
2^-22 |x| there is an absolute error: where (x' - h) 2^11 falls below 2^-14 it is an fp16 subnormal with
spacing 2^-24, so l is off by up to 2^-25, that is 2^-36 in x' and 2^(E-36) in x; linear_ref.py allows
twice that, eps = 2^(E-35), and so does this.  For sum_k (a_k + alpha_k)(b_k + beta_k) with |alpha|, |beta|
<= eps over 256 terms the product moves by at most
  floor_ij = eps (|md0_i|_1 + |md1_j|_1) + 256 eps^2.
la = (x - rmax - rlog) + (x - cmax - clog) + ls0 + ls1: x enters twice directly and once through each
log-sum-exp, whose derivative with respect to x_ij' is the softmax weight, so
  bar_ij = 2 d_ij + sum_j' p_row_ij' d_ij' + sum_i' p_col_i'j d_i'j + e32_ij
  e32_ij = 2^-24 ((n_row / 64 + 16) + (n_col / 64 + 16))
           + 2^-22 (|x - rmax| + |x - cmax| + |rlog| + |clog| + |ls0| + |ls1| + |la|)
(reduction depth of the two sums, one rounding per level; one rounding per operation of score_at with a
margin of about 4).  Scores: exp(la) (bar + 2^-22).  Dustbins: logsigmoid(-z) in fp32 is min(x, 0) -
log1p(exp(-|x|)), three operations of at most an ulp or two each: 2^-21 |v|.
"""
import math

import numpy as np
import torch

import assign_cases as ac
import linear_ref as lr
import oracle

D = torch.float64
SENT_F = float(np.float32(-123.456))
SENT_I = -77
WRONG = ["drop_low_high", "drop_last_tile", "colstats_next_pair", "dead_cols_in_rowsum", "last_index_ties", "merge_ge",
         "dustbin_at_Nb_fixed", "threshold_ge"]


def dmode(case, src):
    return "h3" if case["route"] == "recomputed" else ("zero" if src == "sim" else "x6")


def measured_exponent(t):
    """The exponent lg_assign's image is written with: range_exponent of the measured max |md|, lshift 11."""
    return lr.range_exponent(max(t["md0"].abs().max().item(), t["md1"].abs().max().item()), lshift=11)


def sim_f32(t):
    """The fp32 similarity a caller hands to the materialised route: the float64 product rounded once."""
    return (t["md0"].double() @ t["md1"].double().transpose(1, 2)).float()


# ---------------------------------------------------------------------------------- layout
def assemble(case, pairs, dtype, fill, dustbin_at_nb=False):
    """Per-pair results -> the contract's layout.  pairs[b]: la_in [mb][nb], d0 [mb], d1 [nb], m0, m1, s0, s1."""
    B, M, N = case["B"], case["M"], case["N"]
    fixed = bool(case["fixed"])
    la = torch.full((B, M + 1, N + 1), -math.inf if fixed else fill, dtype=dtype)
    m0, m1 = torch.full((B, M), SENT_I, dtype=torch.long), torch.full((B, N), SENT_I, dtype=torch.long)
    s0, s1 = torch.full((B, M), fill, dtype=dtype), torch.full((B, N), fill, dtype=dtype)
    for b, p in enumerate(pairs):
        mb, nb = p["la_in"].shape
        jc, ir = (N, M) if fixed and not dustbin_at_nb else (nb, mb)
        la[b, :mb, :nb] = p["la_in"]
        la[b, :mb, jc] = p["d0"]
        la[b, ir, :nb] = p["d1"]
        la[b, M if fixed else mb, N if fixed else nb] = 0.0
        m0[b, :mb], m1[b, :nb], s0[b, :mb], s1[b, :nb] = p["m0"], p["m1"], p["s0"], p["s1"]
    return dict(la=la, m0=m0, m1=m1, s0=s0, s1=s1)


def _no_matches(mb, nb, dtype):
    return dict(m0=torch.full((mb,), -1, dtype=torch.long), m1=torch.full((nb,), -1, dtype=torch.long),
                s0=torch.zeros(mb, dtype=dtype), s1=torch.zeros(nb, dtype=dtype))


# ---------------------------------------------------------------------------------- reference
def _pair_reference(md0, md1, z0, z1, sim, mode, E, th, dups=((), ())):
    mb, nb = md0.shape[0], md1.shape[0]
    r = dict(d0=torch.nn.functional.logsigmoid(-z0.double()), d1=torch.nn.functional.logsigmoid(-z1.double()))
    r["la_in"] = r["bar"] = torch.zeros(mb, nb, dtype=D)
    r["safe0"], r["safe1"] = torch.ones(mb, dtype=torch.bool), torch.ones(nb, dtype=torch.bool)
    if mb == 0 or nb == 0:
        r.update(_no_matches(mb, nb, D), sbar0=torch.zeros(mb, dtype=D), sbar1=torch.zeros(nb, dtype=D))
        return r
    x = sim.double() if sim is not None else md0.double() @ md1.double().T
    if mode == "zero":
        d = torch.zeros_like(x)
    else:
        S = md0.double().abs() @ md1.double().abs().T
        if mode == "x6":
            d = 2.0 ** -21 * S + 2.0 ** -23 * x.abs()
        else:
            eps = 2.0 ** (E - 35)
            floor = eps * (md0.double().abs().sum(1)[:, None] + md1.double().abs().sum(1)[None, :]) + 256 * eps * eps
            d = 2.0 ** -20 * S + 2.0 ** -23 * x.abs() + floor
    rmax, cmax = x.amax(1, keepdim=True), x.amax(0, keepdim=True)
    rlog, clog = (x - rmax).exp().sum(1, keepdim=True).log(), (x - cmax).exp().sum(0, keepdim=True).log()
    ls0 = torch.nn.functional.logsigmoid(z0.double())[:, None]
    ls1 = torch.nn.functional.logsigmoid(z1.double())[None, :]
    la = (x - rmax - rlog) + (x - cmax - clog) + ls0 + ls1
    prow, pcol = torch.softmax(x, 1), torch.softmax(x, 0)
    e32 = 2.0 ** -24 * ((nb / 64 + 16) + (mb / 64 + 16)) + 2.0 ** -22 * (
        (x - rmax).abs() + (x - cmax).abs() + rlog.abs() + clog.abs() + ls0.abs() + ls1.abs() + la.abs())
    bar = 2 * d + (prow * d).sum(1, keepdim=True) + (pcol * d).sum(0, keepdim=True) + e32
    # the planted duplicates are equal by construction; library kernels may round the two copies differently in
    # the last place (vector body against scalar tail), so one copy stands for both
    for _, j1, j2 in dups[0]:
        assert (la[:, j1] - la[:, j2]).abs().max() <= 1e-12
        la[:, j2] = la[:, j1]
    for _, i1, i2 in dups[1]:
        assert (la[i1] - la[i2]).abs().max() <= 1e-12
        la[i2] = la[i1]
    r["la_in"], r["bar"] = la, bar
    full = torch.zeros(1, mb + 1, nb + 1, dtype=D)
    full[0, :mb, :nb] = la
    m0, m1, s0, s1 = (v[0] for v in oracle.filter_matches(full, th))
    r.update(m0=m0, m1=m1, s0=s0, s1=s1)
    # which rows / columns float64 decides: top-1 / top-2 margin >= 2 max bar, exp(max) not within its bar of th
    def margins(v, bars_, dim):
        # values exactly equal to the best are one candidate (a planted duplicate: the first index decides, and
        # ties_bitwise asserts that what the kernels write ties exactly too); the margin is to the best of the rest
        best = v.max(dim)
        rest = v.masked_fill(v == best.values.unsqueeze(dim), -math.inf).amax(dim)
        return best.values - rest >= 2 * bars_.amax(dim), best.indices, best.values
    ok0, a0, v0 = margins(la, bar, 1)
    ok1, a1, _ = margins(la, bar, 0)
    rows = torch.arange(mb)
    sb0 = v0.exp() * (bar[rows, a0] + 2.0 ** -22)
    th_ok = (v0.exp() - th).abs() > sb0
    r["safe0"] = ok0 & ok1[a0] & th_ok
    r["safe1"] = ok1 & ok0[a1] & th_ok[a1]
    r["sbar0"], r["sbar1"] = sb0, sb0[a1]
    r["arg0"], r["arg1"], r["max0"] = la.max(1).indices, la.max(0).indices, v0  # torch-CPU max: the first index
    return r


def reference(case, t, src="md"):
    """src: "md" (similarity from md0 / md1) or "sim" (materialised route on sim_f32(t))."""
    mode = dmode(case, src)
    E = measured_exponent(t) if mode == "h3" else 0
    sim = sim_f32(t) if src == "sim" else None
    pairs = []
    for b, (mb, nb) in enumerate(t["counts"]):
        pairs.append(_pair_reference(t["md0"][b, :mb], t["md1"][b, :nb], t["z0"][b, :mb], t["z1"][b, :nb],
                                     None if sim is None else sim[b, :mb, :nb], mode, E, ac.TH,
                                     (t["jt"], t["it"]) if b == 0 else ((), ())))
    ref = assemble(case, pairs, D, math.nan)
    ref["bar"] = assemble(case, [dict(p, la_in=p["bar"], d0=2.0 ** -21 * p["d0"].abs(), d1=2.0 ** -21 * p["d1"].abs())
                                 for p in pairs], D, math.nan)["la"]
    ref["bar"][ref["bar"] == -math.inf] = 0.0
    ref["pairs"], ref["E"] = pairs, E
    live = sum(mb + nb for mb, nb in t["counts"])
    out = sum(int((~p["safe0"]).sum()) + int((~p["safe1"]).sum()) for p in pairs)
    ref["left_out"] = out / max(live, 1)
    return ref


def assert_ties_decide(case, t, ref):
    """The planted duplicates are exact ties in float64 and the best of their row / column: first index decides."""
    p = ref["pairs"][0]
    la = p["la_in"]
    for i, j1, j2 in t["jt"]:
        assert la[i, j1] == la[i, j2] == la[i].max() and p["arg0"][i] == j1, (case["name"], i, j1, j2)
        assert (la[:, j1] == la[:, j2]).all()
    for j, i1, i2 in t["it"]:
        assert la[i1, j] == la[i2, j] == la[:, j].max() and p["arg1"][j] == i1, (case["name"], j, i1, i2)
        assert (la[i1] == la[i2]).all()
    return len(t["jt"]) + len(t["it"])


# ---------------------------------------------------------------------------------- emulation
def _sim_h3(md0, md1, E, wrong):
    ah, al = lr.split2h(lr.f32(md0.double() * 2.0 ** -E))
    bh, bl = lr.split2h(lr.f32(md1.double() * 2.0 ** -E))
    acc = torch.zeros(md0.shape[0], md1.shape[0], dtype=D)
    for kt in range(8):
        ks = slice(kt * 32, kt * 32 + 32)
        if wrong != "drop_low_high":
            acc = lr.f32(acc + al[:, ks] @ bh[:, ks].T)
        acc = lr.f32(acc + ah[:, ks] @ bl[:, ks].T)
        acc = lr.f32(acc + ah[:, ks] @ (bh[:, ks] * 2048.0).T)
    return lr.f32(acc * 2.0 ** (2 * E - 11)).float()


def _edges(n, step):
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def _exp(x):
    """fp32 exp, correctly rounded (torch's vectorised fp32 exp may differ by an ulp between the body and the tail
    of an array, which would break the planted ties on the CPU)."""
    return x.double().exp().float()


def _parts(x, dim, edges):
    out = []
    for a, b in edges:
        seg = x.narrow(dim, a, b - a)
        m = seg.amax(dim)
        # fp32 sums over a contiguous last dimension: every row / column is reduced in the same order
        out.append((m, _exp(seg - m.unsqueeze(dim)).transpose(dim, -1).contiguous().sum(-1)))
    return out


def _merge_pairwise(parts):
    """tile_reduce.h lse_merge, in tile order."""
    m, s = parts[0]
    for bm, bs in parts[1:]:
        mm = torch.maximum(m, bm)
        s = s * _exp(m - mm) + bs * _exp(bm - mm)
        m = mm
    return m, s.double().log().float()


def _merge_chunks(parts):
    """assign.hip col_stats_combine_kernel: the max first, then the rescaled sums in chunk order."""
    m = parts[0][0]
    for bm, _ in parts[1:]:
        m = torch.maximum(m, bm)
    s = torch.zeros_like(m)
    for bm, bs in parts:
        s = s + bs * _exp(bm - m)
    return m, s.double().log().float()


def _argmax(v, dim, edges, last, ge):
    n = v.shape[dim]
    idx = torch.arange(n).view([-1 if k == dim else 1 for k in range(2)]).expand_as(v)
    bv = bi = None
    for a, b in edges:
        seg, ids = v.narrow(dim, a, b - a), idx.narrow(dim, a, b - a)
        val = seg.amax(dim)
        hit = seg == val.unsqueeze(dim)
        i = torch.where(hit, ids, -1).amax(dim) if last else torch.where(hit, ids, n).amin(dim)
        if bv is None:
            bv, bi = val, i
        else:
            take = (val >= bv) if ge else (val > bv)
            bv, bi = torch.where(take, val, bv), torch.where(take, i, bi)
    return bv, bi


def _pair_emulate(route, x, z0, z1, p, wrong, extra_cols=None, colstats=None, th=ac.TH):
    """x: the fp32 similarity [mb][nb] the kernels see.  Returns the pair's results and its column statistics."""
    mb, nb = x.shape
    f = torch.float32
    r = dict(d0=torch.nn.functional.logsigmoid(-z0.to(f)), d1=torch.nn.functional.logsigmoid(-z1.to(f)), la_in=x.new_zeros(mb, nb))
    if mb == 0 or nb == 0:
        r.update(_no_matches(mb, nb, f))
        return r, None
    tile = p["kSimTile"]
    ce = _edges(nb, tile) if route == "recomputed" else [(0, nb)]     # column segments of a row
    re_ = _edges(mb, tile if route == "recomputed" else p["CCH"])     # row segments of a column
    rparts = _parts(x, 1, ce)
    if wrong == "drop_last_tile" and len(rparts) > 1:
        rparts = rparts[:-1]
    if wrong == "dead_cols_in_rowsum" and extra_cols is not None and extra_cols.shape[1]:
        m = extra_cols.amax(1)
        rparts.append((m, _exp(extra_cols - m[:, None]).sum(1)))
    rm, rl = _merge_pairwise(rparts)
    cm, cl = _merge_pairwise(_parts(x, 0, re_)) if route == "recomputed" else _merge_chunks(_parts(x, 0, re_))
    own = (cm, cl)
    if colstats is not None:
        cm, cl = colstats
    l0, l1 = torch.nn.functional.logsigmoid(z0.to(f)), torch.nn.functional.logsigmoid(z1.to(f))
    s0 = (x - rm[:, None]) - rl[:, None]
    s1 = (x - cm[None, :]) - cl[None, :]
    v = (s0 + s1) + (l0[:, None] + l1[None, :])
    last, ge = wrong == "last_index_ties", wrong == "merge_ge"
    max0, arg0 = _argmax(v, 1, ce, last, ge)
    _, arg1 = _argmax(v, 0, re_, last, ge)
    th = torch.tensor(th, dtype=f)
    sc = torch.exp(max0)
    over = (sc >= th) if wrong == "threshold_ge" else (sc > th)
    mut0 = arg1[arg0] == torch.arange(mb)
    mut1 = arg0[arg1] == torch.arange(nb)
    r.update(la_in=v, m0=torch.where(mut0 & over, arg0, -1), s0=torch.where(mut0, sc, sc.new_zeros(())),
             m1=torch.where(mut1 & over[arg1], arg1, -1), s1=torch.where(mut1, sc[arg1], sc.new_zeros(())))
    return r, own


def emulate(case, t, src="md", wrong=None, th=ac.TH):
    """The route's arithmetic on the CPU, in the contract's layout (fp32)."""
    p = ac.parsed()
    route = case["route"]
    mode = dmode(case, src)
    E = measured_exponent(t) if mode == "h3" else 0
    given = sim_f32(t) if src == "sim" else None
    sims = []
    for b, (mb, nb) in enumerate(t["counts"]):
        md0, md1 = t["md0"][b, :mb], t["md1"][b]
        if mode == "h3":
            x = _sim_h3(md0, md1, E, wrong)
        elif mode == "x6":
            x = lr._acc_x6({"A0": md0, "A1": None, "W": md1}, 256).float()
        else:
            x = given[b, :mb]
        if b == 0:  # identical rows go through identical arithmetic in the kernels (see _pair_reference)
            x = x.clone()
            for _, j1, j2 in t["jt"]:
                x[:, j2] = x[:, j1]
            for _, i1, i2 in t["it"]:
                x[i2] = x[i1]
        sims.append(x)
    stats = [None] * len(sims)
    if wrong == "colstats_next_pair":
        for b, (mb, nb) in enumerate(t["counts"]):
            _, stats[b] = _pair_emulate(route, sims[b][:, :nb], t["z0"][b, :mb], t["z1"][b, :nb], p, None)
        stats = stats[1:] + stats[:1]
    pairs = []
    for b, (mb, nb) in enumerate(t["counts"]):
        r, _ = _pair_emulate(route, sims[b][:, :nb], t["z0"][b, :mb], t["z1"][b, :nb], p, wrong, sims[b][:, nb:], stats[b], th)
        pairs.append(r)
    got = assemble(case, pairs, torch.float32, SENT_F, dustbin_at_nb=wrong == "dustbin_at_Nb_fixed")
    got["E"] = E
    return got


# ---------------------------------------------------------------------------------- checks
def check(case, t, ref, got, th=ac.TH, vs64=True):
    """Exact checks (assert) and {name: worst err / bar}.  got: la (or None), m0, m1, s0, s1 in the layout.
    vs64 = False (a threshold other than the reference's): only the checks that need no float64 matches."""
    name = case["name"]
    B, M, N = case["B"], case["M"], case["N"]
    fixed = bool(case["fixed"])
    ratios = {}
    sent = torch.tensor(SENT_F)
    la = got.get("la")
    if la is not None:
        want, bar = ref["la"], ref["bar"]
        undefined = want.isnan()
        assert (la[undefined] == sent).all(), f"{name}: la written outside the defined blocks"
        exact = ~undefined & ((bar == 0) | want.isinf())
        assert (la[exact].double() == want[exact]).all(), f"{name}: an exact entry of la (-inf / corner 0) is off"
        num = ~undefined & ~exact
        err = (la[num].double() - want[num]).abs()
        assert torch.isfinite(err).all(), f"{name}: non-finite la"
        inner = torch.zeros_like(num)
        for b, (mb, nb) in enumerate(t["counts"]):
            inner[b, :mb, :nb] = True
        ratios["la"] = ((la.double() - want).abs() / bar)[num & inner].max().item() if (num & inner).any() else 0.0
        ratios["dustbin"] = ((la.double() - want).abs() / bar)[num & ~inner].max().item() if (num & ~inner).any() else 0.0
    for b, (mb, nb) in enumerate(t["counts"]):
        p = ref["pairs"][b]
        gm0, gm1, gs0, gs1 = got["m0"][b], got["m1"][b], got["s0"][b], got["s1"][b]
        # dead rows / columns keep the sentinel
        assert (gm0[mb:] == SENT_I).all() and (gm1[nb:] == SENT_I).all(), f"{name}[{b}]: a dead match was written"
        assert (gs0[mb:] == sent).all() and (gs1[nb:] == sent).all(), f"{name}[{b}]: a dead score was written"
        if mb == 0 or nb == 0:  # an empty side: no matches
            assert (gm0[:mb] == -1).all() and (gm1[:nb] == -1).all() and (gs0[:mb] == 0).all() and (gs1[:nb] == 0).all(), \
                f"{name}[{b}]: matches in a pair with an empty side"
            continue
        # the filter on the values actually written: every argmax, tie and merge order, exactly
        if la is not None:
            own = torch.zeros(1, mb + 1, nb + 1)
            own[0, :mb, :nb] = la[b, :mb, :nb]
            o0, o1, os0, os1 = (v[0] for v in oracle.filter_matches(own, th))
            assert torch.equal(gm0[:mb], o0) and torch.equal(gm1[:nb], o1), f"{name}[{b}]: matches differ from filter_matches on the written la"
            np.testing.assert_allclose(gs0[:mb].numpy(), os0.numpy(), rtol=3e-7, atol=0, err_msg=f"{name}[{b}] s0")
            np.testing.assert_allclose(gs1[:nb].numpy(), os1.numpy(), rtol=3e-7, atol=0, err_msg=f"{name}[{b}] s1")
        if not vs64:
            continue
        # against float64, wherever float64 decides
        s0, s1 = p["safe0"], p["safe1"]
        assert torch.equal(gm0[:mb][s0], p["m0"][s0]) and torch.equal(gm1[:nb][s1], p["m1"][s1]), \
            f"{name}[{b}]: matches differ from float64 on decided rows / columns"
        for k, g, w, sb, ok in (("s0", gs0[:mb], p["s0"], p["sbar0"], s0), ("s1", gs1[:nb], p["s1"], p["sbar1"], s1)):
            e = (g.double() - w).abs()[ok]
            zero = w[ok] == 0
            assert (e[zero] == 0).all(), f"{name}[{b}]: a non-mutual {k} is not 0"
            if (~zero).any():
                ratios[k] = max(ratios.get(k, 0.0), (e[~zero] / sb[ok][~zero]).max().item())
    return ratios


def ties_bitwise(t, got):
    """The planted duplicates are exact ties in what was written, whole columns / rows."""
    la = got["la"][0]
    for _, j1, j2 in t["jt"]:
        assert torch.equal(la[:-1, j1], la[:-1, j2])
    for _, i1, i2 in t["it"]:
        assert torch.equal(la[i1, :-1], la[i2, :-1])
