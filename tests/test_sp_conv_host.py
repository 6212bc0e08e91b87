"""CPU self-checks of the kernel-level SuperPoint convolution tests (no GPU): the bars of sp_conv_ref.py
are reachable by the kernels' arithmetic, they notice deliberate mistakes, and the seam cases make a
workgroup of the persistent halo kernel walk at least three tiles."""
import functools

import pytest
import torch

import sp_conv_cases as sc
import sp_conv_ref as sr


@functools.lru_cache(maxsize=None)
def prepared(name, cus=256):
    c = sc.case(name, cus)
    t = sc.build_inputs(c)
    return c, t, sr.reference(c, t)


# ---------------------------------------------------------------- 1. the bars are reachable
@pytest.mark.parametrize("name", sc.CONV_NAMES)
def test_emulation_meets_the_bars(name):
    c, t, ref = prepared(name)
    for order in (("halo",) if c["seam"] else ("halo", "gather")):
        got, e = sr.emulate(c, t, order=order)
        r = sr.check(ref, got, e["out"])
        print(f"SPCONV-EMU {name} {order} err/bar={r:.3f} exps={e}")
        assert r <= 0.5, f"{name}/{order}: emulation at {r:.3f} of the bar"


@pytest.mark.parametrize("name", sc.CONV1A_NAMES)
def test_conv1a_emulation_meets_the_bars(name):
    c, t, ref = prepared(name)
    got, e = sr.emulate_conv1a(c, t)
    r = sr.check(ref, got, e["out"])
    print(f"SPCONV-EMU {name} err/bar={r:.3f} exps={e}")
    assert r <= 0.5, f"{name}: emulation at {r:.3f} of the bar"


def test_emulated_exponents_are_what_the_cases_claim():
    e = {n: sr.emulate(*prepared(n)[:2])[1] for n in ("b2_17x33_64to64", "b2_17x33_64to64_x3e5", "b2_17x33_64to64_x1e-6",
                                                      "b2_17x33_64to64_allzero", "b2_17x33_64to64_wchan1e4")}
    base = e["b2_17x33_64to64"]
    assert base["out"] == 0
    assert e["b2_17x33_64to64_x3e5"]["in"] - base["in"] in (18, 19) and e["b2_17x33_64to64_x3e5"]["out"] > 0  # log2(3e5) = 18.2
    assert e["b2_17x33_64to64_x1e-6"]["in"] - base["in"] in (-20, -19) and e["b2_17x33_64to64_x1e-6"]["out"] == 0
    assert e["b2_17x33_64to64_allzero"]["out"] == 0
    assert e["b2_17x33_64to64_wchan1e4"]["out"] > 0
    c, t, ref = prepared("b2_17x33_64to64_allzero")
    assert (ref["y"] == 0).all() and (sr.emulate(c, t)[0] == 0).all()


# ---------------------------------------------------------------- 2. the bars notice mistakes
SENSITIVITY = {
    "drop_low_in": ["b2_17x33_64to64", "b1_24x40_128to256"],
    "wrap_rows": ["b2_17x33_64to64", "b1_2x2_32to64+pool"],
    "tile_border_tap": ["b2_17x33_64to64", "b1_19x21_64to128+pool"],
    "swap_cblocks": ["b2_17x33_64to64", "b1_24x40_128to256"],
    "maxpool_neg_scale": ["b2_17x33_64to64_aff_neg+pool", "b1_19x21_64to128_aff_mixed+pool"],
    "partial_tile_unwritten": ["b2_17x33_64to64", "b1_19x21_64to128+pool"],
    "bias_after_affine": ["b2_17x33_64to64_aff_mixed", "b1_19x21_64to128_aff_wide+pool"],
}


@pytest.mark.parametrize("wrong", sr.WRONG)
def test_bars_notice_a_wrong_kernel(wrong):
    """Each wrong variant of the emulation misses the bar on every case listed for it."""
    assert set(SENSITIVITY) == set(sr.WRONG)
    for name in SENSITIVITY[wrong]:
        c, t, ref = prepared(name)
        got, e = sr.emulate(c, t, wrong=wrong)
        r = sr.check(ref, got, e["out"])
        print(f"SPCONV-WRONG {wrong} {name} err/bar={r:.3g}")
        assert r > 1.0, f"{wrong} on {name}: {r:.3f} of the bar goes unnoticed"


# ---------------------------------------------------------------- 3. the tile walk
def test_tile_counts_cover_every_tile_once():
    for ntiles, cus in ((1, 256), (7, 256), (8, 256), (9, 256), (255, 256), (256, 256), (257, 256), (592, 256), (704, 304),
                        (1000, 3), (1000, 8), (1000, 9)):
        grid = min(ntiles, cus)
        G = min(8, grid)
        seen = []
        for blk, T in enumerate(sc.tile_counts(ntiles, cus)):
            xcd, local = blk % G, blk // G
            nx = (grid - xcd + G - 1) // G
            seen += [ntiles * xcd // G + local + k * nx for k in range(T)]
        assert sorted(seen) == list(range(ntiles)), (ntiles, cus)


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("name", sc.SEAM_NAMES)
def test_seam_cases_walk_three_tiles(name, cus):
    c = sc.case(name, cus)
    BN, num_n, ntiles = sc.halo_tiles(c)
    assert ntiles > 2 * cus + 64
    assert max(sc.tile_counts(ntiles, cus)) >= 3
    assert BN == (128 if c["Cout"] % 128 == 0 else 64) and c["H"] % 16 and c["W"] % 16  # partial tiles, seams across images
    # the float64 reference stays affordable
    assert 2 * c["B"] * c["H"] * c["W"] * 9 * c["Cin"] * c["Cout"] < 25e9


def test_case_list_reaches_every_instantiation():
    """(BN, POOL, AFF) of both 3x3 kernels and AFF of conv1a, from the dispatch in sp_conv3x3."""
    seen = {(sc.halo_tiles(sc.case(n))[0], bool(sc.BY_NAME[n]["pool"]), sc.BY_NAME[n]["aff"] is not None) for n in sc.CONV_NAMES}
    assert seen == {(bn, p, a) for bn in (64, 128) for p in (False, True) for a in (False, True)}
    assert {sc.BY_NAME[n]["aff"] is not None for n in sc.CONV1A_NAMES} == {False, True}
    seam = {(sc.halo_tiles(sc.case(n))[0], sc.BY_NAME[n]["aff"] is not None) for n in sc.SEAM_NAMES}
    assert {bn for bn, _ in seam} == {64, 128} and {a for _, a in seam} == {False, True}


# ---------------------------------------------------------------- 4. the dense heads' references
def test_scores_reference_unfolds_by_one_hot():
    B, Hc, Wc = 2, 3, 5
    logits = torch.full((B * Hc * Wc, 65), -1e4)
    ch = torch.arange(B * Hc * Wc) % 64
    logits[torch.arange(B * Hc * Wc), ch] = 0.0
    p, _ = sr.scores_reference(logits, B, Hc, Wc)
    for cell in range(B * Hc * Wc):
        b, y, x = cell // (Hc * Wc), cell % (Hc * Wc) // Wc, cell % Wc
        blk = p[b, 8 * y:8 * y + 8, 8 * x:8 * x + 8]
        assert blk[ch[cell] // 8, ch[cell] % 8] == 1.0 and blk.sum() == 1.0
