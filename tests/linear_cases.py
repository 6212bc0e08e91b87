"""The cases of the kernel-level linear tests (test_gpu_linear.py, test_linear_host.py), the seeded
inputs they run on, and the launcher conditions that send each case to its kernel instantiation.

Every case names the path of csrc/gemm_h3.hip / gemm.hip it is there for ("why").  Which instantiation
a case runs follows from its shape and the LG_GEMM_TILE / LG_GEMM_KSPLIT overrides alone;
test_linear_host.py::test_cases_reach_their_routes -- no GPU -- reads the dispatch constants out of
gemm_h3.hip and recomputes the route of every case and override, so moving a threshold fails there
and names the case to re-pick.
"""
import math
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs566-project-lightglue_amd", "csrc")

# B = 2, M0 = 160, N0 = 128 over R = 576 rows: segment 1 (160 rows of capacity, none live) holds
# whole dead 64-row tiles (the early exit), segment 2 (5 of 128 live) a mostly dead live tile
MASK = dict(B=2, M0=160, N0=128, cnt=[160, 0, 5, 128], sel=None, sel_eq=0)
MASK_SEL = dict(MASK, sel=[1, 0], sel_eq=1)  # pair 1 frozen on top


def _case(name, why, epi="store", R=300, K0=256, K=256, Nout=256, **kw):
    c = dict(name=name, why=why, epi=epi, R=R, K0=K0, K=K, Nout=Nout, bias=True, res=False, res2_row0=None, y2_row0=None,
             fp32=True, planes=False, relu=0, out_scale=1.0, a0_scale=1.0, a1_scale=1.0, mask=None, poison=0,
             head=None, rotary=True, qk_scale=1.0, q_given=True, seed=1)
    c.update(kw)
    return c


_FFN3 = dict(R=576, K0=512, K=512, Nout=256, res=True, res2_row0=130, y2_row0=130, planes=True)
_LN = dict(epi="ln_gelu", R=200, K0=256, K=512, Nout=512, fp32=False, planes=True)
_QKV = dict(epi="qkv_rot", R=230, K0=256, K=256, Nout=768, head=(2, 70, 45), fp32=False)
_CROSS = dict(epi="cross_qkv", R=230, K0=256, K=256, Nout=512, head=(2, 70, 45), fp32=False, qk_scale=64.0 ** -0.25)

CASES = [
    _case("store_plain", "bias, no residual, fp32 rows; R = 300 leaves a partial 256-, 128- and 64-row last tile", seed=1),
    _case("store_ffn3", "ffn.3 of layer 0: res + res2 and Y + Y2 switching at row 130 (no multiple of 8, 32 or 64), fp32 "
          "rows and planes together", seed=2, **dict(_FFN3, R=300)),
    _case("store_planes_only", "Y null, res null, planes only, relu, out_scale 0.25: the !fp32_pass branch of the plane "
          "pass", seed=3, fp32=False, planes=True, relu=1, out_scale=0.25),
    _case("store_relu_res", "residual, then ReLU (SuperGlue's order), fp32 rows", seed=4, res=True, relu=1),
    _case("cat_k[256|512]", "A = [A0 | A1], the ffn.0 shape: under KSPLIT = 4 the seam is a group boundary", seed=5,
          K0=256, K=512, planes=True),
    _case("cat_k[96|256]", "A = [A0 | A1], seam at k-tile 3: inside group 1 (k-tiles 2, 3) under KSPLIT = 4", seed=6,
          K0=96, K=256, planes=True),
    _case("single_ktile[32]", "K = 32: the pipeline's prologue only, every KSPLIT request falls back to 1", seed=7, K0=32,
          K=32),
    _case("single_ktile[64]", "K = 64: a KSPLIT = 4 request falls back to 2", seed=8, K0=64, K=64),
    _case("row_mask", "store_ffn3's epilogue under a row mask: whole dead 64-row tiles (early exit), a mostly dead live "
          "tile, stale A rows", seed=9, mask=MASK, poison=1, **_FFN3),
    _case("row_mask_sel", "the same with pair 1 frozen (sel = [1, 0], sel_eq = 1)", seed=9, mask=MASK_SEL, poison=1,
          **_FFN3),
    _case("ln_gelu", "ffn.0 + LayerNorm + GELU: partial 128- and 64-row tile, a near-constant row (eps matters), a 1e4 "
          "outlier row, stale padding rows", seed=10, poison=1, **_LN),
    _case("ln_gelu_mask", "the same under the row-mask layout (R = 576)", seed=11, mask=MASK, poison=1, **dict(_LN, R=576)),
    _case("qkv_rot", "Wqkv + rotary + head-major scatter, ragged M != N", seed=12, **_QKV),
    _case("qkv_plain", "cosb null: SuperGlue's plain q / k / v", seed=12, rotary=False, **_QKV),
    _case("qkv_rot_big", "inputs at 3e5: keys past the fp16 range (E[k] > 0), the values' two-sided exponent positive",
          seed=13, a0_scale=3e5, **_QKV),
    _case("qkv_rot_small_v", "inputs at 1e-6: the values are their bias, the two-sided exponent far below zero", seed=14,
          a0_scale=1e-6, **_QKV),
    _case("cross_qkv", "to_qk / to_v, qk * 64^-0.25 as fp32 rows and planes", seed=15, **_CROSS),
    _case("cross_qkv_planes", "q null: qk leaves only as planes (the attention's q_planes route)", seed=15, q_given=False,
          **_CROSS),
]
# cat_k_exponents: the two halves get different, non-zero range exponents (or one of them zero)
for _k0, _k, _sd in ((256, 512, 20), (96, 256, 23)):
    for _s0, _s1 in ((3e5, 5e6), (3e5, 1.0), (1.0, 3e5)):
        CASES.append(_case(f"cat_k_exponents[{_k0}|{_k},{_s0:g},{_s1:g}]", "E[a0] != E[a1]: the 2^(e0-e1) rescale at the "
                           "A0|A1 seam, in the loop or after a group that saw only A0 tiles", seed=_sd, K0=_k0, K=_k,
                           planes=True, a0_scale=_s0, a1_scale=_s1))
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every launch shape the env overrides reach (LG_GEMM_TILE, LG_GEMM_KSPLIT); None = not set
STORE_LAUNCHES = [("big", None), ("medium", None), ("small", "1"), ("small", "2"), ("small", "4")]
# ln_gelu: (LG_GEMM_TILE, ln_route)
LN_LAUNCHES = [("big", 0), ("small", 0), ("small", 1)]


# ------------------------------------------------------------------------------------ inputs
def head_perm_row(t, h, j, epi):
    """The reference-layout row of packed projection row c' = t*256 + h*64 + j (lightglue_api.cpp head_perm):
    j < 32 -> dim 2j, j >= 32 -> dim 2(j-32)+1; Wqkv row = h*192 + dim*3 + t, to_qk / to_v row = h*64 + dim."""
    dim = 2 * j if j < 32 else 2 * (j - 32) + 1
    return h * 192 + dim * 3 + t if epi == "qkv_rot" else t * 256 + h * 64 + dim


def packed_order(epi, H=4):
    """perm with W_packed = W_natural[perm] (natural: Wqkv [768][K] rows h*192 + dim*3 + t; cross: to_qk rows
    h*64 + dim stacked on to_v's)."""
    T = 3 if epi == "qkv_rot" else 2
    return torch.tensor([head_perm_row(t, h, j, epi) for t in range(T) for h in range(H) for j in range(64)])


def live_rows(case):
    """bool [R]: row_live of kernels.h for the case's mask."""
    R, m = case["R"], case["mask"]
    live = torch.ones(R, dtype=torch.bool)
    if not m:
        return live
    B, M0, N0 = m["B"], m["M0"], m["N0"]
    for r in range(R):
        if r < B * M0:
            s, local = r // M0, r % M0
        else:
            s, local = B + (r - B * M0) // N0, (r - B * M0) % N0
        ok = local < m["cnt"][s]
        if ok and m["sel"] is not None:
            ok = m["sel"][s if s < B else s - B] == m["sel_eq"]
        live[r] = ok
    return live


def build_inputs(case):
    """Seeded fp32 CPU tensors of a case (mixed-sign Gaussians; W ~ 1/sqrt(K) so outputs are O(1))."""
    g = torch.Generator().manual_seed(1000 + case["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    R, K0, K, Nout = case["R"], case["K0"], case["K"], case["Nout"]
    t = {}
    A = rn(R, K)
    W = rn(Nout, K) / math.sqrt(K)
    t["bias"] = 0.5 * rn(Nout) if case["bias"] else None
    if case["epi"] == "ln_gelu":
        # a constant bias: a row of tiny A then has near-constant pre-activations (LayerNorm is shift-invariant,
        # a dropped bias block still moves its columns by 0.37)
        t["bias"] = torch.full((Nout,), 0.37)
        A[7] = 1e-3 * rn(K)  # (A W^T)[7] ~ N(0, 1e-6): variance ~1e-6 < eps
        w0 = W[100].double()
        A[93] = (1e4 * w0 / (w0 @ w0)).float()  # pre-activation [93, 100] = 1e4
        t["ln_g"] = 1.0 + 0.3 * rn(Nout)
        t["ln_b"] = 0.3 * rn(Nout)
    if case["head"]:
        B, M, N = case["head"]
        assert B * (M + N) == R
        t["W_nat"], t["bias_nat"] = W, t["bias"]  # natural (reference) row order
        perm = packed_order(case["epi"])
        W, t["bias"] = W[perm].contiguous(), t["bias"][perm].contiguous()
        if case["rotary"] and case["epi"] == "qkv_rot":
            ang = 6.283185307179586 * torch.rand(R, 32, generator=g, dtype=torch.float64)
            t["cos"], t["sin"] = ang.cos().float(), ang.sin().float()
    t["A0"] = (A[:, :K0] * case["a0_scale"]).contiguous()
    t["A1"] = (A[:, K0:] * case["a1_scale"]).contiguous() if K0 < K else None
    t["W"] = W.contiguous()
    if case["res"]:
        res = rn(R, Nout)
        r0 = case["res2_row0"]
        t["res"], t["res2"] = (res[:r0].contiguous(), res[r0:].contiguous()) if r0 is not None else (res, None)
    t["live"] = live_rows(case)
    return t


# ------------------------------------------------------------------------------------ routes
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: gemm_h3.hip no longer reads as /{pattern}/ -- update tests/linear_cases.py"
    return m


def parsed():
    """The constants of gemm_h3's dispatch, read from the source text."""
    src, common = _src("gemm_h3.hip"), _src("common.h")
    t = {"TB": int(_one(r"constexpr int TB = (\d+);", src, "TB").group(1)),
         "kKB": int(_one(r"constexpr int kKB = (\d+);", common, "kKB").group(1))}
    t["BIG_MIN"] = int(_one(r"if \(big_tiles >= (\d+)\) return TILE_BIG;", src, "gemm_tile_for").group(1))
    m = _one(r"return (\d+) \* big_tiles >= (\d+) \? TILE_MEDIUM : TILE_SMALL;", src, "gemm_tile_for")
    t["MED_MUL"], t["MED_MIN"] = int(m.group(1)), int(m.group(2))
    t["SMALL_LT"] = int(_one(r"o == TILE_SMALL \|\| \(o == TILE_AUTO && big_tiles < (\d+)\)", src, "use_small_tiles").group(1))
    _one(r"int ksplit = 4;", src, "default k-split")
    _one(r"if \(ksplit >= 4 && a\.K >= 4 \* kKB\) return gemm_h3_launch<64, 2, 64, 64, 4>", src, "KSPLIT 4 fallback")
    _one(r"if \(ksplit >= 2 && a\.K >= 2 \* kKB\) return gemm_h3_launch<64, 4, 64, 64, 2>", src, "KSPLIT 2 fallback")
    _one(r"return gemm_h3_launch<64, 4, 64, 64>\(a, epi, st\);", src, "KSPLIT 1")
    _one(r"case TILE_MEDIUM: return gemm_h3_launch<128, 2, 128, 64>", src, "medium tile")
    m = _one(r"#define LG_GEMM_H3_TILE (\d+), (\d+)", src, "big tile")
    t["BIG_BM"] = int(m.group(1))
    _one(r"if \(use_small_tiles\(\(a\.R \+ 127\) / 128\)\) return gemm_h3_ln_launch<64, 64>\(a, st\);", src, "LN small tile")
    _one(r"return use_small_tiles\(\(R \+ 127\) / 128\) && gemm_tile_override\(\) != TILE_BIG;", src, "gemm_h3_ln_split")
    _one(r"template <int WN, int BM = 128>\nhipError_t gemm_h3_ln_launch", src, "LN big tile")
    _one(r"if \(kt == nk0 && e0 != e1\) scale_acc", src, "in-loop seam rescale")
    _one(r"if \(KS > 1 && ke <= nk0 && e0 != e1\) scale_acc", src, "after-loop seam rescale")
    _one(r"const int kb = KS > 1 \? \(ks \* nk\) / KS : 0, ke = KS > 1 \? \(\(ks \+ 1\) \* nk\) / KS : nk;", src, "k-split ranges")
    return t


def store_route(t, R, K, Nout, tile=None, ksplit=None):
    """(BM, KS) of gemm_h3's EPI_STORE / QKV launch for a shape under the overrides."""
    big_tiles = ((R + t["TB"] - 1) // t["TB"]) * (Nout // t["TB"])
    if tile is None:
        tile = "big" if big_tiles >= t["BIG_MIN"] else "medium" if t["MED_MUL"] * big_tiles >= t["MED_MIN"] else "small"
    if tile == "big":
        return t["BIG_BM"], 1
    if tile == "medium":
        return 128, 1
    req = 4 if ksplit is None else int(ksplit)
    if req >= 4 and K >= 4 * t["kKB"]:
        return 64, 4
    if req >= 2 and K >= 2 * t["kKB"]:
        return 64, 2
    return 64, 1


def ln_route(t, R, tile=None):
    """BM of the fused EPI_LN_GELU launch, and whether the forward would take the split route."""
    small = tile == "small" or (tile is None and (R + 127) // 128 < t["SMALL_LT"])
    return (64 if small else 128), (small and tile != "big")


def ksplit_groups(t, K0, K, KS):
    """[(kb, ke)] per k-split group and nk0 (the seam's k-tile)."""
    nk, nk0 = K // t["kKB"], K0 // t["kKB"]
    return [((s * nk) // KS, ((s + 1) * nk) // KS) for s in range(KS)], nk0
