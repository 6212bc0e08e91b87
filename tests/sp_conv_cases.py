"""Cases of the kernel-level SuperPoint convolution tests (test_sp_conv_host.py, test_gpu_sp_conv.py).

A case is a dict: B, H, W, Cin, Cout, pool, aff (None or the kind of post-ReLU scale), xs (input
scale), bias / wmode (range cases), conv1a (then Cin is the image's channel count and `img` its
content).  The seam cases take their batch size from the CU count of the device they are meant for
(`case(name, cus)`): a workgroup of the persistent halo kernel walks a second and third tile only
when there are more than twice as many tiles as CUs.

tile_counts restates the tile walk of sp_conv3x3_halo_kernel (superpoint.hip: G, nx, t_begin, t_end,
T) so that both the CPU and the GPU test can assert that the seam cases really reach T >= 3.
"""
import zlib

import torch

AFF_KINDS = ("mixed", "neg", "zeros", "wide")
SEAM_HW = 56  # 4 x 4 tiles of 16 x 16 per image, the last row and column of tiles partial (8 pixels)


def _c(name, B, H, W, Cin, Cout, pool=0, aff=None, xs=1.0, bias=None, wmode=None, conv1a=0, img="unit", seam=False):
    return dict(name=name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, pool=pool, aff=aff, xs=xs, bias=bias, wmode=wmode,
                conv1a=conv1a, img=img, seam=seam)


def _both(name, *shape, **kw):
    return [_c(name, *shape, pool=0, **kw), _c(name + "+pool", *shape, pool=1, **kw)]


CASES = []
# ---- small and partial tiles
CASES += [_c("b1_1x1_32to64", 1, 1, 1, 32, 64)]
CASES += _both("b1_2x2_32to64", 1, 2, 2, 32, 64)
CASES += _both("b2_17x33_64to64", 2, 17, 33, 64, 64)   # a 1-pixel overhang in both axes, two images
CASES += _both("b1_19x21_64to128", 1, 19, 21, 64, 128)  # odd sizes: the pool floor drops a row and a column
CASES += _both("b3_16x16_32to64", 3, 16, 16, 32, 64)   # exactly one tile per image
# ---- channel routing
CASES += _both("b1_24x40_32to192", 1, 24, 40, 32, 192)   # BN = 64, num_n = 3; CB = 1
CASES += _both("b1_24x40_128to256", 1, 24, 40, 128, 256)  # BN = 128, num_n = 2, CB = 4
CASES += _both("b1_24x40_64to128", 1, 24, 40, 64, 128)
CASES += _both("b1_24x40_128to512", 1, 24, 40, 128, 512)  # [convPa | convDa]: Nh = 512 in superpoint_api.cpp
# ---- affine (the open model's blocks)
for _k in AFF_KINDS:
    CASES += _both(f"b2_17x33_64to64_aff_{_k}", 2, 17, 33, 64, 64, aff=_k)
    CASES += _both(f"b1_19x21_64to128_aff_{_k}", 1, 19, 21, 64, 128, aff=_k)
# ---- ranges
CASES += _both("b2_17x33_64to64_x3e5", 2, 17, 33, 64, 64, xs=3e5)
CASES += _both("b2_17x33_64to64_x1e-6", 2, 17, 33, 64, 64, xs=1e-6)
CASES += _both("b2_17x33_64to64_allzero", 2, 17, 33, 64, 64, bias=-1e3)
CASES += _both("b2_17x33_64to64_wchan1e4", 2, 17, 33, 64, 64, wmode="chan1e4")
# ---- tile seams (B from the CU count; B = 0 here)
CASES += _both("seam_32to64", 0, SEAM_HW, SEAM_HW, 32, 64, seam=True)      # BN = 64
CASES += [_c("seam_32to64_aff", 0, SEAM_HW, SEAM_HW, 32, 64, aff="mixed", seam=True)]
CASES += _both("seam_32to128", 0, SEAM_HW, SEAM_HW, 32, 128, seam=True)    # BN = 128
CASES += [_c("seam_64to256_aff+pool", 0, SEAM_HW, SEAM_HW, 64, 256, pool=1, aff="mixed", seam=True)]  # num_n = 2
# ---- conv1a
for _C in (1, 3):
    for _B, _H, _W in ((1, 1, 1), (2, 17, 33), (1, 40, 56)):
        for _a in (None, "mixed"):
            CASES += [_c(f"conv1a_c{_C}_b{_B}_{_H}x{_W}" + ("_aff" if _a else ""), _B, _H, _W, _C, 64, aff=_a, conv1a=1)]
    CASES += [_c(f"conv1a_c{_C}_0_1_255", 2, 17, 33, _C, 64, conv1a=1, img="0_1_255")]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CONV_NAMES = [c["name"] for c in CASES if not c["conv1a"]]
CONV1A_NAMES = [c["name"] for c in CASES if c["conv1a"]]
SEAM_NAMES = [c["name"] for c in CASES if c["seam"]]


def halo_tiles(c):
    """(BN, num_n, ntiles) of sp_conv3x3_halo_kernel for a case."""
    BN = 128 if c["Cout"] % 128 == 0 else 64
    num_n = c["Cout"] // BN
    return BN, num_n, c["B"] * ((c["H"] + 15) // 16) * ((c["W"] + 15) // 16) * num_n


def tile_counts(ntiles, cus):
    """T of every workgroup of the halo kernel's grid (superpoint.hip: one workgroup per CU, each of
    G = min(8, grid) tile ranges walked by the workgroups blockIdx % G == xcd with stride nx)."""
    grid = min(ntiles, cus)
    G = min(8, grid)
    out = []
    for blk in range(grid):
        xcd, local = blk % G, blk // G
        nx = (grid - xcd + G - 1) // G
        t_begin, t_end = ntiles * xcd // G, ntiles * (xcd + 1) // G
        out.append((t_end - t_begin - local + nx - 1) // nx if local < t_end - t_begin else 0)
    return out


def case(name, cus=256):
    """The case with its batch size filled in: a seam case gets the smallest B with ntiles > 2 cus + 64."""
    c = dict(BY_NAME[name])
    if c["seam"]:
        c["B"] = 1
        per_image = halo_tiles(c)[2]
        c["B"] = (2 * cus + 64) // per_image + 1
    return c


def build_inputs(c):
    """fp32 CPU tensors of a case: x (NHWC rows, or the NCHW image for conv1a), w, bias, s, t."""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    t = {}
    if c["conv1a"]:
        if c["img"] == "0_1_255":  # an unnormalised image: pixels at exactly 0, 1 and 255
            t["x"] = torch.tensor([0.0, 1.0, 255.0])[torch.randint(0, 3, (B, Cin, H, W), generator=g)]
        else:
            t["x"] = torch.rand(B, Cin, H, W, generator=g)
        t["w"] = r(64, 1, 3, 3) / 3.0
    else:
        t["x"] = r(B, H, W, Cin) * c["xs"]
        t["w"] = r(Cout, Cin, 3, 3) / (9.0 * Cin) ** 0.5
        if c["wmode"] == "chan1e4":
            t["w"][Cout // 2 + 1] *= 1e4
    t["bias"] = torch.full((Cout,), float(c["bias"])) if c["bias"] is not None else r(Cout) * 0.25 * c["xs"]
    t["s"] = t["t"] = None
    if c["aff"]:
        kind = c["aff"]
        s = r(Cout)
        if kind == "neg":
            s = -(0.5 + torch.rand(Cout, generator=g))
        elif kind == "zeros":
            s[::3] = 0.0
        elif kind == "wide":
            s = torch.sign(s) * 10.0 ** torch.linspace(-3.0, 3.0, Cout)[torch.randperm(Cout, generator=g)]
        t["s"], t["t"] = s.contiguous(), r(Cout) * 0.5
    return {k: (v.float().contiguous() if v is not None else None) for k, v in t.items()}
