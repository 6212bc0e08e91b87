#!/usr/bin/env python3
"""Generate the line ground-truth fixtures by running the REAL reference.

Run from the repo root where the reference checkout exists (it does not on the GPU box)::

    python tests/golden/make_line_gt_golden.py

Imports the reference's ``gluefactory/geometry/gt_generation.py`` through the shim of
make_gt_golden.py and runs ``gt_line_matches_from_homography`` in fp32 and in fp64 on inputs from NumPy
PCG64 recipes, with ``linear_sum_assignment`` wrapped to record the cost matrices it is handed and the
``assignation`` it returns.  The counts and the out_of flags, which the reference does not return, come
from its own ``sample_pts`` / ``warp_points_torch`` / ``torch_perp_dist`` called as :450-488 calls them
(``torch.einsum`` wrapped to record ``rotated``); they are checked against the recorded cost matrices
(cost == -cnt0 * cnt1t wherever it is not 1e6).  Writes ``tests/golden/line_gt/line_gt_*.npz``: the
inputs, the fp32 ``positive`` (index triples), ``m0``, ``m1``, counts, flags, cost (int32), assignation
and the margins.

Near-tie gating (random cases; the exact ones have none), per direction.  ``e`` is the reference's own
largest |fp32 - fp64| of rot_x and rot_y over samples within 4 dist_th of a segment, tau = 4 e; a
sample is undecidable within tau of any of the three comparisons; a count may lie in
[decided close, decided close + undecidable] (tests/line_gt_ref.py:margins).  For the out_of flags the
same with e_p = max |fp32 - fp64| of the warped samples against the image borders.  Asserted here
(change a failing seed or recipe, never the cap): entries with an undecidable sample <= 3 % of the
entries with a nonzero count, per direction; undecidable out_of flags <= 3 % of the lines; the
reference's fp32 and fp64 counts differ only inside undecidable entries.

Seeds.  The forward direction stays at 0-0.5 % for every seed tried; the inverse direction depends on
torch's fp32 ``inverse`` of the particular H (e from 2e-4 to 1.2e-2 px), and seeds whose share of
undecidable entries exceeded the cap were rejected -- REJECTED below lists them with the share seen.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import line_gt_ref as ref  # noqa: E402
from make_gt_golden import install_shim  # noqa: E402

CAP = 0.03
W, Hh = 640, 480

# seeds tried and not used: (n0, n1, recipe variant, seed) -> share of undecidable entries in the inverse
# direction (num_close_pts0), all above the cap; their fp32 inverse is off by 2e-3 to 1.2e-2 px
REJECTED = {
    (128, 128, "perspective", 34): 0.132, (128, 128, "perspective", 35): 0.032, (128, 128, "perspective", 36): 0.043,
    (96, 130, "perspective", 34): 0.137, (96, 130, "perspective", 36): 0.041,
    (130, 96, "affine", 38): 0.038,
    (300, 257, "perspective", 36): 0.034, (300, 257, "perspective", 39): 0.033,
    (250, 250, "perspective", 36): 0.036, (250, 250, "perspective", 38): 0.050, (250, 250, "perspective", 39): 0.030,
    (250, 250, "perspective", 40): 0.033,
}


def random_case(seed, B, n0, n1, affine=False):
    """H = I + N(0, 0.05) on the 2x2 block, a shift within +-30 px, N(0, 1e-4) on the last row (zero for
    an affine case); segments of 20-200 px in a 640x480 image, some reaching past the border; two thirds
    of image 1 are lines of image 0 warped, with 1.5 px of endpoint noise, the rest random; image 1
    shuffled; about one line in twelve invalid."""
    rng = np.random.Generator(np.random.PCG64(seed))
    size = np.array([W, Hh], float)
    H = np.tile(np.eye(3), (B, 1, 1))
    H[:, :2, :2] += rng.standard_normal((B, 2, 2)) * 0.05
    H[:, :2, 2] = rng.uniform(-30.0, 30.0, (B, 2))
    if not affine:
        H[:, 2, :2] = rng.standard_normal((B, 2)) * 1e-4

    def segments(n):
        a = rng.random((B, n, 2)) * (size + 40.0) - 20.0
        ang = rng.uniform(0, 2 * np.pi, (B, n))
        ln = rng.uniform(20.0, 200.0, (B, n))
        return np.concatenate([a, a + ln[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)], -1)

    l0, l1 = segments(n0), segments(n1)
    nw = min(2 * n1 // 3, n0)
    for b in range(B):
        src = rng.permutation(n0)[:nw]
        p = np.concatenate([l0[b, src].reshape(nw * 2, 2), np.ones((nw * 2, 1))], 1) @ H[b].T
        l1[b, :nw] = (p[:, :2] / p[:, 2:]).reshape(nw, 4) + rng.standard_normal((nw, 4)) * 1.5
        l1[b] = l1[b, rng.permutation(n1)]
    v0, v1 = rng.random((B, n0)) > 1 / 12, rng.random((B, n1)) > 1 / 12
    return l0.astype(np.float32), l1.astype(np.float32), v0, v1, H.astype(np.float32)


def inverse_is_exact(H):
    """The reference's fp32 inverse of a pure shift is the opposite shift, bit for bit."""
    want = H.clone()
    want[..., :2, 2] *= -1
    return torch.equal(torch.inverse(H), want)


def exact_case(seed, B, n0, n1):
    """Axis-aligned integer segments (lengths are integers: exact in fp16), H = I + an integer shift
    whose fp32 inverse by torch is exact.
    Image 1 takes lines of image 0, shifted by H and by small integer offsets across (up to 6 px, on
    either side of dist_th) and along; a quarter of either image repeats earlier lines (ties between
    assignments) or extends them collinearly; starts reach 12 px past the border (clamped lines, some to
    zero length) and the shift pushes others out of the other image; about one line in ten invalid."""
    rng = np.random.Generator(np.random.PCG64(seed))
    w, h = 200, 150
    H = np.tile(np.eye(3), (B, 1, 1))
    for b in range(B):  # torch's fp32 inverse is not exact for every integer shift: draw until it is
        for _ in range(100):
            H[b, :2, 2] = rng.integers(-30, 31, 2)
            if inverse_is_exact(torch.from_numpy(H[b].astype(np.float32))):
                break

    def segments(n):
        a = np.stack([rng.integers(-12, w + 12, (B, n)), rng.integers(-12, h + 12, (B, n))], -1)
        ln = rng.choice([8, 16, 24, 32, 48, 64], (B, n)) * rng.choice([-1, 1], (B, n))
        horiz = rng.random((B, n)) < 0.5
        d = np.where(horiz[..., None], np.stack([ln, 0 * ln], -1), np.stack([0 * ln, ln], -1))
        return np.concatenate([a, a + d], -1).astype(float)

    l0 = segments(n0)
    q = n0 // 4
    l0[:, n0 - q:] = l0[:, :q]  # duplicates in image 0 ...
    ext = l0[:, n0 - q: n0 - q // 2]
    ext[..., 2:] += ext[..., 2:] - ext[..., :2]  # ... half of them extended collinearly to twice the length
    l1 = segments(n1)
    nw = min(3 * n1 // 4, n0)
    for b in range(B):
        src = rng.permutation(n0)[:nw]
        s = l0[b, src].copy()
        horiz = s[:, 1] == s[:, 3]
        across, along = rng.integers(-6, 7, nw), rng.integers(-4, 5, nw)
        off = np.where(horiz[:, None], np.stack([along, across], -1), np.stack([across, along], -1))
        l1[b, :nw] = s + np.tile(off + H[b, :2, 2], 2)
        l1[b, n1 - n1 // 4:] = l1[b, : n1 // 4]  # duplicates in image 1
        l1[b] = l1[b, rng.permutation(n1)]
    v0, v1 = rng.random((B, n0)) > 0.1, rng.random((B, n1)) > 0.1
    return l0.astype(np.float32), l1.astype(np.float32), v0, v1, H.astype(np.float32), (h, w)


CASES = [
    # name, recipe, seed, B, n0, n1, kwargs of the reference call, recipe kwargs
    ("line_gt_exact_b3_n64_n48", exact_case, 21, 3, 64, 48, {}, {}),
    ("line_gt_exact_b1_n48_n64", exact_case, 22, 1, 48, 64, {}, {}),
    ("line_gt_rand_b2_n128_n128", random_case, 32, 2, 128, 128, {}, {}),
    ("line_gt_rand_b2_n96_n130", random_case, 37, 2, 96, 130, {}, {}),
    ("line_gt_rand_b2_n130_n96", random_case, 33, 2, 130, 96, {}, {"affine": True}),
    ("line_gt_rand_b1_n300_n257", random_case, 35, 1, 300, 257, {}, {}),
    ("line_gt_rand_b2_n250_n250", random_case, 37, 2, 250, 250, {"min_visibility_th": 0.5}, {}),
    ("line_gt_rand_p7_b2_n96_n96", random_case, 37, 2, 96, 96,
     {"npts": 7, "overlap_th": 0.5, "min_visibility_th": 0.2}, {}),
]
DEFAULTS = {"npts": 50, "dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.2}


def run_reference(gen, l0, l1, v0, v1, shape, H, kw):
    """The reference's labels with the cost matrices and assignations SciPy saw."""
    seen = []
    real = gen.linear_sum_assignment

    def spy(C):
        out = real(C)
        seen.append((np.array(C, copy=True), np.array(out)))
        return out

    gen.linear_sum_assignment = spy
    try:
        pos, m0, m1 = gen.gt_line_matches_from_homography(l0, l1, v0, v1, shape, shape, H, kw["npts"], kw["dist_th"],
                                                          kw["overlap_th"], kw["min_visibility_th"])
    finally:
        gen.linear_sum_assignment = real
    return pos, m0, m1, np.stack([c for c, _ in seen]), np.stack([a for _, a in seen])


def reference_stage_a(gen, l0, l1, shape, H, kw):
    """:441-488 with the reference's own functions; ``rotated`` recorded from its einsum."""
    h, w = shape[-2:]
    npts, dist_th = kw["npts"], kw["dist_th"]
    B, n0, n1 = l0.shape[0], l0.shape[1], l1.shape[1]
    c0, c1 = ref.clamp_lines(l0.clone(), h, w), ref.clamp_lines(l1.clone(), h, w)
    pts0_1 = gen.warp_points_torch(gen.sample_pts(c0, npts).reshape(B, n0 * npts, 2), H, inverse=False).reshape(B, n0, npts, 2)
    pts1_0 = gen.warp_points_torch(gen.sample_pts(c1, npts).reshape(B, n1 * npts, 2), H, inverse=True).reshape(B, n1, npts, 2)
    out_of0 = ref.outside(pts1_0, h, w).float().mean(dim=-1) >= (1 - kw["min_visibility_th"])
    out_of1 = ref.outside(pts0_1, h, w).float().mean(dim=-1) >= (1 - kw["min_visibility_th"])
    rot = []
    real = torch.einsum

    def spy(*a, **k):
        out = real(*a, **k)
        rot.append(out)
        return out

    torch.einsum = spy
    try:
        d0, ov0 = gen.torch_perp_dist(c0, pts1_0)
        d1, ov1 = gen.torch_perp_dist(c1, pts0_1)
    finally:
        torch.einsum = real
    cnt0 = ((d0 < dist_th) & ov0).sum(dim=-1)
    cnt1t = ((d1 < dist_th) & ov1).sum(dim=-1).transpose(-1, -2)
    rots = [(r[..., 0], r[..., 1]) for r in rot[-2:]]
    return cnt0, cnt1t, out_of0, out_of1, rots, (ref.segment_sizes(c0), ref.segment_sizes(c1)), (pts0_1, pts1_0)


def main():
    gen = install_shim()
    os.makedirs(ref.HERE, exist_ok=True)
    for name, recipe, seed, B, n0, n1, kw, rkw in CASES:
        kw = {**DEFAULTS, **kw}
        exact = recipe is exact_case
        made = recipe(seed, B, n0, n1, **rkw)
        l0, l1, v0, v1, H = made[:5]
        shape = made[5] if exact else (Hh, W)
        t = [torch.from_numpy(x) for x in (l0, l1, v0, v1, H)]
        t64 = [t[0].double(), t[1].double(), t[2], t[3], t[4].double()]
        if exact:
            assert inverse_is_exact(t[4]), "the reference's fp32 inverse of H is not exact"
        pos, m0, m1, cost, assignation = run_reference(gen, *t[:4], (1, 1) + tuple(shape), t[4], kw)
        cnt0, cnt1t, o0, o1, rot32, _, pts32 = reference_stage_a(gen, t[0], t[1], shape, t[4], kw)
        assert pos.dtype == torch.bool and m0.dtype == torch.int64
        # the pieces are the full run's: the recorded cost is -cnt0 * cnt1t wherever it is not 1e6, and
        # the restated stage B turns the counts into the reference's labels
        prod = -(cnt0 * cnt1t).numpy().astype(np.float64)
        assert np.array_equal(cost[cost != 1e6], prod[cost != 1e6]), name
        rb = ref.stage_b(cnt0, cnt1t, o0, o1, t[2], t[3], kw["npts"], kw["overlap_th"])
        assert torch.equal(rb[0], pos) and torch.equal(rb[1], m0) and torch.equal(rb[2], m1), name
        assert np.array_equal(rb[3].numpy().astype(np.float64), cost) and np.array_equal(rb[4].numpy(), assignation), name
        assert int(cnt0.max()) <= 255 and np.array_equal(cost, cost.astype(np.int32))
        out = {"lines0": l0, "lines1": l1, "valid_lines0": v0, "valid_lines1": v1, "H_0to1": H,
               "positive_idx": np.argwhere(pos.numpy()).astype(np.int32), "m0": m0.numpy(), "m1": m1.numpy(),
               "cnt0": cnt0.numpy().astype(np.uint8), "cnt1t": cnt1t.numpy().astype(np.uint8),
               "out_of0": o0.numpy(), "out_of1": o1.numpy(), "cost_i32": cost.astype(np.int32),
               "assignation": assignation.astype(np.int32)}
        meta = {"B": B, "n0": n0, "n1": n1, "seed": seed, "exact": exact, "shape": list(shape), **kw}
        stats = f"positives {len(out['positive_idx'])} m0>-1 {(out['m0'] > -1).sum()} m0==-1 {(out['m0'] == -1).sum()} " \
                f"m0==-2 {(out['m0'] == -2).sum()} out_of {int(o0.sum())}+{int(o1.sum())}"
        if exact:
            r64 = run_reference(gen, *t64[:4], (1, 1) + tuple(shape), t64[4], kw)
            assert torch.equal(r64[0], pos) and torch.equal(r64[1], m0) and torch.equal(r64[2], m1), name
            print(f"{name}: {stats}")
        else:
            c64 = reference_stage_a(gen, t64[0], t64[1], shape, t64[4], kw)
            e0 = ref.rot_error(rot32[0], c64[4][0], c64[5][0], kw["dist_th"])
            e1 = ref.rot_error(rot32[1], c64[4][1], c64[5][1], kw["dist_th"])
            ep1 = float((pts32[0].double() - c64[6][0]).abs().max())  # image-0 lines in image 1 (out_of1)
            ep0 = float((pts32[1].double() - c64[6][1]).abs().max())
            mg = ref.margins(l0, l1, shape, shape, H, kw["npts"], kw["dist_th"], kw["min_visibility_th"], 4 * e0, 4 * e1,
                             4 * ep0, 4 * ep1)
            shares = []
            for k, und, k64 in (("cnt0", "und0", c64[0]), ("cnt1t", "und1t", c64[1])):
                nz = int((out[k] > 0).sum())
                share = int((mg[und] > 0).sum()) / max(nz, 1)
                shares.append(share)
                assert share <= CAP, (name, k, share)
                dec = mg[und] == 0
                assert np.array_equal(out[k][dec], k64.numpy()[dec]), (name, k, "fp32 and fp64 differ on a decided entry")
                lo = mg["lo" + und[3:]].astype(int)
                assert ((out[k] >= lo) & (out[k] <= lo + mg[und])).all(), (name, k)
            uo = (int(mg["und_out_of0"].sum()) + int(mg["und_out_of1"].sum())) / (B * (n0 + n1))
            assert uo <= CAP, (name, "out_of", uo)
            for k, v64 in (("out_of0", c64[2]), ("out_of1", c64[3])):
                dec = ~mg["und_" + k]
                assert np.array_equal(out[k][dec], v64.numpy()[dec]), (name, k)
            out.update(mg)
            meta.update({"e0": e0, "e1": e1, "e_p0": ep0, "e_p1": ep1, "und_share0": shares[0], "und_share1": shares[1],
                         "und_out_of_share": uo})
            print(f"{name}: e0 {e0:.2e} e1 {e1:.2e} e_p {ep0:.2e}/{ep1:.2e} undecidable {shares[0]:.4f}/{shares[1]:.4f} "
                  f"out_of {uo:.4f} decided pairs {int(ref.pair_decided(out, meta).sum())}/{B} {stats}")
        out["meta_json"] = np.array(json.dumps(meta))
        path = os.path.join(ref.HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"  wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
