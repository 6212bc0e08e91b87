#!/usr/bin/env python3
"""Generate the pose-and-depth line ground-truth fixtures by running the REAL reference.

Run from the repo root where the reference checkout exists (it does not on the GPU box)::

    python tests/golden/make_line_gt_depth_golden.py

Imports the reference's ``gluefactory/geometry/gt_generation.py`` and ``wrappers.py`` through the shim of
make_gt_golden.py and runs ``gt_line_matches_from_pose_depth`` in fp32 and in fp64 on inputs from NumPy
PCG64 recipes, with ``linear_sum_assignment`` wrapped to record the cost matrices it is handed and the
``assignation`` it returns.  The counts, the out_of and depth-ignore flags and the per-line visible
counts, which the reference does not return, come from its own ``sample_pts`` / ``sample_depth`` /
``project`` / ``torch_perp_dist`` called as :250-352 calls them (``torch.einsum`` wrapped to record
``rotated``); they are checked against the recorded cost matrices (cost == -cnt0 * cnt1t wherever it is
not 1e6) and, through the restated stage B, against the labels of the full run.  Writes
``tests/golden/line_gt_depth/line_gtd_*.npz``: the inputs, the fp32 ``positive`` (index triples), ``m0``,
``m1``, counts, flags, per-line visible counts, cost (int32), assignation and the margins.

The exact cases: every step of the sampling is exact, so the reference's fp32 and fp64 runs must agree bit
for bit in the labels and in every stage-A array (asserted; change the recipe, not the assertion).

The random cases are gated (tests/line_gt_depth_ref.py:margins).  Every tolerance is 4 x the largest
deviation between the fp32 and the fp64 run for that quantity: rot_x / rot_y near a segment and the
projected coordinates from the reference's own two runs; z, the camera's image bound and r^2 - limit from
the restated chain (tests/gt_depth_ref.py, asserted here to give the reference's stage-A arrays bit for
bit in both precisions, because the reference does not hand out those intermediates); the sample
coordinates for the depth-validity margin.  Asserted here (change a failing seed or recipe, never the
cap): entries with an undecidable sample <= 3 % of the entries with a nonzero count, per direction;
undecidable lines <= 3 % of the lines; the reference's fp32 and fp64 runs agree on everything decidable;
every random case has at least 10 positives, 3 depth-ignored lines and 3 out_of lines, and at least one
pair without anything undecidable.  REJECTED lists the seeds tried that broke one of these.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gt_depth_ref as gd  # noqa: E402
import line_gt_depth_ref as ref  # noqa: E402
import line_gt_ref as lr  # noqa: E402
from make_gt_golden import install_shim  # noqa: E402

CAP = 0.03
W, Hh = 256, 192

# seeds tried and not used: case -> seeds.  None of them broke a cap (their shares of undecidable entries
# were 0.1-0.6 %, of undecidable lines 0-0.8 %); each left no pair without an undecidable entry, and the
# end-to-end test wants one whose labels must be the reference's.
REJECTED = {
    "line_gtd_rand_b2_n96_n130_d0": (41, 51, 61, 71),
    "line_gtd_rand_b2_n130_n96_d2": (42, 52, 62, 72, 82, 92),
    "line_gtd_rand_b1_n128_n128_d4": (43, 53, 63, 73, 83, 93),
}


def random_case(seed, B, n0, n1, n_dist=0, image=None):
    """The scene of gt_depth_ref.plane_scene on 256 x 192 maps.  Lines of image 0: segments of 20-120 px,
    some reaching past the border, one in ten a short segment within 6 px of a border (candidates for
    out_of).  Two thirds of image 1 are lines of image 0 whose (clamped) endpoints the scene's own fp64
    projection carries over, plus 1.5 px of noise; the rest random like image 0; image 1 shuffled; about
    one line in twelve invalid."""
    g = gd.plane_scene(seed, B, 8, 8, n_dist=n_dist, width=W, height=Hh)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    size = np.array([W, Hh], float)

    def segments(n):
        a = rng.random((B, n, 2)) * (size + 30.0) - 15.0
        ang = rng.uniform(0, 2 * np.pi, (B, n))
        ln = rng.uniform(20.0, 120.0, (B, n))
        s = np.concatenate([a, a + ln[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)], -1)
        nb = n // 10
        for b in range(B):
            for k in range(nb):  # along a border, within 6 px of it
                side, off, pos, ln = rng.integers(0, 4), rng.uniform(0.5, 6.0), rng.uniform(0.1, 0.8), rng.uniform(8.0, 20.0)
                if side < 2:
                    x = off if side == 0 else W - 1 - off
                    y = pos * Hh
                    s[b, k] = [x, y, x + rng.uniform(-1, 1), y + ln]
                else:
                    y = off if side == 2 else Hh - 1 - off
                    x = pos * W
                    s[b, k] = [x, y, x + ln, y + rng.uniform(-1, 1)]
            s[b] = s[b, rng.permutation(n)]
        return s

    l0, l1 = segments(n0), segments(n1)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).double()  # noqa: E731
    ends = np.clip(l0.astype(np.float32).astype(np.float64).reshape(B, n0 * 2, 2), 0.0, size - 1.0)
    d, v = gd.sample_depth(t64(ends), t64(g["depth0"]))
    p, vis = gd.project(t64(ends), d, None, t64(g["camera0"]), t64(g["camera1"]), t64(g["T_0to1"]), v)
    p, vis = p.numpy().reshape(B, n0, 4), vis.numpy().reshape(B, n0, 2).all(-1)
    nw = min(2 * n1 // 3, n0)
    for b in range(B):
        src = np.nonzero(vis[b])[0]
        src = src[rng.permutation(len(src))][:nw]
        l1[b, :len(src)] = p[b, src] + rng.standard_normal((len(src), 4)) * 1.5
        l1[b] = l1[b, rng.permutation(n1)]
    v0, v1 = rng.random((B, n0)) > 1 / 12, rng.random((B, n1)) > 1 / 12
    g = {k: g[k] for k in ("depth0", "depth1", "camera0", "camera1", "T_0to1", "T_1to0")}
    g.update({"lines0": l0.astype(np.float32), "lines1": l1.astype(np.float32), "valid_lines0": v0, "valid_lines1": v1})
    return g, (image or (Hh, W)), (image or (Hh, W))


def exact_case(seed, B, n0, n1, S=512, lengths=(8, 16, 24, 32, 48, 64)):
    """S x S pinhole cameras (S = 512) with f = c = S / 2 = 256, depth 4 except zero rectangles, R = I,
    t = (0.125, -0.0625, 0): a shift of (8, -4) px (S / 64, -S / 128; the small-shape tests use other
    powers of two and other lengths).  Axis-aligned integer segments with npts = 33: every
    step is a multiple of 1/32.  Image 1 takes lines of image 0, shifted by the pose and by small integer
    offsets across (up to 6 px, on either side of dist_th) and along; a quarter of either image repeats
    earlier lines (ties between assignments) or extends them collinearly; starts reach 12 px past the
    border (clamped lines, some along x = 0 or y = 0 where the zero padding enters, some to zero length)
    and the shift takes lines near the border out of the other image.  Zero rectangles per map: over whole
    lines (depth-ignored), over half of a line (fewer visible samples: another per-line threshold), with an
    edge on a line's own row or column (the bilinear value is NaN and the nearest sample decides), and a
    few anywhere.  About one line in ten invalid."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = np.tile(np.array([S, S, S / 2, S / 2, S / 2, S / 2], float), (B, 1))
    T01 = np.tile(np.concatenate([np.eye(3).reshape(9), [0.125, -0.0625, 0.0]]), (B, 1))
    T10 = np.tile(np.concatenate([np.eye(3).reshape(9), [-0.125, 0.0625, 0.0]]), (B, 1))
    shift = np.array([S / 64, -S / 128])

    def segments(n):
        a = np.stack([rng.integers(-12, S + 12, (B, n)), rng.integers(-12, S + 12, (B, n))], -1)
        ln = rng.choice(list(lengths), (B, n)) * rng.choice([-1, 1], (B, n))
        horiz = rng.random((B, n)) < 0.5
        d = np.where(horiz[..., None], np.stack([ln, 0 * ln], -1), np.stack([0 * ln, ln], -1))
        return np.concatenate([a, a + d], -1).astype(float)

    l0 = segments(n0)
    q = n0 // 4
    l0[:, n0 - q:] = l0[:, :q]
    ext = l0[:, n0 - q: n0 - q // 2]
    ext[..., 2:] += ext[..., 2:] - ext[..., :2]
    l1 = segments(n1)
    nw = min(3 * n1 // 4, n0)
    for b in range(B):
        src = rng.permutation(n0)[:nw]
        s = l0[b, src].copy()
        horiz = s[:, 1] == s[:, 3]
        across, along = rng.integers(-6, 7, nw), rng.integers(-4, 5, nw)
        off = np.where(horiz[:, None], np.stack([along, across], -1), np.stack([across, along], -1))
        l1[b, :nw] = s + np.tile(off + shift, 2)
        l1[b, n1 - n1 // 4:] = l1[b, : n1 // 4]
        l1[b] = l1[b, rng.permutation(n1)]
    depth = np.full((2, B, S, S), 4.0)
    for k, ln in ((0, l0), (1, l1)):
        for b in range(B):
            n = ln.shape[1]
            c = np.clip(ln[b], 0, S - 1).astype(int)
            x0, x1 = np.minimum(c[:, 0], c[:, 2]), np.maximum(c[:, 0], c[:, 2])
            y0, y1 = np.minimum(c[:, 1], c[:, 3]), np.maximum(c[:, 1], c[:, 3])
            pick = rng.permutation(n)
            for i in pick[:4]:  # the whole line
                depth[k, b, max(y0[i] - 2, 0): y1[i] + 3, max(x0[i] - 2, 0): x1[i] + 3] = 0.0
            for i in pick[4:9]:  # the half towards the second endpoint
                mx, my = (x0[i] + x1[i]) // 2, (y0[i] + y1[i]) // 2
                if x1[i] > x0[i]:
                    depth[k, b, max(y0[i] - 2, 0): y1[i] + 3, mx: x1[i] + 3] = 0.0
                else:
                    depth[k, b, my: y1[i] + 3, max(x0[i] - 2, 0): x1[i] + 3] = 0.0
            for i in pick[9:15]:  # an edge on the line's own row / column, on either side
                if x1[i] > x0[i]:
                    r = y0[i] - int(rng.integers(0, 2)) * 6
                    depth[k, b, max(r, 0): max(r, 0) + 6, x0[i]: (x0[i] + x1[i]) // 2 + 1] = 0.0
                else:
                    r = x0[i] - int(rng.integers(0, 2)) * 6
                    depth[k, b, y0[i]: (y0[i] + y1[i]) // 2 + 1, max(r, 0): max(r, 0) + 6] = 0.0
            for _ in range(6):
                hw, hh = rng.integers(8, S // 8), rng.integers(8, S // 8)
                xx, yy = rng.integers(0, S - hw), rng.integers(0, S - hh)
                depth[k, b, yy:yy + hh, xx:xx + hw] = 0.0
    v0, v1 = rng.random((B, n0)) > 0.1, rng.random((B, n1)) > 0.1
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))  # noqa: E731
    g = {"depth0": f32(depth[0]), "depth1": f32(depth[1]), "camera0": f32(cam), "camera1": f32(cam), "T_0to1": f32(T01),
         "T_1to0": f32(T10), "lines0": f32(l0), "lines1": f32(l1), "valid_lines0": v0, "valid_lines1": v1}
    return g, (S, S), (S, S)


CASES = [
    # name, recipe, seed, B, n0, n1, kwargs of the reference call, recipe kwargs
    ("line_gtd_exact_b3_n64_n48", exact_case, 21, 3, 64, 48, {"npts": 33}, {}),
    ("line_gtd_exact_b1_n48_n64", exact_case, 22, 1, 48, 64, {"npts": 33}, {}),
    ("line_gtd_rand_b2_n96_n130_d0", random_case, 81, 2, 96, 130, {}, {"n_dist": 0}),
    ("line_gtd_rand_b2_n130_n96_d2", random_case, 102, 2, 130, 96, {}, {"n_dist": 2}),
    ("line_gtd_rand_b1_n128_n128_d4", random_case, 103, 1, 128, 128, {}, {"n_dist": 4}),
    ("line_gtd_rand_p7_b2_n96_n96", random_case, 44, 2, 96, 96, {"npts": 7, "overlap_th": 0.5, "min_visibility_th": 0.2},
     {"n_dist": 0}),
]
DEFAULTS = {"npts": 50, "dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.5}


def ref_data(Wr, g, dtype, shape0, shape1):
    t = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    B = g["depth0"].shape[0]
    return {"view0": {"camera": Wr.Camera(t(g["camera0"])), "depth": t(g["depth0"]), "image": torch.zeros((B, 1) + tuple(shape0))},
            "view1": {"camera": Wr.Camera(t(g["camera1"])), "depth": t(g["depth1"]), "image": torch.zeros((B, 1) + tuple(shape1))},
            "T_0to1": Wr.Pose(t(g["T_0to1"])), "T_1to0": Wr.Pose(t(g["T_1to0"]))}


def run_reference(gen, l0, l1, v0, v1, data, kw):
    """The reference's labels with the cost matrices and assignations SciPy saw and the two ``rotated``."""
    seen, rot = [], []
    real, real_einsum = gen.linear_sum_assignment, torch.einsum

    def spy(C):
        out = real(C)
        seen.append((np.array(C, copy=True), np.array(out)))
        return out

    def spy_einsum(*a, **k):
        out = real_einsum(*a, **k)
        rot.append(out)
        return out

    gen.linear_sum_assignment = spy
    torch.einsum = spy_einsum
    try:
        pos, m0, m1 = gen.gt_line_matches_from_pose_depth(l0, l1, v0, v1, data, kw["npts"], kw["dist_th"], kw["overlap_th"],
                                                          kw["min_visibility_th"])
    finally:
        gen.linear_sum_assignment = real
        torch.einsum = real_einsum
    assert len(rot) == 2
    rots = [(r[..., 0], r[..., 1]) for r in rot]
    return pos, m0, m1, np.stack([c for c, _ in seen]), np.stack([a for _, a in seen]), rots


def reference_stage_a(gen, l0, l1, data, kw):
    """:250-352 with the reference's own functions."""
    npts, dist_th, mvt = kw["npts"], kw["dist_th"], kw["min_visibility_th"]
    B, n0, n1 = l0.shape[0], l0.shape[1], l1.shape[1]
    h0, w0 = data["view0"]["depth"][0].shape
    h1, w1 = data["view1"]["depth"][0].shape
    c0, c1 = lr.clamp_lines(l0.clone(), h0, w0), lr.clamp_lines(l1.clone(), h1, w1)
    pts0 = gen.sample_pts(c0, npts).reshape(B, n0 * npts, 2)
    pts1 = gen.sample_pts(c1, npts).reshape(B, n1 * npts, 2)
    d0, valid0 = gen.sample_depth(pts0, data["view0"]["depth"])
    d1, valid1 = gen.sample_depth(pts1, data["view1"]["depth"])
    pts0_1, vis0 = gen.project(pts0, d0, data["view1"]["depth"], data["view0"]["camera"], data["view1"]["camera"],
                               data["T_0to1"], valid0)
    pts1_0, vis1 = gen.project(pts1, d1, data["view0"]["depth"], data["view1"]["camera"], data["view0"]["camera"],
                               data["T_1to0"], valid1)
    ih0, iw0 = data["view0"]["image"].shape[-2:]
    ih1, iw1 = data["view1"]["image"].shape[-2:]
    out_of0 = lr.outside(pts1_0, ih0, iw0).reshape(B, n1, npts).float().mean(dim=-1) >= (1 - mvt)
    out_of1 = lr.outside(pts0_1, ih1, iw1).reshape(B, n0, npts).float().mean(dim=-1) >= (1 - mvt)
    pts0_1, pts1_0 = pts0_1.reshape(B, n0, npts, 2), pts1_0.reshape(B, n1, npts, 2)
    pd0, ov0 = gen.torch_perp_dist(c0, pts1_0)
    cnt0 = (((pd0 < dist_th) & ov0) * vis1.reshape(B, 1, n1, npts)).sum(dim=-1)
    pd1, ov1 = gen.torch_perp_dist(c1, pts0_1)
    cnt1 = (((pd1 < dist_th) & ov1) * vis0.reshape(B, 1, n0, npts)).sum(dim=-1)
    ign0 = valid0.reshape(B, n0, npts).float().mean(dim=-1) < mvt
    ign1 = valid1.reshape(B, n1, npts).float().mean(dim=-1) < mvt
    a = {"cnt0": cnt0, "cnt1t": cnt1.transpose(-1, -2), "out_of0": out_of0, "out_of1": out_of1, "ignore_depth0": ign0,
         "ignore_depth1": ign1, "num_visible0": vis0.reshape(B, n0, npts).sum(-1), "num_visible1": vis1.reshape(B, n1, npts).sum(-1)}
    return a, {"pts0_1": pts0_1, "pts1_0": pts1_0, "pts0": pts0.reshape(B, n0, npts, 2), "pts1": pts1.reshape(B, n1, npts, 2)}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ref.STAGE_A_KEYS)


def build(gen, Wr, name, recipe, seed, B, n0, n1, kw, rkw):
    """One case; returns (arrays, meta, report) or raises AssertionError naming what the seed broke."""
    kw = {**DEFAULTS, **kw}
    exact = recipe is exact_case
    g, shape0, shape1 = recipe(seed, B, n0, n1, **rkw)
    meta = {"B": B, "n0": n0, "n1": n1, "seed": seed, "exact": exact, "image_shape0": list(shape0), "image_shape1": list(shape1),
            "n_dist": int(g["camera0"].shape[1] - 6), **kw}
    l0, l1, v0, v1 = (torch.from_numpy(g[k]) for k in ("lines0", "lines1", "valid_lines0", "valid_lines1"))
    d32, d64 = ref_data(Wr, g, torch.float32, shape0, shape1), ref_data(Wr, g, torch.float64, shape0, shape1)
    pos, m0, m1, cost, assignation, rot32 = run_reference(gen, l0, l1, v0, v1, d32, kw)
    r64 = run_reference(gen, l0.double(), l1.double(), v0, v1, d64, kw)
    a32, x32 = reference_stage_a(gen, l0, l1, d32, kw)
    a64, x64 = reference_stage_a(gen, l0.double(), l1.double(), d64, kw)
    assert pos.dtype == torch.bool and m0.dtype == torch.int64
    # the pieces are the full run's: the recorded cost is -cnt0 * cnt1t wherever it is not 1e6, and the
    # restated stage B turns the stage-A arrays into the reference's labels, cost and assignation
    prod = -(a32["cnt0"] * a32["cnt1t"]).numpy().astype(np.float64)
    assert np.array_equal(cost[cost != 1e6], prod[cost != 1e6]), "cost"
    rb = ref.stage_b_of(a32, v0, v1, kw["npts"], kw["overlap_th"])
    assert torch.equal(rb[0], pos) and torch.equal(rb[1], m0) and torch.equal(rb[2], m1), "stage B"
    assert np.array_equal(rb[3].numpy().astype(np.float64), cost) and np.array_equal(rb[4].numpy(), assignation), "stage B cost"
    assert int(a32["cnt0"].max()) <= 255 and np.array_equal(cost, cost.astype(np.int32))
    # the restated stage A gives the reference's arrays bit for bit, in both precisions
    f32, f64 = ref.feed_of(g, meta), ref.feed_of(g, meta, torch.float64)
    i32, i64 = {}, {}
    assert same(ref.stage_a(l0, l1, f32, kw["npts"], kw["dist_th"], kw["min_visibility_th"], info=i32), a32), "restated stage A, fp32"
    assert same(ref.stage_a(l0.double(), l1.double(), f64, kw["npts"], kw["dist_th"], kw["min_visibility_th"], info=i64), a64), \
        "restated stage A, fp64"
    out = {k: g[k] for k in g}
    out.update({"positive_idx": np.argwhere(pos.numpy()).astype(np.int32), "m0": m0.numpy(), "m1": m1.numpy(),
                "cost_i32": cost.astype(np.int32), "assignation": assignation.astype(np.int32)})
    for k in ref.STAGE_A_KEYS:
        a = a32[k].numpy()
        out[k] = a if a.dtype == bool else a.astype(np.uint8)
    ign = int(a32["ignore_depth0"].sum()) + int(a32["ignore_depth1"].sum())
    oo = int(a32["out_of0"].sum()) + int(a32["out_of1"].sum())
    stats = f"positives {len(out['positive_idx'])} m0>-1 {(out['m0'] > -1).sum()} m0==-1 {(out['m0'] == -1).sum()} " \
            f"m0==-2 {(out['m0'] == -2).sum()} depth-ignored {ign} out_of {oo}"
    if exact:
        assert torch.equal(r64[0], pos) and torch.equal(r64[1], m0) and torch.equal(r64[2], m1), "fp32 and fp64 labels differ"
        assert same(a32, a64), "fp32 and fp64 stage-A arrays differ"
        assert ign >= 3 and oo >= 3 and len(out["positive_idx"]) >= 10, stats
        return out, meta, stats
    i32.update(x32)  # the reference's own projections and rotated
    i64.update(x64)
    sz32, sz64 = (i32["rot0"][2], i32["rot1"][2]), (i64["rot0"][2], i64["rot1"][2])
    i32["rot0"], i32["rot1"] = rot32[0] + (sz32[0],), rot32[1] + (sz32[1],)
    i64["rot0"], i64["rot1"] = r64[5][0] + (sz64[0],), r64[5][1] + (sz64[1],)
    tol = ref.tolerances(i32, i64, kw["dist_th"])
    mg = ref.margins(i32, i64, f64, tol, kw["npts"], kw["dist_th"], kw["min_visibility_th"])
    shares = []
    for k, und in (("cnt0", "und0"), ("cnt1t", "und1t")):
        nz = int((out[k] > 0).sum())
        share = int((mg[und] > 0).sum()) / max(nz, 1)
        shares.append(share)
        assert share <= CAP, (k, "undecidable share", round(share, 4))
        dec = mg[und] == 0
        assert np.array_equal(out[k][dec], a64[k].numpy()[dec]), (k, "fp32 and fp64 differ on a decided entry")
        lo = mg["lo" + und[3:]].astype(int)
        assert ((out[k] >= lo) & (out[k] <= lo + mg[und])).all(), (k, "outside its bounds")
    ul = (int(mg["und_line0"].sum()) + int(mg["und_line1"].sum())) / (B * (n0 + n1))
    assert ul <= CAP, ("undecidable lines", round(ul, 4))
    for k, line in (("out_of0", "und_line1"), ("out_of1", "und_line0"), ("ignore_depth0", "und_line0"),
                    ("ignore_depth1", "und_line1"), ("num_visible0", "und_line0"), ("num_visible1", "und_line1")):
        dec = ~mg[line]
        assert np.array_equal(a32[k].numpy()[dec], a64[k].numpy()[dec]), (k, "fp32 and fp64 differ on a decided line")
    out.update(mg)
    decided = ref.pair_decided(out, meta)
    for b in np.nonzero(decided)[0]:
        assert torch.equal(r64[0][b], pos[b]) and torch.equal(r64[1][b], m0[b]) and torch.equal(r64[2][b], m1[b]), \
            "fp32 and fp64 labels differ on a decided pair"
    assert len(out["positive_idx"]) >= 10 and ign >= 3 and oo >= 3, stats
    assert decided.sum() >= 1, "no decided pair"
    meta.update({"tol": tol, "und_share0": shares[0], "und_share1": shares[1], "und_line_share": ul})
    report = " ".join(f"{k} {v:.1e}" for k, v in tol.items()) + \
        f" undecidable {shares[0]:.4f}/{shares[1]:.4f} lines {ul:.4f} decided pairs {int(decided.sum())}/{B} {stats}"
    return out, meta, report


def main():
    gen = install_shim()
    Wr = importlib.import_module("gluefactory.geometry.wrappers")
    for fn in ("sample_depth", "project"):
        assert hasattr(gen, fn), fn
    os.makedirs(ref.HERE, exist_ok=True)
    only = sys.argv[1:]
    for name, recipe, seed, B, n0, n1, kw, rkw in CASES:
        if only and name not in only:
            continue
        out, meta, report = build(gen, Wr, name, recipe, seed, B, n0, n1, kw, rkw)
        print(f"{name}: {report}")
        out["meta_json"] = np.array(json.dumps(meta))
        path = os.path.join(ref.HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"  wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
