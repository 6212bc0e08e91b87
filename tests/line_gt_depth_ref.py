"""Torch-CPU restatement of the reference's line ground truth from pose and depth, for the tests only
(any dtype).

``gt_line_matches_from_pose_depth`` is ``gluefactory/geometry/gt_generation.py:207-406`` over
``sample_pts`` (:164-170), ``sample_depth`` / ``project`` (``geometry/depth.py:20-68``, restated in
tests/gt_depth_ref.py) and ``torch_perp_dist`` (:173-204, its CPU path, restated in tests/line_gt_ref.py).
tests/golden/make_line_gt_depth_golden.py runs the reference itself; tests/test_line_gt_depth_golden.py
holds this restatement to those fixtures.

Stage A gives the two counts of close *and visible* samples, the out_of flags, the depth-ignore flags and
the per-line numbers of visible samples; stage B turns those into labels.  Also here: the integer
thresholds the kernels use, evaluated with torch as the reference evaluates them; the near-tie margins
(:func:`margins`); the fixture loader and the comparisons under the gating the fixtures record, shared by
the CPU and the GPU tests.
"""
import glob
import json
import os

import numpy as np
import torch

import gt_depth_ref as gd
import line_gt_ref as lr

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_gt_depth")
STAGE_A_KEYS = ("cnt0", "cnt1t", "out_of0", "out_of1", "ignore_depth0", "ignore_depth1", "num_visible0", "num_visible1")


# ---------------------------------------------------------------------------------------------
# stage A
def image_sizes(data):
    """(h0, w0), (h1, w1) of the out-of-image test (:290-291); without ``image`` the depth map's size (the
    reference raises a KeyError there)."""
    out = []
    for v in ("view0", "view1"):
        src = data[v]["image"] if "image" in data[v] else data[v]["depth"]
        out.append(tuple(int(s) for s in src.shape[-2:]))
    return out


@torch.no_grad()
def stage_a(lines0, lines1, data, npts=50, dist_th=5, min_visibility_th=0.5, info=None):
    """:240-316 and :345-347.  Returns a dict: cnt0 / cnt1t [B,n0,n1] int64, out_of0 [B,n1], out_of1 [B,n0],
    ignore_depth0 [B,n0], ignore_depth1 [B,n1] (bool), num_visible0 [B,n0], num_visible1 [B,n1] (int64).
    ``info``: a dict that receives the intermediates the margins need."""
    cam0, cam1 = gd._data(data["view0"]["camera"]), gd._data(data["view1"]["camera"])
    T01, T10 = gd._data(data["T_0to1"]), gd._data(data["T_1to0"])
    depth0, depth1 = data["view0"]["depth"], data["view1"]["depth"]
    h0, w0 = depth0[0].shape
    h1, w1 = depth1[0].shape
    l0 = lr.clamp_lines(lr.flat_lines(lines0.clone()), h0, w0)
    l1 = lr.clamp_lines(lr.flat_lines(lines1.clone()), h1, w1)
    B, n0, n1 = l0.shape[0], l0.shape[1], l1.shape[1]
    pts0 = lr.sample_points(l0, npts).reshape(B, n0 * npts, 2)
    pts1 = lr.sample_points(l1, npts).reshape(B, n1 * npts, 2)
    d0, valid0 = gd.sample_depth(pts0, depth0)
    d1, valid1 = gd.sample_depth(pts1, depth1)
    i0 = {} if info is not None else None
    i1 = {} if info is not None else None
    pts0_1, vis0 = gd.project(pts0, d0, depth1, cam0, cam1, T01, valid0, info=i0)
    pts1_0, vis1 = gd.project(pts1, d1, depth0, cam1, cam0, T10, valid1, info=i1)
    (ih0, iw0), (ih1, iw1) = image_sizes(data)
    out_of0 = lr.outside(pts1_0, ih0, iw0).reshape(B, n1, npts).float().mean(dim=-1) >= (1 - min_visibility_th)
    out_of1 = lr.outside(pts0_1, ih1, iw1).reshape(B, n0, npts).float().mean(dim=-1) >= (1 - min_visibility_th)
    pts0_1, pts1_0 = pts0_1.reshape(B, n0, npts, 2), pts1_0.reshape(B, n1, npts, 2)

    def counts(segs, pts, vis):
        rx, ry, sizes = lr.rotate(segs, pts)
        close = (ry.abs() < dist_th) & (rx <= 0) & (rx.abs() <= sizes[..., None, None])
        return (close * vis.reshape(B, 1, -1, npts)).sum(dim=-1), (rx, ry, sizes)

    cnt0, rot0 = counts(l0, pts1_0, vis1)
    cnt1, rot1 = counts(l1, pts0_1, vis0)
    ign0 = valid0.reshape(B, n0, npts).float().mean(dim=-1) < min_visibility_th
    ign1 = valid1.reshape(B, n1, npts).float().mean(dim=-1) < min_visibility_th
    if info is not None:
        info.update({"p0": i0, "p1": i1, "pts0": pts0.reshape(B, n0, npts, 2), "pts1": pts1.reshape(B, n1, npts, 2),
                     "pts0_1": pts0_1, "pts1_0": pts1_0, "valid0": valid0.reshape(B, n0, npts),
                     "valid1": valid1.reshape(B, n1, npts), "vis0": vis0.reshape(B, n0, npts),
                     "vis1": vis1.reshape(B, n1, npts), "rot0": rot0, "rot1": rot1, "l0": l0, "l1": l1})
    return {"cnt0": cnt0, "cnt1t": cnt1.transpose(-1, -2), "out_of0": out_of0, "out_of1": out_of1, "ignore_depth0": ign0,
            "ignore_depth1": ign1, "num_visible0": vis0.reshape(B, n0, npts).sum(-1), "num_visible1": vis1.reshape(B, n1, npts).sum(-1)}


# ---------------------------------------------------------------------------------------------
# the integer thresholds, by evaluating the reference's expressions on every count
def min_close_table(npts, overlap_th):
    """table[v]: the smallest count c with ``c > float(v) * overlap_th`` as :329-336 compares them (an int64
    count against an fp32 product); npts + 1 if none."""
    counts = torch.arange(npts + 1)
    table = []
    for v in range(npts + 1):
        visible = torch.zeros(npts, dtype=torch.bool)
        visible[:v] = True
        ok = counts > visible.float().sum(-1) * overlap_th
        table.append(int(ok.nonzero()[0]) if ok.any() else npts + 1)
    return table


def min_valid_count(npts, min_visibility_th):
    """The smallest number of samples with valid depth that is not ignored (:345-347); npts + 1 if none."""
    rows = (torch.arange(npts)[None] < torch.arange(npts + 1)[:, None])  # row c: c valid samples
    ok = ~(rows.float().mean(dim=-1) < min_visibility_th)
    return int(ok.nonzero()[0]) if ok.any() else npts + 1


# ---------------------------------------------------------------------------------------------
# stage B
def cost_from_counts(cnt0, cnt1t, out_of0, out_of1, ign0, ign1, nvis0, nvis1, overlap_th):  # :328-363
    mask = (cnt1t > nvis0.float()[:, :, None] * overlap_th) & (cnt0 > nvis1.float()[:, None] * overlap_th)
    unm0 = torch.all(~mask, dim=2) | out_of1
    unm1 = torch.all(~mask, dim=1) | out_of0
    cost = -(cnt0 * cnt1t).clone()
    cost[unm0] = 1e6
    cost[ign0] = 1e6
    cost = cost.transpose(1, 2)
    cost[unm1] = 1e6
    cost[ign1] = 1e6
    return mask, unm0, unm1, cost.transpose(1, 2)


@torch.no_grad()
def stage_b(cnt0, cnt1t, out_of0, out_of1, ignore_depth0, ignore_depth1, num_visible0, num_visible1, valid0, valid1,
            npts=50, overlap_th=0.2, solver=None):
    """Labels from counts (:321-400).  Returns (positive, m0, m1, cost, assignation)."""
    solver = solver or lr.lsap
    cnt0, cnt1t = cnt0.long(), cnt1t.long()
    B, n0, n1 = cnt0.shape
    ign0, ign1 = ignore_depth0.bool() | ~valid0.bool(), ignore_depth1.bool() | ~valid1.bool()
    mask, unm0, unm1, cost = cost_from_counts(cnt0, cnt1t, out_of0.bool(), out_of1.bool(), ign0, ign1, num_visible0.long(),
                                              num_visible1.long(), overlap_th)
    assignation = torch.tensor(np.array([solver(C.astype(np.float64)) for C in cost.numpy()])).long()
    positive = torch.zeros((B, n0, n1), dtype=torch.bool)
    bi = torch.arange(B)[:, None].repeat(1, assignation.shape[-1]).flatten()
    positive[bi, assignation[:, 0].flatten(), assignation[:, 1].flatten()] = True
    m0 = torch.full((B, n0), -1, dtype=torch.long)
    m0.scatter_(-1, assignation[:, 0], assignation[:, 1])
    m1 = torch.full((B, n1), -1, dtype=torch.long)
    m1.scatter_(-1, assignation[:, 1], assignation[:, 0])
    positive = positive & mask
    positive[unm0] = False
    positive[ign0] = False
    positive = positive.transpose(1, 2)
    positive[unm1] = False
    positive[ign1] = False
    positive = positive.transpose(1, 2)
    m0[~positive.any(-1)] = -1
    m0[unm0] = -1
    m0[ign0] = -2
    m1[~positive.any(-2)] = -1
    m1[unm1] = -1
    m1[ign1] = -2
    return positive, m0, m1, cost, assignation


def stage_b_of(a, valid0, valid1, npts, overlap_th, solver=None):
    """:func:`stage_b` on a stage-A dict of torch tensors or NumPy arrays."""
    t = [torch.as_tensor(np.asarray(a[k])) for k in STAGE_A_KEYS]
    return stage_b(*t, torch.as_tensor(np.asarray(valid0)), torch.as_tensor(np.asarray(valid1)), npts, overlap_th, solver)


def gt_line_matches_from_pose_depth(lines0, lines1, valid0, valid1, data, npts=50, dist_th=5, overlap_th=0.2,
                                    min_visibility_th=0.5, solver=None):
    if lines0.shape[1] == 0 or lines1.shape[1] == 0:  # :227-238
        B, n0, n1 = lines0.shape[0], lines0.shape[1], lines1.shape[1]
        return torch.zeros((B, n0, n1), dtype=torch.bool), torch.full((B, n0), -1), torch.full((B, n1), -1)
    a = stage_a(lines0, lines1, data, npts, dist_th, min_visibility_th)
    return stage_b_of(a, valid0, valid1, npts, overlap_th, solver)[:3]


# ---------------------------------------------------------------------------------------------
# margins and gating (computed in fp64)
def feed_of(g, meta, dtype=torch.float32, device="cpu", image=True):
    """The reference's ``data`` dict from fixture arrays (cameras and poses as rows); ``image``: with images
    of the recorded size (only their shape is read)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).to(device)  # noqa: E731
    B = g["depth0"].shape[0]
    d = {"view0": {"camera": t(g["camera0"]), "depth": t(g["depth0"])},
         "view1": {"camera": t(g["camera1"]), "depth": t(g["depth1"])}, "T_0to1": t(g["T_0to1"]), "T_1to0": t(g["T_1to0"])}
    if image:
        for v, k in (("view0", "image_shape0"), ("view1", "image_shape1")):
            d[v]["image"] = torch.zeros((B, 1) + tuple(meta[k]), dtype=dtype, device=device)
    return d


def _dev(a, b, sel=None):
    a, b = a.double(), b.double()
    ok = torch.isfinite(a) & torch.isfinite(b)
    if sel is not None:
        ok = ok & sel
    return float((a - b)[ok].abs().max()) if bool(ok.any()) else 0.0


def tolerances(i32, i64, dist_th):
    """4 x the largest deviation between the fp32 and the fp64 run, per quantity (``i32`` / ``i64``: the
    ``info`` of :func:`stage_a`; the generator puts the reference's own fp32 ``rotated`` and projections into
    ``i32``)."""
    tol = {}
    band = 4.0 * dist_th
    for k in ("rot0", "rot1"):
        rx, ry, sz = i64[k]
        near = (ry.abs() < band) & (rx <= band) & (rx >= -(sz.double()[..., None, None] + band))
        tol[k] = 4 * max(_dev(i32[k][0], rx, near), _dev(i32[k][1], ry, near))
    tol["proj"] = 4 * max(_dev(i32["pts0_1"], i64["pts0_1"]), _dev(i32["pts1_0"], i64["pts1_0"]))
    tol["own"] = 4 * max(_dev(i32["pts0"], i64["pts0"]), _dev(i32["pts1"], i64["pts1"]))
    both = lambda k: max(_dev(i32["p0"][k], i64["p0"][k]), _dev(i32["p1"][k], i64["p1"][k]))  # noqa: E731
    tol["z"] = 4 * both("z")
    tol["bound"] = 4 * max(_dev(i32[p]["bound"], i64[p]["bound"], i64[p]["bound"] < 8.0) for p in ("p0", "p1"))
    tol["r2"] = 4 * both("r2_margin") if "r2_margin" in i64["p0"] else 0.0
    return tol


DEPTH_JUMP = 1e-5


def _own_und(xy32, xy64, depth, tol_own):
    """Samples whose sampled depth hangs on the footprint: the fp64 chain at the sample moved by
    +-tol_own in every coordinate that is not bit-equal in the two precisions (a clamped or an exactly
    representable coordinate takes the same footprint in both) gives another validity, or a depth that
    differs by more than DEPTH_JUMP.  Within one footprint the depth moves by its gradient times tol_own
    (~1e-7 here) and an fp32 result is within ~1e-6 of it; a change of the bilinear footprint next to a
    pixel without depth, or of the nearest sample, moves it by the difference of two pixels (>= 2e-4 on the
    fixtures' maps): 1e-5 separates the two.  Within half a pixel of the map's first row or column the zero
    padding enters with a weight that grows by 1 per px, so there the depth legitimately moves by up to
    depth * tol_own per coordinate and the bound is wider by 4 * tol_own * max(depth)."""
    B = depth.shape[0]
    shape = xy64.shape[:-1]
    neq = (xy32.double() != xy64).double()
    d0, v0 = gd.sample_depth(xy64.reshape(B, -1, 2), depth)
    und = torch.zeros_like(v0)
    band = (xy64 < 0.5).any(-1).reshape(B, -1)
    jump = DEPTH_JUMP + band.double() * (4.0 * tol_own * float(depth.max()))
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            q = xy64 + neq * xy64.new_tensor([sx, sy]) * tol_own
            d, v = gd.sample_depth(q.reshape(B, -1, 2), depth)
            und |= (v != v0) | (v & v0 & ((d - d0).abs() > jump))
    return und.reshape(shape)


def margins(i32, i64, data64, tol, npts, dist_th, min_visibility_th):
    """What the fp64 run cannot decide for an fp32 one.  Per sample: its depth validity (:func:`_own_und`);
    its visibility (that, or with valid depth z - eps, an image bound of the camera or r^2 - limit within
    tolerance); whether it is outside the other image (its validity, or a projected coordinate within
    tol["proj"] of a border).  Per entry and direction: ``lo`` = samples firmly close and firmly visible,
    ``und`` = samples that may count (not firmly far, not firmly invisible) but not firmly; a count may lie
    in [lo, lo + und].  A line with any sample undecidable in validity, visibility or outside is undecidable
    (its num_visible, ignore_depth and out_of)."""
    (ih0, iw0), (ih1, iw1) = image_sizes(data64)
    out = {}
    per_side = {}
    for s, pts, prj, pinfo, depth, (ih, iw) in (("0", "pts0", "pts0_1", "p0", data64["view0"]["depth"], (ih1, iw1)),
                                                ("1", "pts1", "pts1_0", "p1", data64["view1"]["depth"], (ih0, iw0))):
        shape = i64[pts].shape[:-1]
        own = _own_und(i32[pts], i64[pts], depth, tol["own"])
        pi = i64[pinfo]
        u = (pi["z"] - gd.EPS).abs() < tol["z"]
        u |= pi["bound"] < max(tol["bound"], tol["proj"])
        if "r2_margin" in pi:
            u |= pi["r2_margin"].abs() < tol["r2"]
        vis_und = (u.reshape(shape) & i64["valid" + s]) | own
        p = i64[prj]
        lim = torch.tensor([iw, ih]).to(p)
        out_und = (((p.abs() < tol["proj"]) | ((p - lim).abs() < tol["proj"])).any(-1)) | own
        per_side[s] = (i64["vis" + s] & ~vis_und, vis_und)
        out["und_line" + s] = (own | vis_und | out_und).any(-1).numpy()

    def direction(rot, tau, vis_firm, vis_und):
        rx, ry, sizes = rot
        sz = sizes.double()[..., None, None]
        ms = torch.stack([dist_th - ry.abs(), -rx, sz - rx.abs()])
        firm_false = ~(ms > -tau)  # NaNs (no depth, a zero-length segment): firmly false
        cu = (ms.abs() < tau).any(0) & ~firm_false.any(0)
        cf = (ms[0] > 0) & (ms[1] >= 0) & (ms[2] >= 0) & ~cu
        vf, vu = vis_firm[:, None], vis_und[:, None]
        firm = cf & vf
        # a sample whose visibility is undecidable may also project elsewhere: it may count wherever it is
        # not firmly far in the fp64 run, and wherever that run has no projection at all
        maybe = ((cf | cu) & (vf | vu) & ~firm) | (vu & torch.isnan(ry))
        return firm.sum(-1), maybe.sum(-1)

    lo0, und0 = direction(i64["rot0"], tol["rot0"], *per_side["1"])
    lo1, und1 = direction(i64["rot1"], tol["rot1"], *per_side["0"])
    out.update({"lo0": lo0.numpy().astype(np.uint8), "und0": und0.numpy().astype(np.uint8),
                "lo1t": lo1.transpose(1, 2).numpy().astype(np.uint8), "und1t": und1.transpose(1, 2).numpy().astype(np.uint8)})
    return out


# ---------------------------------------------------------------------------------------------
# fixtures
def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "line_gtd_*.npz")))


_CACHE = {}


def load_fixture(name):
    """The fixture as (dict of arrays, meta); loaded once and shared (treat as read-only)."""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(HERE, name + ".npz"))
    g = {k: z[k] for k in z.files if k != "meta_json"}
    meta = json.loads(str(z["meta_json"]))
    B, n0, n1 = meta["B"], meta["n0"], meta["n1"]
    a = np.zeros((B, n0, n1), bool)
    t = g.pop("positive_idx")
    a[t[:, 0], t[:, 1], t[:, 2]] = True
    g["positive"] = a
    g["cost"] = g.pop("cost_i32").astype(np.float64)
    _CACHE[name] = (g, meta)
    return g, meta


def call_kw(meta):
    return {k: meta[k] for k in ("npts", "dist_th", "overlap_th", "min_visibility_th")}


def check_stage_a(got, g, meta):
    """Stage A outputs (a dict under STAGE_A_KEYS, NumPy) against fixture ``g``: the exact fixtures bit for
    bit; the others equal on decided entries and lines, counts inside [lo, lo + und] elsewhere."""
    for k, lo, und in (("cnt0", "lo0", "und0"), ("cnt1t", "lo1t", "und1t")):
        a = np.asarray(got[k]).astype(np.int64)
        if meta["exact"]:
            np.testing.assert_array_equal(a, g[k], err_msg=k)
            continue
        dec = g[und] == 0
        np.testing.assert_array_equal(a[dec], g[k][dec], err_msg=k)
        low, high = g[lo].astype(np.int64), g[lo].astype(np.int64) + g[und]
        assert ((a >= low) & (a <= high)).all(), f"{k}: {int(((a < low) | (a > high)).sum())} counts outside their bounds"
    for k, line in (("out_of0", "und_line1"), ("out_of1", "und_line0"), ("ignore_depth0", "und_line0"),
                    ("ignore_depth1", "und_line1"), ("num_visible0", "und_line0"), ("num_visible1", "und_line1")):
        a = np.asarray(got[k]).astype(g[k].dtype)
        dec = np.ones(a.shape, bool) if meta["exact"] else ~g[line]
        np.testing.assert_array_equal(a[dec], g[k][dec], err_msg=k)


def pair_decided(g, meta):
    """Per pair: no undecidable entry and no undecidable line (the labels are then the reference's)."""
    B = meta["B"]
    if meta["exact"]:
        return np.ones(B, bool)
    return np.array([not (g["und0"][b].any() or g["und1t"][b].any() or g["und_line0"][b].any() or g["und_line1"][b].any())
                     for b in range(B)])


def check_labels(got, g, pairs=None):
    """(positive, m0, m1) as NumPy against the fixture's, on the given pairs (all by default), no gating."""
    sel = slice(None) if pairs is None else pairs
    for a, k in zip(got, ("positive", "m0", "m1")):
        a = np.asarray(a)
        assert a.dtype == g[k].dtype, (k, a.dtype)
        np.testing.assert_array_equal(a[sel], g[k][sel], err_msg=k)
