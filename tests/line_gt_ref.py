"""Torch-CPU restatement of the reference's line ground truth from a homography, for the tests only
(any dtype), and a NumPy port of SciPy's assignment solver.

``gt_line_matches_from_homography`` is ``gluefactory/geometry/gt_generation.py:409-558`` over
``sample_pts`` (:160-170), ``torch_perp_dist`` (:173-204, its CPU path) and ``warp_points_torch``
(``geometry/homography.py:161-180``).  tests/golden/make_line_gt_golden.py runs the reference itself;
tests/test_line_gt_golden.py holds this restatement to those fixtures.

Also here: the near-tie margins (:func:`margins`), the fixture loader and the comparisons under the
gating the fixtures record, shared by the CPU and the GPU tests.
"""
import glob
import json
import os

import numpy as np
import torch

from gt_ref import warp_points_torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_gt")


def flat_lines(lines):  # :430-437
    if lines.shape[-2:] == (2, 2):
        return torch.flatten(lines, -2)
    if lines.dim() == 4:
        return torch.cat([lines[:, :, 0], lines[:, :, -1]], dim=2)
    return lines


def clamp_lines(lines, h, w):  # :441-448
    top = lines.new_tensor([w - 1, h - 1, w - 1, h - 1], dtype=torch.float)
    return torch.min(torch.max(lines, torch.zeros_like(lines)), top)


def sample_points(lines, npts):  # :165-169, [B, n, npts, 2]
    step = (lines[..., 2:4] - lines[..., :2]) / (npts - 1)
    k = torch.arange(npts).to(lines)
    return lines[..., None, :2] + step[..., None, :] * k[:, None]


def segment_sizes(segs):  # :177-178: the length rounded to fp16
    return torch.norm(segs[..., 2:] - segs[..., :2], dim=-1).half()


def rotate(segs, pts):
    """torch_perp_dist's ``rotated`` as two [B, nsegs, nlines, npts] tensors: the samples centred on the
    second endpoint, along (rot_x) and across (rot_y) the segment."""
    sizes = segment_sizes(segs)
    nd = (segs[..., 2:] - segs[..., :2]) / sizes.unsqueeze(-1)
    c = pts[:, None] - segs[:, :, None, None, 2:]
    nx, ny = nd[..., 0, None, None], nd[..., 1, None, None]
    rot_x = nx * c[..., 0] + ny * c[..., 1]
    rot_y = (-ny) * c[..., 0] + nx * c[..., 1]
    return rot_x, rot_y, sizes


def close_counts(segs, pts, dist_th):  # :472-473, :483
    rot_x, rot_y, sizes = rotate(segs, pts)
    close = (rot_y.abs() < dist_th) & (rot_x <= 0) & (rot_x.abs() <= sizes[..., None, None])
    return close.sum(-1)


def outside(pts, h, w):  # :461-463
    return (pts < 0).any(-1) | (pts >= torch.tensor([w, h]).to(pts)).any(-1)


@torch.no_grad()
def stage_a(lines0, lines1, shape0, shape1, H, npts=50, dist_th=5, min_visibility_th=0.2):
    """The counts [B,n0,n1] (int64) and the out_of flags of :450-488."""
    h0, w0 = shape0[-2:]
    h1, w1 = shape1[-2:]
    l0, l1 = clamp_lines(flat_lines(lines0.clone()), h0, w0), clamp_lines(flat_lines(lines1.clone()), h1, w1)
    B, n0, n1 = l0.shape[0], l0.shape[1], l1.shape[1]
    pts0_1 = warp_points_torch(sample_points(l0, npts).reshape(B, n0 * npts, 2), H, inverse=False).reshape(B, n0, npts, 2)
    pts1_0 = warp_points_torch(sample_points(l1, npts).reshape(B, n1 * npts, 2), H, inverse=True).reshape(B, n1, npts, 2)
    out_of0 = outside(pts1_0, h0, w0).float().mean(-1) >= (1 - min_visibility_th)
    out_of1 = outside(pts0_1, h1, w1).float().mean(-1) >= (1 - min_visibility_th)
    cnt0 = close_counts(l0, pts1_0, dist_th)
    cnt1t = close_counts(l1, pts0_1, dist_th).transpose(-1, -2)
    return cnt0, cnt1t, out_of0, out_of1


def min_out_count(npts, min_visibility_th):
    """The smallest number of outside samples with ``mean >= 1 - min_visibility_th`` (:465), by evaluating
    that expression on every count; npts + 1 if none."""
    rows = (torch.arange(npts)[None] < torch.arange(npts + 1)[:, None]).float()  # row c: c ones
    ok = rows.mean(dim=-1) >= (1 - min_visibility_th)
    return int(ok.nonzero()[0]) if ok.any() else npts + 1


def min_close_count(npts, overlap_th):
    """The smallest count with ``count > npts * overlap_th`` (:492-493, an int64 tensor against a Python
    float); npts + 1 if none."""
    ok = torch.arange(npts + 1) > npts * overlap_th
    return int(ok.nonzero()[0]) if ok.any() else npts + 1


def cost_from_counts(cnt0, cnt1t, out_of0, out_of1, valid0, valid1, npts, overlap_th):  # :490-513
    mask = (cnt1t > npts * overlap_th) & (cnt0 > npts * overlap_th) & ~out_of0.unsqueeze(1) & ~out_of1.unsqueeze(-1)
    unm0 = torch.all(~mask, dim=2) | out_of1
    unm1 = torch.all(~mask, dim=1) | out_of0
    ign0, ign1 = ~valid0, ~valid1
    cost = -(cnt0 * cnt1t).clone()
    cost[unm0] = 1e6
    cost[ign0] = 1e6
    cost = cost.transpose(1, 2)
    cost[unm1] = 1e6
    cost[ign1] = 1e6
    return mask, unm0, unm1, ign0, ign1, cost.transpose(1, 2)


@torch.no_grad()
def stage_b(cnt0, cnt1t, out_of0, out_of1, valid0, valid1, npts=50, overlap_th=0.2, solver=None):
    """Labels from counts (:490-552); ``solver(cost [n0,n1] float64 ndarray) -> (rows, cols)``, the NumPy
    port below by default.  Returns (positive, m0, m1, cost, assignation)."""
    solver = solver or lsap
    cnt0, cnt1t = cnt0.long(), cnt1t.long()
    B, n0, n1 = cnt0.shape
    mask, unm0, unm1, ign0, ign1, cost = cost_from_counts(cnt0, cnt1t, out_of0, out_of1, valid0, valid1, npts, overlap_th)
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


def gt_line_matches_from_homography(lines0, lines1, valid0, valid1, shape0, shape1, H, npts=50, dist_th=5, overlap_th=0.2,
                                    min_visibility_th=0.2, solver=None):
    cnt0, cnt1t, o0, o1 = stage_a(lines0, lines1, shape0, shape1, H, npts, dist_th, min_visibility_th)
    return stage_b(cnt0, cnt1t, o0, o1, valid0, valid1, npts, overlap_th, solver)[:3]


# ---------------------------------------------------------------------------------------------
# SciPy's rectangular_lsap (scipy/optimize/rectangular_lsap) in fp64, row by row and step by step
def lsap(cost):
    """``scipy.optimize.linear_sum_assignment(cost)``: the same rows in the same order, the same scan of the
    remaining columns and the same pick among equal reduced costs, so the same assignment among optimal
    ones."""
    cost = np.asarray(cost, dtype=np.float64)
    transposed = cost.shape[1] < cost.shape[0]
    c = np.ascontiguousarray(cost.T if transposed else cost)
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    path = np.full(nc, -1)
    for cur in range(nr):
        remaining = np.arange(nc - 1, -1, -1)
        shortest = np.full(nc, np.inf)
        visited_rows, visited_cols = [], []
        num_remaining, i, min_val, sink = nc, cur, 0.0, -1
        while sink == -1:
            visited_rows.append(i)
            # one step of the scan over it = 0..num_remaining-1, vectorised: the relaxations touch one
            # column each; the sequential pick (strict < on the value, or == with an unassigned column)
            # ends on the last unassigned slot among the minima if there is one, else on the first slot
            js = remaining[:num_remaining]
            r = min_val + c[i, js] - u[i] - v[js]
            better = r < shortest[js]
            path[js[better]] = i
            shortest[js[better]] = r[better]
            sh = shortest[js]
            lowest = sh.min()
            if lowest == np.inf:
                raise ValueError("cost matrix is infeasible")
            at_min = np.nonzero(sh == lowest)[0]
            free = at_min[row4col[js[at_min]] == -1]
            index = free[-1] if free.size else at_min[0]
            min_val = lowest
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            visited_cols.append(j)
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += min_val
        for i in visited_rows:
            if i != cur:
                u[i] += min_val - shortest[col4row[i]]
        for j in visited_cols:
            v[j] -= min_val - shortest[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transposed:
        order = np.argsort(col4row)
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


# ---------------------------------------------------------------------------------------------
# margins and gating (the issue's definition; computed in fp64)
def rot_error(r32, r64, sizes64, dist_th):
    """e of one direction: the largest |fp32 - fp64| of rot_x and rot_y over the samples within
    4 dist_th of a segment (in the fp64 run)."""
    rx, ry = r64
    band = 4.0 * dist_th
    near = (ry.abs() < band) & (rx <= band) & (rx >= -(sizes64.double()[..., None, None] + band))
    if not near.any():
        return 0.0
    return float(max((r32[0].double() - rx)[near].abs().max(), (r32[1].double() - ry)[near].abs().max()))


@torch.no_grad()
def margins(lines0, lines1, shape0, shape1, H, npts, dist_th, min_visibility_th, tau0, tau1, tau_p0, tau_p1):
    """fp64 run of stage A and what it cannot decide.  Direction 0 (segments of image 0, tolerance tau0 on
    rot_x / rot_y) and direction 1: ``lo`` = samples close by more than tau in all three comparisons,
    ``und`` = samples with a comparison within tau of its threshold and none failing by more, per entry; a count may lie in [lo, lo + und].  An out_of
    flag is undecidable when the samples within tau_p of an image border straddle the count threshold."""
    lines0, lines1, H = (torch.as_tensor(np.asarray(x)).double() for x in (lines0, lines1, H))
    h0, w0 = shape0[-2:]
    h1, w1 = shape1[-2:]
    l0, l1 = clamp_lines(flat_lines(lines0), h0, w0).double(), clamp_lines(flat_lines(lines1), h1, w1).double()
    B, n0, n1 = l0.shape[0], l0.shape[1], l1.shape[1]
    pts0_1 = warp_points_torch(sample_points(l0, npts).reshape(B, n0 * npts, 2), H, inverse=False).reshape(B, n0, npts, 2)
    pts1_0 = warp_points_torch(sample_points(l1, npts).reshape(B, n1 * npts, 2), H, inverse=True).reshape(B, n1, npts, 2)

    def direction(segs, pts, tau):
        rx, ry, sizes = rotate(segs, pts)
        sz = sizes.double()[..., None, None]
        # the three comparisons as signed margins (positive: holds); NaNs (a zero-length segment) make
        # every comparison false and firmly so
        ms = torch.stack([dist_th - ry.abs(), -rx, sz - rx.abs()])
        firm_false = ~(ms > -tau)
        unsure = ms.abs() < tau
        # a sample is undecidable when a comparison within tau of its threshold can change the outcome:
        # none of the three fails firmly and at least one is within tau
        und = unsure.any(0) & ~firm_false.any(0)
        close = (ms[0] > 0) & (ms[1] >= 0) & (ms[2] >= 0)
        return (close & ~und).sum(-1), und.sum(-1)

    def flags(pts, h, w, tau_p):
        lim = torch.tensor([w, h]).to(pts)
        und = ((pts.abs() < tau_p) | ((pts - lim).abs() < tau_p)).any(-1)
        out = outside(pts, h, w)
        n_out, n_und = (out & ~und).sum(-1), und.sum(-1)
        th = min_out_count(npts, min_visibility_th)
        return (n_out < th) & (n_out + n_und >= th)

    lo0, und0 = direction(l0, pts1_0, tau0)
    lo1, und1 = direction(l1, pts0_1, tau1)
    return {"lo0": lo0.numpy().astype(np.uint8), "und0": und0.numpy().astype(np.uint8),
            "lo1t": lo1.transpose(1, 2).numpy().astype(np.uint8), "und1t": und1.transpose(1, 2).numpy().astype(np.uint8),
            "und_out_of0": flags(pts1_0, h0, w0, tau_p0).numpy(), "und_out_of1": flags(pts0_1, h1, w1, tau_p1).numpy()}


# ---------------------------------------------------------------------------------------------
# fixtures
def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "line_gt_*.npz")))


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


def check_counts(got, g, meta):
    """Stage A outputs (NumPy: cnt0, cnt1t, out_of0, out_of1) against fixture ``g``: the exact fixtures
    bit for bit; the others equal on decided entries and inside [lo, lo + und] elsewhere, out_of equal on
    decided lines."""
    for k, lo, und in (("cnt0", "lo0", "und0"), ("cnt1t", "lo1t", "und1t")):
        a = np.asarray(got[k]).astype(np.int64)
        if meta["exact"]:
            np.testing.assert_array_equal(a, g[k], err_msg=k)
            continue
        dec = g[und] == 0
        np.testing.assert_array_equal(a[dec], g[k][dec], err_msg=k)
        low, high = g[lo].astype(np.int64), g[lo].astype(np.int64) + g[und]
        assert ((a >= low) & (a <= high)).all(), f"{k}: {int(((a < low) | (a > high)).sum())} counts outside their bounds"
    for k in ("out_of0", "out_of1"):
        a = np.asarray(got[k]).astype(bool)
        dec = np.ones(a.shape, bool) if meta["exact"] else ~g["und_" + k]
        np.testing.assert_array_equal(a[dec], g[k][dec], err_msg=k)


def pair_decided(g, meta):
    """Per pair: no undecidable entry and no undecidable out_of flag (the labels are then the reference's)."""
    B = meta["B"]
    if meta["exact"]:
        return np.ones(B, bool)
    return np.array([not (g["und0"][b].any() or g["und1t"][b].any() or g["und_out_of0"][b].any() or g["und_out_of1"][b].any())
                     for b in range(B)])


def check_labels(got, g, pairs=None):
    """(positive, m0, m1) as NumPy against the fixture's, on the given pairs (all by default), no gating."""
    sel = slice(None) if pairs is None else pairs
    for a, k in zip(got, ("positive", "m0", "m1")):
        a = np.asarray(a)
        assert a.dtype == g[k].dtype, (k, a.dtype)
        np.testing.assert_array_equal(a[sel], g[k][sel], err_msg=k)
