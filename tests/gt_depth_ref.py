"""Torch-CPU restatement of the reference's pose-and-depth ground truth, for the tests only (any dtype).

``gt_matches_from_pose_depth`` is ``gluefactory/geometry/gt_generation.py:13-106``; ``sample_depth`` and
``project`` are ``geometry/depth.py:8-68``; the camera and pose arithmetic is that of
``geometry/wrappers.py`` (``Pose.inv`` / ``transform``, ``Camera.image2cam`` / ``cam2image``) on the bare
``_data`` rows; ``distort_points`` is ``geometry/utils.py:90-127`` and ``sym_epipolar_distance_all``
``geometry/epipolar.py:59-72``.  tests/golden/make_gt_depth_golden.py runs the reference itself and
asserts that this restatement gives the same bits in fp32 and in fp64; tests/test_gt_depth_golden.py
holds it to the fixtures.

Also here: the scene recipe of the random fixtures (:func:`plane_scene`), the margins that decide
which items a lower-precision run may legitimately get differently (:func:`margins`), the fixture
loader and the comparison (:func:`check_against_fixture`), shared by the CPU and the GPU tests.
"""
import glob
import json
import os

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_depth")
KEYS = ["assignment", "reward", "matches0", "matches1", "matching_scores0", "matching_scores1", "depth_keypoints0",
        "depth_keypoints1", "proj_0to1", "proj_1to0", "visible0", "visible1"]
EPS = 1e-4  # Camera.eps


# ---------------------------------------------------------------------------------------------
# the chain
def sample_fmap(pts, fmap):  # depth.py:8-17
    h, w = fmap.shape[-2:]
    grid_sample = torch.nn.functional.grid_sample
    pts = (pts / pts.new_tensor([[w, h]]) * 2 - 1)[:, None]
    interp_lin = grid_sample(fmap, pts, align_corners=False, mode="bilinear")
    interp_nn = grid_sample(fmap, pts, align_corners=False, mode="nearest")
    return torch.where(torch.isnan(interp_lin), interp_nn, interp_lin)[:, :, 0].permute(0, 2, 1)


def sample_depth(pts, depth_):  # depth.py:20-25
    depth = torch.where(depth_ > 0, depth_, depth_.new_tensor(float("nan")))
    depth = depth[:, None]
    interp = sample_fmap(pts, depth).squeeze(-1)
    valid = (~torch.isnan(interp)) & (interp > 0)
    return interp, valid


def distort_points(pts, dist, info=None):  # utils.py:90-127
    dist = dist.unsqueeze(-2)
    ndist = dist.shape[-1]
    undist = pts
    valid = torch.ones(pts.shape[:-1], device=pts.device, dtype=torch.bool)
    if ndist > 0:
        k1, k2 = dist[..., :2].split(1, -1)
        r2 = torch.sum(pts**2, -1, keepdim=True)
        radial = k1 * r2 + k2 * r2**2
        undist = undist + pts * radial
        limited = ((k2 > 0) & ((9 * k1**2 - 20 * k2) > 0)) | ((k2 <= 0) & (k1 > 0))
        limit = torch.abs(torch.where(k2 > 0, (torch.sqrt(9 * k1**2 - 20 * k2) - 3 * k1) / (10 * k2), 1 / (3 * k1)))
        valid = valid & torch.squeeze(~limited | (r2 < limit), -1)
        if info is not None:  # r^2 - limit where the rule applies, +inf elsewhere
            info["r2_margin"] = torch.where(limited.expand_as(r2), r2 - limit, torch.full_like(r2, float("inf"))).squeeze(-1)
        if ndist > 2:
            p12 = dist[..., 2:]
            p21 = p12.flip(-1)
            uv = torch.prod(pts, -1, keepdim=True)
            undist = undist + 2 * p12 * uv + p21 * (r2 + 2 * pts**2)
    return undist, valid


def cam_size(cam):
    return cam[..., :2]


def image2cam(cam, p2d):  # wrappers.py:371-373, 393-398: no undistortion
    p = (p2d - cam[..., 4:6].unsqueeze(-2)) / cam[..., 2:4].unsqueeze(-2)
    return torch.cat([p, p.new_ones(p.shape[:-1] + (1,))], -1)


def cam2image(cam, p3d, info=None):  # wrappers.py:337-343, 354-385
    z = p3d[..., -1]
    visible = z > EPS
    zc = z.clamp(min=EPS)
    p2d = p3d[..., :-1] / zc.unsqueeze(-1)
    p2d, mask = distort_points(p2d, cam[..., 6:], info)
    p2d = p2d * cam[..., 2:4].unsqueeze(-2) + cam[..., 4:6].unsqueeze(-2)
    size = cam_size(cam).unsqueeze(-2)
    inside = torch.all((p2d >= 0) & (p2d <= (size - 1)), -1)
    if info is not None:
        info["z"] = z
        info["bound"] = torch.minimum(p2d, size - 1 - p2d).abs().min(-1).values  # distance to the nearest image bound
    return p2d, visible & mask & inside


def pose_R(T):
    return T[..., :9].reshape(T.shape[:-1] + (3, 3))


def pose_t(T):
    return T[..., -3:]


def pose_from_Rt(R, t):
    return torch.cat([R.flatten(start_dim=-2), t], -1)


def pose_inv(T):  # wrappers.py:173-177
    R = pose_R(T).transpose(-1, -2)
    t = -(R @ pose_t(T).unsqueeze(-1)).squeeze(-1)
    return pose_from_Rt(R, t)


def pose_transform(T, p3d):  # wrappers.py:186-193
    return p3d @ pose_R(T).transpose(-1, -2) + pose_t(T).unsqueeze(-2)


def calibration_matrix(cam):  # wrappers.py:278-291
    K = torch.zeros(*cam.shape[:-1], 3, 3, dtype=cam.dtype)
    K[..., 0, 2] = cam[..., 4]
    K[..., 1, 2] = cam[..., 5]
    K[..., 0, 0] = cam[..., 2]
    K[..., 1, 1] = cam[..., 3]
    K[..., 2, 2] = 1.0
    return K


def skew_symmetric(v):  # utils.py:44-61
    z = torch.zeros_like(v[..., 0])
    return torch.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], dim=-1).reshape(
        v.shape[:-1] + (3, 3))


def to_homogeneous(p):
    return torch.cat([p, p.new_ones(p.shape[:-1] + (1,))], dim=-1)


def sym_epipolar_distance_all(p0, p1, E, eps=1e-15):  # epipolar.py:59-72
    p0, p1 = to_homogeneous(p0), to_homogeneous(p1)
    p1_E_p0 = torch.einsum("...mi,...ij,...nj->...nm", p1, E, p0).abs()
    E_p0 = torch.einsum("...ij,...nj->...ni", E, p0)
    Et_p1 = torch.einsum("...ij,...mi->...mj", E, p1)
    d0 = p1_E_p0 / (E_p0[..., None, 0] ** 2 + E_p0[..., None, 1] ** 2 + eps).sqrt()
    d1 = p1_E_p0 / (Et_p1[..., None, :, 0] ** 2 + Et_p1[..., None, :, 1] ** 2 + eps).sqrt()
    return (d0 + d1) / 2


def project(kpi, di, depthj, cam_i, cam_j, T_itoj, validi, ccth=None, info=None):  # depth.py:37-68
    kpi_3d_i = image2cam(cam_i, kpi)
    kpi_3d_i = kpi_3d_i * di[..., None]
    kpi_3d_j = pose_transform(T_itoj, kpi_3d_i)
    kpi_j, validj = cam2image(cam_j, kpi_3d_j, info)
    validi = validi & validj
    if depthj is None or ccth is None:
        return kpi_j, validi & validj
    dj, validj = sample_depth(kpi_j, depthj)
    kpi_j_3d_j = image2cam(cam_j, kpi_j) * dj[..., None]
    back = {} if info is not None else None
    kpi_j_i, validj_i = cam2image(cam_i, pose_transform(pose_inv(T_itoj), kpi_j_3d_j), back)
    cc = ((kpi - kpi_j_i) ** 2).sum(-1)
    consistent = cc < ccth
    if info is not None:
        info["cc"] = cc
        info["back"] = back
        info["cc_xy"] = kpi_j
    return kpi_j, validi & consistent & validj_i & validj


def _data(x):
    return getattr(x, "_data", x)


@torch.no_grad()
def gt_matches_from_pose_depth(kp0, kp1, data, pos_th=3, neg_th=5, epi_th=None, cc_th=None, info=None, **kw):
    """gt_generation.py:13-106 with the cameras and poses as rows (or objects with ``_data``)."""
    if kp0.shape[1] == 0 or kp1.shape[1] == 0:  # :17-25
        b_size, n_kp0 = kp0.shape[:2]
        n_kp1 = kp1.shape[1]
        assignment = torch.zeros(b_size, n_kp0, n_kp1, dtype=torch.bool, device=kp0.device)
        m0 = -torch.ones_like(kp0[:, :, 0]).long()
        m1 = -torch.ones_like(kp1[:, :, 0]).long()
        return assignment, m0, m1
    camera0, camera1 = _data(data["view0"]["camera"]), _data(data["view1"]["camera"])
    T_0to1, T_1to0 = _data(data["T_0to1"]), _data(data["T_1to0"])
    depth0 = data["view0"].get("depth")
    depth1 = data["view1"].get("depth")
    if "depth_keypoints0" in kw and "depth_keypoints1" in kw:
        d0, valid0 = kw["depth_keypoints0"], kw["valid_depth_keypoints0"]
        d1, valid1 = kw["depth_keypoints1"], kw["valid_depth_keypoints1"]
    else:
        assert depth0 is not None and depth1 is not None
        d0, valid0 = sample_depth(kp0, depth0)
        d1, valid1 = sample_depth(kp1, depth1)
    i0 = {} if info is not None else None
    i1 = {} if info is not None else None
    kp0_1, visible0 = project(kp0, d0, depth1, camera0, camera1, T_0to1, valid0, ccth=cc_th, info=i0)
    kp1_0, visible1 = project(kp1, d1, depth0, camera1, camera0, T_1to0, valid1, ccth=cc_th, info=i1)
    mask_visible = visible0.unsqueeze(-1) & visible1.unsqueeze(-2)

    dist0 = torch.sum((kp0_1.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2, -1)
    dist1 = torch.sum((kp0.unsqueeze(-2) - kp1_0.unsqueeze(-3)) ** 2, -1)
    dist_raw = torch.max(dist0, dist1)
    inf = dist_raw.new_tensor(float("inf"))
    dist = torch.where(mask_visible, dist_raw, inf)

    min0 = dist.min(-1).indices
    min1 = dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < pos_th**2)

    negative0 = (dist0.min(-1).values > neg_th**2) & valid0
    negative1 = (dist1.min(-2).values > neg_th**2) & valid1

    unmatched = min0.new_tensor(-1)
    ignore = min0.new_tensor(-2)
    m0 = torch.where(positive.any(-1), min0, ignore)
    m1 = torch.where(positive.any(-2), min1, ignore)
    m0 = torch.where(negative0, unmatched, m0)
    m1 = torch.where(negative1, unmatched, m1)

    F = (calibration_matrix(camera1).inverse().transpose(-1, -2) @ (skew_symmetric(pose_t(T_0to1)) @ pose_R(T_0to1))
         @ calibration_matrix(camera0).inverse())
    epi_all = sym_epipolar_distance_all(kp0, kp1, F)
    epi_dist = epi_all
    m0_pre, m1_pre = m0, m1
    emin0 = emin1 = None
    if epi_th is not None:  # :85-91
        mask_ignore = (m0.unsqueeze(-1) == ignore) & (m1.unsqueeze(-2) == ignore)
        epi_dist = torch.where(mask_ignore, epi_dist, inf)
        emin0, emin1 = epi_dist.min(-1).values, epi_dist.min(-2).values
        exclude0 = emin0 > neg_th
        exclude1 = emin1 > neg_th
        m0 = torch.where((~valid0) & exclude0, ignore.new_tensor(-1), m0)
        m1 = torch.where((~valid1) & exclude1, ignore.new_tensor(-1), m1)
    if info is not None:
        info.update({"p0": i0, "p1": i1, "dist": dist, "dist_raw": dist_raw, "dist0": dist0, "dist1": dist1,
                     "epi_all": epi_all, "epi": epi_dist, "valid0": valid0, "valid1": valid1, "m0_pre": m0_pre,
                     "m1_pre": m1_pre, "emin0": emin0, "emin1": emin1})
    return {
        "assignment": positive,
        "reward": (dist < pos_th**2).float() - (epi_dist > neg_th).float(),
        "matches0": m0,
        "matches1": m1,
        "matching_scores0": (m0 > -1).float(),
        "matching_scores1": (m1 > -1).float(),
        "depth_keypoints0": d0,
        "depth_keypoints1": d1,
        "proj_0to1": kp0_1,
        "proj_1to0": kp1_0,
        "visible0": visible0,
        "visible1": visible1,
    }


# ---------------------------------------------------------------------------------------------
# the scene of the random fixtures and of the end-to-end test
def _rot(axis_angle):
    th = np.linalg.norm(axis_angle)
    k = axis_angle / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def plane_scene(seed, B, M, N, n_dist=0, width=320, height=240, holes=12, hole_max=(48, 36), noise=1.0):
    """A tilted plane at depth ~5 seen by two cameras (rotation ~0.08 rad, baseline <= 0.4): analytic
    depth maps at the pixel centres with ``holes`` zero rectangles each; keypoints of image 0 uniform,
    half of image 1 the reprojection of image-0 points (through this restatement in fp64) plus
    ``noise`` px of Gaussian noise, the rest uniform, shuffled.  Returns fp32 NumPy arrays."""
    rng = np.random.Generator(np.random.PCG64(seed))
    W, H = width, height
    f = 0.95 * W
    cam = np.zeros((B, 6 + n_dist))
    cam[:, :6] = [W, H, f, f * 1.02, W / 2 + 1.5, H / 2 - 2.5]
    if n_dist >= 2:
        cam[:, 6:8] = [-0.06, 0.015]
    if n_dist == 4:
        cam[:, 8:10] = [0.002, -0.0015]
    cam0, cam1 = cam.copy(), cam.copy()
    cam1[:, 2:4] *= 1.03
    T01 = np.zeros((B, 12))
    depth = np.zeros((2, B, H, W))
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    for b in range(B):
        aa = rng.standard_normal(3)
        R = _rot(aa / np.linalg.norm(aa) * 0.08)
        t = rng.standard_normal(3)
        t = t / np.linalg.norm(t) * rng.uniform(0.2, 0.4)
        T01[b] = np.concatenate([R.reshape(9), t])
        n = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), 1.0])
        n1 = R @ n
        for k, (c, nn, h) in enumerate(((cam0[b], n, 5.0), (cam1[b], n1, 5.0 + n1 @ t))):
            ray = np.stack([(u - c[4]) / c[2], (v - c[5]) / c[3], np.ones_like(u)], -1)
            depth[k, b] = np.round(h / (ray @ nn) * 4096.0) / 4096.0  # short mantissas: the fixture compresses
            for _ in range(holes):
                hw, hh = rng.integers(8, hole_max[0]), rng.integers(8, hole_max[1])
                x0, y0 = rng.integers(0, W - hw), rng.integers(0, H - hh)
                depth[k, b, y0:y0 + hh, x0:x0 + hw] = 0.0
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).double()  # noqa: E731
    T01_t = t64(T01)
    T10_t = pose_inv(T01_t)
    size = np.array([W - 1.0, H - 1.0])
    kp0 = rng.random((B, M, 2)) * size
    kp1 = rng.random((B, N, 2)) * size
    d0, v0 = sample_depth(t64(kp0), t64(depth[0]))
    p01, vis0 = project(t64(kp0), d0, None, t64(cam0), t64(cam1), T01_t, v0)
    nw = min(N // 2, M)
    for b in range(B):
        src = np.nonzero(vis0[b].numpy())[0]
        src = src[rng.permutation(len(src))][:nw]
        kp1[b, :len(src)] = np.clip(p01[b, src].numpy() + rng.standard_normal((len(src), 2)) * noise, 0.0, size)
        kp1[b] = kp1[b, rng.permutation(N)]
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))  # noqa: E731
    return {"keypoints0": f32(kp0), "keypoints1": f32(kp1), "depth0": f32(depth[0]), "depth1": f32(depth[1]),
            "camera0": f32(cam0), "camera1": f32(cam1), "T_0to1": f32(T01), "T_1to0": f32(T10_t.numpy())}


def feed_of(g, dtype=torch.float32, device="cpu", maps=True):
    """The reference's ``data`` dict from fixture arrays (cameras and poses as rows)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).to(device)  # noqa: E731
    view0, view1 = {"camera": t(g["camera0"])}, {"camera": t(g["camera1"])}
    if maps and "depth0" in g:
        view0["depth"], view1["depth"] = t(g["depth0"]), t(g["depth1"])
    return {"keypoints0": t(g["keypoints0"]), "keypoints1": t(g["keypoints1"]), "view0": view0, "view1": view1,
            "T_0to1": t(g["T_0to1"]), "T_1to0": t(g["T_1to0"])}


# ---------------------------------------------------------------------------------------------
# tolerances and margins
def _run(g, dtype, pos_th, neg_th, epi_th, cc_th, kw=None):
    d = feed_of(g, dtype)
    info = {}
    kw = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in (kw or {}).items()}
    out = gt_matches_from_pose_depth(d["keypoints0"], d["keypoints1"], d, pos_th, neg_th, epi_th, cc_th, info=info, **kw)
    return out, info


def _dev(a, b, sel=None):
    """max |a - b| over entries finite in both (and selected)."""
    a, b = a.double(), b.double()
    ok = torch.isfinite(a) & torch.isfinite(b)
    if sel is not None:
        ok = ok & sel
    return float((a - b)[ok].abs().max()) if bool(ok.any()) else 0.0


def tolerances(g, pos_th, neg_th, epi_th, cc_th, kw=None):
    """4 x the largest deviation between the chain's own fp32 and fp64 runs, per quantity."""
    (o32, i32), (o64, i64) = _run(g, torch.float32, pos_th, neg_th, epi_th, cc_th, kw), _run(
        g, torch.float64, pos_th, neg_th, epi_th, cc_th, kw)
    tol = {}
    both = lambda k: max(_dev(i32["p0"][k], i64["p0"][k]), _dev(i32["p1"][k], i64["p1"][k]))  # noqa: E731
    tol["proj"] = 4 * max(_dev(o32["proj_0to1"], o64["proj_0to1"], o64["visible0"][..., None]),
                          _dev(o32["proj_1to0"], o64["proj_1to0"], o64["visible1"][..., None]))
    tol["depth"] = 4 * max(_dev(o32["depth_keypoints0"], o64["depth_keypoints0"]),
                           _dev(o32["depth_keypoints1"], o64["depth_keypoints1"]))
    tol["z"] = 4 * both("z")
    tol["bound"] = 4 * max(_dev(i32[p]["bound"], i64[p]["bound"], i64[p]["bound"] < 8.0) for p in ("p0", "p1"))
    tol["r2"] = 4 * both("r2_margin") if "r2_margin" in i64["p0"] else 0.0
    if cc_th is not None:
        tol["cc"] = 4 * max(_dev(i32[p]["cc"], i64[p]["cc"], i64[p]["cc"] < 4.0 * max(cc_th, 1.0)) for p in ("p0", "p1"))
    near = i64["dist_raw"] < 4.0 * max(pos_th, neg_th) ** 2
    tol["tau"] = 4 * _dev(i32["dist_raw"], i64["dist_raw"], near)
    tol["epi"] = 4 * _dev(i32["epi_all"], i64["epi_all"], i64["epi_all"] < 4.0 * neg_th)
    return tol


def _frac_margin(xy):
    """Distance of the sampling coordinate (ix, iy) to the nearest integer: where the bilinear
    footprint or the nearest sample changes."""
    ix = xy[..., 0] - 0.5
    iy = xy[..., 1] - 0.5
    fr = lambda a: (a - a.round()).abs()  # noqa: E731
    half = lambda a: ((a - a.floor()) - 0.5).abs()  # noqa: E731
    m = torch.minimum(torch.minimum(fr(ix), fr(iy)), torch.minimum(half(ix), half(iy)))
    return torch.where(torch.isfinite(m), m, torch.full_like(m, float("inf")))


def margins(g, pos_th, neg_th, epi_th, cc_th, tol, kw=None):
    """The fp64 run and the undecidable masks: points [B,M] / [B,N] (``visible``), rows / columns
    (labels) and reward entries [B,M,N].

    A point is undecidable when one of its boolean tests lies within tolerance of its threshold:
    z - 1e-4, an image bound, r^2 - limit, the consistency distance against th_consistency (those of
    the way back included) -- these only for a point with valid depth, since without it the point is
    not visible anyway -- or a sampling coordinate within tolerance of where its footprint changes.
    A row is undecidable when make_gt_golden.py's row rule holds on the masked dist; or it is an
    undecidable point; or an undecidable point of the other image has unmasked dist < pos_th^2 + tau
    to it; or, with th_epi, its epipolar minimum is within tolerance of neg_th, its top-2 gap is
    under tolerance while the runner-up's label is undecidable, or a column with an undecidable label
    lies within neg_th + tolerance of it.  Columns likewise.  A reward entry is undecidable when its
    dist is within tau of pos_th^2, its epi within tolerance of neg_th, its row or column is an
    undecidable point while its unmasked dist is below pos_th^2 + tau (elsewhere the mask changes nothing), or (th_epi) its row's or column's label is undecidable and its epi is below
    neg_th + tolerance (the mask of :87 could flip what :95 compares)."""
    o, info = _run(g, torch.float64, pos_th, neg_th, epi_th, cc_th, kw)
    p2, n2 = float(pos_th) ** 2, float(neg_th) ** 2
    tau = tol["tau"]
    pre = kw is not None

    def point_und(pi, own_xy, valid):
        u = (pi["z"] - EPS).abs() < tol["z"]
        u |= pi["bound"] < max(tol["bound"], tol["proj"])
        if "r2_margin" in pi:
            u |= pi["r2_margin"].abs() < tol["r2"]
        if "cc" in pi:
            u |= (pi["cc"] - cc_th).abs() < tol["cc"]
            u |= _frac_margin(pi["cc_xy"]) < tol["proj"]
            b = pi["back"]
            u |= (b["z"] - EPS).abs() < tol["z"]
            u |= b["bound"] < max(tol["bound"], tol["proj"])
            if "r2_margin" in b:
                u |= b["r2_margin"].abs() < tol["r2"]
        u &= valid  # a point without valid depth fails `visible` whatever its other tests say ...
        if not pre:  # ... but whether its depth is valid hangs on the footprint of its own sample:
            u |= _frac_margin(own_xy) < 1e-4  # 4 x the 2e-5 px the fp32 coordinate is off at 512 px
        return u

    d64 = feed_of(g, torch.float64)
    und_p0 = point_und(info["p0"], d64["keypoints0"], info["valid0"])
    und_p1 = point_und(info["p1"], d64["keypoints1"], info["valid1"])

    d, draw = info["dist"], info["dist_raw"]
    draw = torch.where(torch.isnan(draw), torch.full_like(draw, float("inf")), draw)

    def side(dm, dh, valid):
        inf = dm.new_full(dm.shape[:-1] + (1,), float("inf"))
        top = torch.cat([dm, inf], -1).topk(2, dim=-1, largest=False).values
        gap = top[..., 1] - top[..., 0]
        gap = torch.where(torch.isnan(gap), torch.full_like(gap, float("inf")), gap)  # inf - inf: nothing to tie
        half = dh.min(-1).values
        half_und = ((half - n2).abs() < tau) & valid
        return top[..., 0], gap, dm.argmin(-1), half_und

    rmin, rgap, rarg, rhalf = side(d, info["dist0"], info["valid0"])
    cmin, cgap, carg, chalf = side(d.transpose(1, 2), info["dist1"].transpose(1, 2), info["valid1"])
    und_r = ((rmin - p2).abs() < tau) | rhalf | ((rmin < p2 + tau) & ((rgap < tau) | (cgap.gather(1, rarg) < tau)))
    und_c = ((cmin - p2).abs() < tau) | chalf | ((cmin < p2 + tau) & ((cgap < tau) | (rgap.gather(1, carg) < tau)))
    reach = draw < p2 + tau
    und_r |= und_p0 | (reach & und_p1[:, None, :]).any(2)
    und_c |= und_p1 | (reach & und_p0[:, :, None]).any(1)
    und_e = ((d - p2).abs() < tau) | ((info["epi"] - neg_th).abs() < tol["epi"])
    und_e |= (und_p0[:, :, None] | und_p1[:, None, :]) & reach  # visibility only masks dist, and only dist < pos_th^2 counts
    if epi_th is not None:
        ea = info["epi_all"]
        lab_r, lab_c = und_r.clone(), und_c.clone()  # labels before the epipolar step

        def epi_side(em, lab_other, own_invalid):
            inf = em.new_full(em.shape[:-1] + (1,), float("inf"))
            top = torch.cat([em, inf], -1).topk(2, dim=-1, largest=False)
            gap = top.values[..., 1] - top.values[..., 0]
            gap = torch.where(torch.isnan(gap), torch.full_like(gap, float("inf")), gap)
            runner = top.indices[..., 1].clamp(max=em.shape[-1] - 1)
            u = (top.values[..., 0] - neg_th).abs() < tol["epi"]
            u |= (gap < tol["epi"]) & lab_other.gather(1, runner)
            return u & own_invalid

        near_r = ((ea < neg_th + tol["epi"]) & lab_c[:, None, :]).any(2)
        near_c = ((ea < neg_th + tol["epi"]) & lab_r[:, :, None]).any(1)
        und_r |= epi_side(info["epi"], lab_c, ~info["valid0"]) | (near_r & ~info["valid0"])
        und_c |= epi_side(info["epi"].transpose(1, 2), lab_r, ~info["valid1"]) | (near_c & ~info["valid1"])
        und_e |= (lab_r[:, :, None] | lab_c[:, None, :]) & (ea < neg_th + tol["epi"])
    return {"und_p0": und_p0.numpy(), "und_p1": und_p1.numpy(), "und_rows": und_r.numpy(), "und_cols": und_c.numpy(),
            "und_reward": und_e.numpy(), "out": o, "info": info}


# ---------------------------------------------------------------------------------------------
# fixtures
def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "gtd_*.npz")))


def load_fixture(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    g = {k: z[k] for k in z.files if k != "meta_json"}
    meta = json.loads(str(z["meta_json"]))
    B, M, N = meta["B"], meta["M"], meta["N"]
    for v in meta["variants"]:
        p = v["prefix"]
        a = np.zeros((B, M, N), bool)
        t = g.pop(p + "assignment_idx")
        a[t[:, 0], t[:, 1], t[:, 2]] = True
        g[p + "assignment"] = a
        g[p + "reward"] = g.pop(p + "reward_i8").astype(np.float32)
        und = np.zeros((B, M, N), bool)
        t = g.pop(p + "und_reward_idx")
        und[t[:, 0], t[:, 1], t[:, 2]] = True
        g[p + "und_reward"] = und
    return g, meta


def variant_conf(v):
    return {"th_positive": v["th_positive"], "th_negative": v["th_negative"], "th_epi": v["th_epi"],
            "th_consistency": v["th_consistency"]}


def precomputed_kw(g, meta, dtype=torch.float32, device="cpu"):
    if not meta.get("precomputed"):
        return {}
    return {"depth_keypoints0": torch.from_numpy(g["in_depth_keypoints0"]).to(dtype).to(device),
            "depth_keypoints1": torch.from_numpy(g["in_depth_keypoints1"]).to(dtype).to(device),
            "valid_depth_keypoints0": torch.from_numpy(g["in_valid0"]).to(device),
            "valid_depth_keypoints1": torch.from_numpy(g["in_valid1"]).to(device)}


def _bits(a):
    return a if a.dtype == bool else a.view(np.uint8)


def compare(got, want, und, tol, exact, reward=True):
    """``got`` against ``want`` (dicts of NumPy arrays under the twelve keys; ``want`` may carry the
    continuous outputs in fp64).  exact: bit for bit, NaN positions equal.  Otherwise every decidable
    item equal, the continuous outputs within tolerance where valid / visible."""
    keys = [k for k in KEYS if reward or k != "reward"]
    if exact:
        for k in keys:
            assert got[k].dtype == want[k].dtype, k
            np.testing.assert_array_equal(_bits(np.ascontiguousarray(got[k])), _bits(np.ascontiguousarray(want[k])), err_msg=k)
        return
    ok_r, ok_c = ~und["und_rows"], ~und["und_cols"]
    for k, ok in (("matches0", ok_r), ("matches1", ok_c), ("matching_scores0", ok_r), ("matching_scores1", ok_c),
                  ("visible0", ~und["und_p0"]), ("visible1", ~und["und_p1"])):
        np.testing.assert_array_equal(got[k][ok], want[k][ok], err_msg=k)
    ok_a = ok_r[:, :, None] & ok_c[:, None, :]
    np.testing.assert_array_equal(got["assignment"][ok_a], want["assignment"][ok_a], err_msg="assignment")
    if reward:
        ok_e = ~und["und_reward"]
        np.testing.assert_array_equal(got["reward"][ok_e], want["reward"][ok_e], err_msg="reward")
    for s in "01":
        v = np.isfinite(want["depth_keypoints" + s]) & (want["depth_keypoints" + s] > 0) & ~und["und_p" + s]
        np.testing.assert_allclose(got["depth_keypoints" + s][v].astype(np.float64), want["depth_keypoints" + s][v], rtol=0,
                                   atol=tol["depth"], err_msg="depth_keypoints" + s)
    for k, s in (("proj_0to1", "0"), ("proj_1to0", "1")):
        v = want["visible" + s] & ~und["und_p" + s]
        np.testing.assert_allclose(got[k][v].astype(np.float64), want[k][v], rtol=0, atol=tol["proj"], err_msg=k)


def check_against_fixture(got, g, meta, variant, reward=True):
    p = variant["prefix"]
    want = {k: g[p + k] for k in KEYS}
    if not meta["exact"]:
        for k in ("depth_keypoints0", "depth_keypoints1", "proj_0to1", "proj_1to0"):
            want[k] = g[p + k + "_f64"]
    und = {k: g[p + k] for k in ("und_p0", "und_p1", "und_rows", "und_cols", "und_reward")} if not meta["exact"] else None
    compare(got, want, und, variant.get("tol"), meta["exact"], reward)
