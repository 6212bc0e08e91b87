"""Line ground truth on the HIP library: the reference's ``gt_line_matches_from_homography``
(``gluefactory/geometry/gt_generation.py:409-558``) and ``gt_line_matches_from_pose_depth`` (:207-406),
the ``use_lines`` halves of its ``matchers.homography_matcher`` and ``matchers.depth_matcher``, which
feed ``GlueStick.loss`` with ``gt_line_assignment`` / ``gt_line_matches0`` / ``gt_line_matches1``.

The reference builds two ``[B, n0, n1, npts, 2]`` tensors, copies the ``[B, n0, n1]`` cost to the host,
runs SciPy's ``linear_sum_assignment`` once per pair and copies the result back.  Here (csrc/gt_lines.hip):

* stage A, :func:`close_point_counts_from_homography` -- the two ``[B, n0, n1]`` counts of close samples
  and the out-of-image flags, with nothing of size ``n0 * n1 * npts`` written;
* stage B, :func:`line_labels_from_counts` -- mask, fp64 cost, assignment and labels, all on the device;
  the assignment is SciPy's algorithm (``rectangular_lsap``) with its scan order and tie rule, one pair per
  wave, so the labels are the reference's even where several assignments are optimal;
* :func:`linear_sum_assignment` -- that solver alone, batched.

The point-to-segment test follows the reference's CPU path in fp32 (segment length rounded to fp16, every
product and sum rounded on its own).  The reference's CUDA branch additionally casts the rotation and the
centred samples to fp16 "to reduce memory"; that is deliberately not reproduced: nothing that large is
stored here, and the fixtures come from the CPU path.

The pose-and-depth variant has the same two stages behind a projection front end:
:func:`close_point_counts_from_pose_depth` samples the depth maps along the lines and projects the
samples through the cameras and the pose (the chain of :mod:`~lightglue_amd.depth_matcher`, with no
consistency check: the reference has none for lines); :func:`line_labels_from_visibility_counts` compares
each count with a threshold that follows the line's number of visible samples, keeps ``out_of`` out of
``mask_close`` and ignores lines without enough valid depth.  One difference from the reference: a
``data`` without ``view*["image"]`` falls back to the depth map's size for the out-of-image test (the
reference raises a ``KeyError``).

``matchers.homography_matcher`` and ``matchers.depth_matcher`` keep raising on ``use_lines: True`` (their
tests pin that); the capability is :class:`LineHomographyMatcher`, registered as
``matchers.line_homography_matcher``, and :class:`LineDepthMatcher`, ``matchers.line_depth_matcher``.
"""
import ctypes

import torch

from . import _lib
from ._native import _ptr
from .depth_matcher import DepthMatcher, _depth, _rows
from .gt_matcher import HomographyMatcher, gt_matches_from_homography


def _need_device(*tensors):
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError("lightglue_amd: inputs must be on a HIP (cuda) device; there is no CPU path")


def _flat_lines(lines):
    """The reference's accepted layouts (:430-437): [B,n,4], [B,n,2,2], or [B,n,k,2] taking the first and
    the last point."""
    if lines.shape[-2:] == (2, 2):
        lines = torch.flatten(lines, -2)
    elif lines.dim() == 4:
        lines = torch.cat([lines[:, :, 0], lines[:, :, -1]], dim=2)
    assert lines.dim() == 3 and lines.shape[-1] == 4, f"lines must be [B,n,4], [B,n,2,2] or [B,n,k,2], got {tuple(lines.shape)}"
    return lines.detach().to(torch.float32).contiguous()


def _check_npts(npts):
    npts = int(npts)
    if not 2 <= npts <= 255:
        raise ValueError(f"npts must be in 2..255 (counts are uint8), got {npts}")
    return npts


def line_count_thresholds(npts, min_visibility_th, overlap_th):
    """The integer thresholds the kernels compare counts with, derived on the host by evaluating the
    reference's fp32 expressions for every count: the smallest number of outside samples with
    ``mean >= 1 - min_visibility_th`` and the smallest count with ``count > npts * overlap_th``
    (``npts + 1`` when none qualifies)."""
    a, b = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().lg_gt_line_thresholds(_check_npts(npts), float(min_visibility_th), float(overlap_th),
                                                 ctypes.byref(a), ctypes.byref(b)), "lg_gt_line_thresholds")
    return a.value, b.value


def close_point_counts_from_homography(lines0, lines1, shape0, shape1, H, npts=50, dist_th=5, min_visibility_th=0.2):
    """Stage A.  Returns ``num_close_pts0`` [B,n0,n1] (samples of line j of image 1, warped by H^-1, close to
    segment i of image 0), ``num_close_pts1_t`` [B,n0,n1] (samples of line i, warped by H, close to segment j
    of image 1), both uint8, and the bool flags ``out_of0`` [B,n1], ``out_of1`` [B,n0] (:461-470)."""
    _need_device(lines0, lines1, H)
    npts = _check_npts(npts)
    dev = lines0.device
    l0, l1 = _flat_lines(lines0), _flat_lines(lines1)
    B, n0 = l0.shape[:2]
    n1 = l1.shape[1]
    assert l1.shape[0] == B
    H = H.detach().to(torch.float32)
    if H.dim() == 2:
        H = H[None].expand(B, 3, 3)
    H = H.contiguous()
    assert H.shape == (B, 3, 3)
    h0, w0 = (int(v) for v in shape0[-2:])
    h1, w1 = (int(v) for v in shape1[-2:])
    cnt0 = torch.zeros((B, n0, n1), dtype=torch.uint8, device=dev)
    cnt1t = torch.zeros((B, n0, n1), dtype=torch.uint8, device=dev)
    out0 = torch.zeros((B, n1), dtype=torch.bool, device=dev)
    out1 = torch.zeros((B, n0), dtype=torch.bool, device=dev)
    if B == 0 or n0 == 0 or n1 == 0:
        return cnt0, cnt1t, out0, out1
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_gt_line_counts_workspace_bytes(B, n0, n1, npts, ctypes.byref(nb)), "lg_gt_line_counts_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(
            lib.lg_gt_line_counts_homography(_ptr(l0), _ptr(l1), _ptr(H), B, n0, n1, h0, w0, h1, w1, npts, float(dist_th),
                                             float(min_visibility_th), _ptr(cnt0), _ptr(cnt1t), _ptr(out0), _ptr(out1),
                                             _ptr(ws), nb.value, ctypes.c_void_p(stream)),
            "lg_gt_line_counts_homography",
        )
    return cnt0, cnt1t, out0, out1


def _empty_labels(B, n0, n1, dev):
    # :554-556: an all-false `positive` and two empty [B, 0] tensors of its dtype
    positive = torch.zeros((B, n0, n1), dtype=torch.bool, device=dev)
    no_matches = torch.zeros((B, 0), dtype=torch.bool, device=dev)
    return positive, no_matches, no_matches


def line_labels_from_counts(cnt0, cnt1t, out_of0, out_of1, valid0, valid1, npts, overlap_th):
    """Stage B (:490-552): ``mask_close``, the unmatched / ignored lines, the fp64 cost, the assignment and
    the labels.  Returns ``(positive bool [B,n0,n1], m0 int64 [B,n0], m1 int64 [B,n1])`` with -1 for
    unmatched and -2 for ignored (invalid) lines."""
    _need_device(cnt0, cnt1t, out_of0, out_of1, valid0, valid1)
    npts = _check_npts(npts)
    dev = cnt0.device
    B, n0, n1 = cnt0.shape
    assert cnt1t.shape == (B, n0, n1) and out_of0.shape == (B, n1) and out_of1.shape == (B, n0)
    assert valid0.shape == (B, n0) and valid1.shape == (B, n1)
    if B == 0 or n0 == 0 or n1 == 0:
        return _empty_labels(B, n0, n1, dev)
    u8 = [t.detach().to(torch.uint8).contiguous() for t in (cnt0, cnt1t)]
    flags = [t.detach().to(torch.bool).contiguous() for t in (out_of0, out_of1, valid0, valid1)]
    positive = torch.empty((B, n0, n1), dtype=torch.bool, device=dev)
    m0 = torch.empty((B, n0), dtype=torch.int64, device=dev)
    m1 = torch.empty((B, n1), dtype=torch.int64, device=dev)
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_gt_line_labels_workspace_bytes(B, n0, n1, ctypes.byref(nb)), "lg_gt_line_labels_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(
            lib.lg_gt_line_labels(_ptr(u8[0]), _ptr(u8[1]), _ptr(flags[0]), _ptr(flags[1]), _ptr(flags[2]), _ptr(flags[3]),
                                  B, n0, n1, npts, float(overlap_th), _ptr(positive), _ptr(m0), _ptr(m1), _ptr(ws), nb.value,
                                  ctypes.c_void_p(stream)),
            "lg_gt_line_labels",
        )
    return positive, m0, m1


def gt_line_matches_from_homography(lines0, lines1, valid_lines0, valid_lines1, shape0, shape1, H, npts=50, dist_th=5,
                                    overlap_th=0.2, min_visibility_th=0.2):
    """``gt_generation.py:409-558`` on the device: stage A, then stage B.  Lines that reproject outside the
    other image, or far from every line there, are UNMATCHED (-1); invalid lines are IGNORED (-2)."""
    _need_device(lines0, lines1, valid_lines0, valid_lines1, H)
    cnt0, cnt1t, out0, out1 = close_point_counts_from_homography(lines0, lines1, shape0, shape1, H, npts, dist_th,
                                                                 min_visibility_th)
    return line_labels_from_counts(cnt0, cnt1t, out0, out1, valid_lines0, valid_lines1, npts, overlap_th)


def line_depth_thresholds(npts, min_visibility_th, overlap_th):
    """The integer thresholds of the pose-and-depth variant, derived on the host by evaluating the
    reference's fp32 expressions for every count: ``min_close`` (a list of ``npts + 1``: for a line with v
    visible samples the smallest count c with ``float(c) > float(v) * overlap_th``, ``npts + 1`` when none
    qualifies), the smallest number of outside samples with ``mean >= 1 - min_visibility_th`` and the
    smallest number of samples with valid depth that is not ignored (``mean < min_visibility_th``)."""
    npts = _check_npts(npts)
    tab = (ctypes.c_int32 * (npts + 1))()
    a, b = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().lg_gt_line_depth_thresholds(npts, float(min_visibility_th), float(overlap_th), tab,
                                                       ctypes.byref(a), ctypes.byref(b)), "lg_gt_line_depth_thresholds")
    return list(tab), a.value, b.value


def close_point_counts_from_pose_depth(lines0, lines1, data, npts=50, dist_th=5, min_visibility_th=0.5):
    """Stage A of the pose-and-depth variant (:240-316).  ``data`` holds ``view0`` / ``view1`` (``camera``,
    ``depth`` and, for the out-of-image test, ``image``; without it the depth map's size), ``T_0to1`` and
    ``T_1to0``, taken as :func:`~lightglue_amd.depth_matcher.gt_matches_from_pose_depth` takes them.
    Returns a dict: ``num_close_pts0`` / ``num_close_pts1_t`` [B,n0,n1] uint8 (visible samples only),
    ``out_of0`` [B,n1] / ``out_of1`` [B,n0] bool, ``ignore_depth0`` [B,n0] / ``ignore_depth1`` [B,n1] bool
    (too few samples with valid depth) and ``num_visible0`` [B,n0] / ``num_visible1`` [B,n1] uint8."""
    _need_device(lines0, lines1)
    npts = _check_npts(npts)
    dev = lines0.device
    l0, l1 = _flat_lines(lines0), _flat_lines(lines1)
    B, n0 = l0.shape[:2]
    n1 = l1.shape[1]
    assert l1.shape[0] == B

    def zeros(shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=dev)

    out = {"num_close_pts0": zeros((B, n0, n1), torch.uint8), "num_close_pts1_t": zeros((B, n0, n1), torch.uint8),
           "out_of0": zeros((B, n1), torch.bool), "out_of1": zeros((B, n0), torch.bool),
           "ignore_depth0": zeros((B, n0), torch.bool), "ignore_depth1": zeros((B, n1), torch.bool),
           "num_visible0": zeros((B, n0), torch.uint8), "num_visible1": zeros((B, n1), torch.uint8)}
    if B == 0 or n0 == 0 or n1 == 0:
        return out
    cam0 = _rows(data["view0"]["camera"], B, dev, "camera")
    cam1 = _rows(data["view1"]["camera"], B, dev, "camera")
    if cam0.shape[1] != cam1.shape[1]:
        raise ValueError("the two cameras must have the same number of distortion terms")
    T01, T10 = _rows(data["T_0to1"], B, dev, "pose"), _rows(data["T_1to0"], B, dev, "pose")
    depth0, depth1 = _depth(data["view0"]["depth"], B, dev), _depth(data["view1"]["depth"], B, dev)
    H0, W0 = depth0.shape[1:]
    H1, W1 = depth1.shape[1:]
    # :290-291; the reference raises a KeyError without the images
    ih0, iw0 = (int(v) for v in data["view0"]["image"].shape[-2:]) if "image" in data["view0"] else (H0, W0)
    ih1, iw1 = (int(v) for v in data["view1"]["image"].shape[-2:]) if "image" in data["view1"] else (H1, W1)
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_gt_line_counts_pose_depth_workspace_bytes(B, n0, n1, npts, ctypes.byref(nb)),
               "lg_gt_line_counts_pose_depth_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(
            lib.lg_gt_line_counts_pose_depth(
                _ptr(l0), _ptr(l1), _ptr(depth0), H0, W0, _ptr(depth1), H1, W1, ih0, iw0, ih1, iw1, _ptr(cam0), _ptr(cam1),
                cam0.shape[1] - 6, _ptr(T01), _ptr(T10), B, n0, n1, npts, float(dist_th), float(min_visibility_th),
                _ptr(out["num_close_pts0"]), _ptr(out["num_close_pts1_t"]), _ptr(out["out_of0"]), _ptr(out["out_of1"]),
                _ptr(out["ignore_depth0"]), _ptr(out["ignore_depth1"]), _ptr(out["num_visible0"]),
                _ptr(out["num_visible1"]), _ptr(ws), nb.value, ctypes.c_void_p(stream)),
            "lg_gt_line_counts_pose_depth",
        )
    return out


def _empty_depth_labels(B, n0, n1, dev):
    # :227-238: an all-false `positive` and matches of -1, unlike the homography variant's [B, 0] pair
    return (torch.zeros((B, n0, n1), dtype=torch.bool, device=dev),
            torch.full((B, n0), -1, dtype=torch.int64, device=dev), torch.full((B, n1), -1, dtype=torch.int64, device=dev))


def line_labels_from_visibility_counts(cnt0, cnt1t, out_of0, out_of1, ignore_depth0, ignore_depth1, num_visible0,
                                       num_visible1, valid0, valid1, npts, overlap_th):
    """Stage B of the pose-and-depth variant (:321-400): ``mask_close`` with per-line thresholds
    (``cnt1t[i,j] > num_visible0[i] * overlap_th`` and ``cnt0[i,j] > num_visible1[j] * overlap_th``),
    ``out_of`` only in the unmatched lines, ``ignore = ignore_depth | ~valid``, then cost, assignment and
    labels as :func:`line_labels_from_counts`.  Returns ``(positive bool [B,n0,n1], m0 int64 [B,n0],
    m1 int64 [B,n1])``."""
    tensors = (cnt0, cnt1t, out_of0, out_of1, ignore_depth0, ignore_depth1, num_visible0, num_visible1, valid0, valid1)
    _need_device(*tensors)
    npts = _check_npts(npts)
    dev = cnt0.device
    B, n0, n1 = cnt0.shape
    assert cnt1t.shape == (B, n0, n1) and out_of0.shape == (B, n1) and out_of1.shape == (B, n0)
    assert ignore_depth0.shape == (B, n0) and ignore_depth1.shape == (B, n1)
    assert num_visible0.shape == (B, n0) and num_visible1.shape == (B, n1)
    assert valid0.shape == (B, n0) and valid1.shape == (B, n1)
    if B == 0 or n0 == 0 or n1 == 0:
        return _empty_depth_labels(B, n0, n1, dev)
    u8 = [t.detach().to(torch.uint8).contiguous() for t in (cnt0, cnt1t, num_visible0, num_visible1)]
    flags = [t.detach().to(torch.bool).contiguous() for t in (out_of0, out_of1, ignore_depth0, ignore_depth1, valid0, valid1)]
    positive = torch.empty((B, n0, n1), dtype=torch.bool, device=dev)
    m0 = torch.empty((B, n0), dtype=torch.int64, device=dev)
    m1 = torch.empty((B, n1), dtype=torch.int64, device=dev)
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_gt_line_labels_visibility_workspace_bytes(B, n0, n1, ctypes.byref(nb)),
               "lg_gt_line_labels_visibility_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(
            lib.lg_gt_line_labels_visibility(_ptr(u8[0]), _ptr(u8[1]), _ptr(flags[0]), _ptr(flags[1]), _ptr(flags[2]),
                                             _ptr(flags[3]), _ptr(u8[2]), _ptr(u8[3]), _ptr(flags[4]), _ptr(flags[5]), B, n0,
                                             n1, npts, float(overlap_th), _ptr(positive), _ptr(m0), _ptr(m1), _ptr(ws),
                                             nb.value, ctypes.c_void_p(stream)),
            "lg_gt_line_labels_visibility",
        )
    return positive, m0, m1


def gt_line_matches_from_pose_depth(lines0, lines1, valid_lines0, valid_lines1, data, npts=50, dist_th=5, overlap_th=0.2,
                                    min_visibility_th=0.5):
    """``gt_generation.py:207-406`` on the device: stage A, then stage B.  Lines that reproject outside the
    other image, or far from every line there, are UNMATCHED (-1); lines without enough valid depth along
    them, or invalid, are IGNORED (-2)."""
    _need_device(lines0, lines1, valid_lines0, valid_lines1)
    if lines0.shape[1] == 0 or lines1.shape[1] == 0:  # :227-238
        return _empty_depth_labels(lines0.shape[0], lines0.shape[1], lines1.shape[1], lines0.device)
    a = close_point_counts_from_pose_depth(lines0, lines1, data, npts, dist_th, min_visibility_th)
    return line_labels_from_visibility_counts(a["num_close_pts0"], a["num_close_pts1_t"], a["out_of0"], a["out_of1"],
                                              a["ignore_depth0"], a["ignore_depth1"], a["num_visible0"], a["num_visible1"],
                                              valid_lines0, valid_lines1, npts, overlap_th)


def linear_sum_assignment(cost):
    """``scipy.optimize.linear_sum_assignment`` for a device tensor ``[n0,n1]`` or a batch ``[B,n0,n1]`` of
    any real dtype (converted to fp64; entries must be finite).  Returns ``(row_ind, col_ind)`` as int64
    ``[B, min(n0,n1)]`` (``[min(n0,n1)]`` for a single matrix): SciPy's own result, not merely an optimal
    one -- the same algorithm, scan order and tie rule.  A matrix without a finite assignment (SciPy raises)
    gets -1 in every slot."""
    _need_device(cost)
    if cost.is_complex():
        raise TypeError("linear_sum_assignment: the cost must be real")
    single = cost.dim() == 2
    c = cost.detach()[None] if single else cost.detach()
    assert c.dim() == 3, f"cost must be [n0,n1] or [B,n0,n1], got {tuple(cost.shape)}"
    c = c.to(torch.float64).contiguous()
    dev = c.device
    B, nr, nc = c.shape
    k = min(nr, nc)
    row = torch.empty((B, k), dtype=torch.int64, device=dev)
    col = torch.empty((B, k), dtype=torch.int64, device=dev)
    if B and k:
        lib = _lib.load()
        nb = ctypes.c_size_t()
        _lib.check(lib.lg_linear_sum_assignment_workspace_bytes(B, nr, nc, ctypes.byref(nb)),
                   "lg_linear_sum_assignment_workspace_bytes")
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev) if nb.value else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.lg_linear_sum_assignment(_ptr(c), B, nr, nc, _ptr(row), _ptr(col), _ptr(ws), nb.value,
                                                    ctypes.c_void_p(stream)), "lg_linear_sum_assignment")
    return (row[0], col[0]) if single else (row, col)


class LineHomographyMatcher(HomographyMatcher):
    """The reference's ``matchers.homography_matcher`` with ``use_lines`` on by default
    (``homography_matcher.py:8-66``): the point dict of :class:`HomographyMatcher` (with ``use_points``) plus
    ``line_matches0``, ``line_matches1`` and ``line_assignment``."""

    default_conf = {**HomographyMatcher.default_conf, "use_lines": True}

    required_data_keys = ["H_0to1"]

    def _init(self, conf):  # :24-34
        if conf.use_points:
            self.required_data_keys += ["keypoints0", "keypoints1"]
        if conf.use_lines:
            self.required_data_keys += ["lines0", "lines1", "valid_lines0", "valid_lines1"]

    def _forward(self, data):  # :36-63
        result = {}
        if self.conf.use_points:
            result = gt_matches_from_homography(data["keypoints0"], data["keypoints1"], data["H_0to1"],
                                                pos_th=self.conf.th_positive, neg_th=self.conf.th_negative,
                                                reward=bool(self.conf.reward))
        if self.conf.use_lines:
            line_assignment, line_m0, line_m1 = gt_line_matches_from_homography(
                data["lines0"], data["lines1"], data["valid_lines0"], data["valid_lines1"],
                data["view0"]["image"].shape, data["view1"]["image"].shape, data["H_0to1"],
                self.conf.n_line_sampled_pts, self.conf.line_perp_dist_th, self.conf.overlap_th,
                self.conf.min_visibility_th)
            result["line_matches0"] = line_m0
            result["line_matches1"] = line_m1
            result["line_assignment"] = line_assignment
        return result


class LineDepthMatcher(DepthMatcher):
    """The reference's ``matchers.depth_matcher`` with ``use_lines`` on by default
    (``depth_matcher.py:10-79``): the point dict of :class:`~lightglue_amd.depth_matcher.DepthMatcher` (with
    ``use_points``) plus ``line_matches0``, ``line_matches1`` and ``line_assignment``.  ``th_consistency``
    applies to the points only, as in the reference."""

    default_conf = {**DepthMatcher.default_conf, "use_lines": True}

    required_data_keys = ["view0", "view1", "T_0to1", "T_1to0"]

    def _init(self, conf):  # :28-38
        if conf.use_points:
            self.required_data_keys += ["keypoints0", "keypoints1"]
        if conf.use_lines:
            self.required_data_keys += ["lines0", "lines1", "valid_lines0", "valid_lines1"]

    def _forward(self, data):  # :41-79
        result = DepthMatcher._forward(self, data)
        if self.conf.use_lines:
            line_assignment, line_m0, line_m1 = gt_line_matches_from_pose_depth(
                data["lines0"], data["lines1"], data["valid_lines0"], data["valid_lines1"], data,
                self.conf.n_line_sampled_pts, self.conf.line_perp_dist_th, self.conf.overlap_th,
                self.conf.min_visibility_th)
            result["line_matches0"] = line_m0
            result["line_matches1"] = line_m1
            result["line_assignment"] = line_assignment
        return result


__main_model__ = LineHomographyMatcher
