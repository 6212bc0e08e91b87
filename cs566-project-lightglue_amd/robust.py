"""Robust homography estimation on the HIP library: the reference's ``robust_estimators`` package for
homographies (``gluefactory/robust_estimators/base_estimator.py``, ``homography/opencv.py``) and its
``eval_homography_robust`` (``gluefactory/eval/utils.py:132-173``), which produces ``H_error_ransac``.

The reference hands each pair to OpenCV or PoseLib on the host.  Here ``lg_ransac_homography``
(csrc/ransac_homography.hip) runs a deterministic LO-RANSAC for every pair of a batch
in one launch, one workgroup per pair, in float64: counter-based sampling (splitmix64 of seed,
hypothesis and draw, so a pair draws the same samples alone and inside any batch), a closed-form
four-point solver, rounds of 256 hypotheses, a DLT local optimisation after every round that improved,
and the usual confidence stopping rule.  The returned mask is the classification under the returned
fp32 matrix, so the two are consistent with each other.

Differences from the reference:

* The sampler is this project's own: the numbers agree with OpenCV's RANSAC in distribution, not pair
  by pair (no two RANSAC implementations do), so AUC values computed from them are close to, not equal
  to, the ones in BASELINE.md.
* ``options`` has ``seed`` and ``min_area`` (px^2; samples with a nearly collinear triple are rejected)
  and no ``method``.
* Batched inputs ``[B, K, 2]`` are accepted, with an optional ``num_matches`` ``[B]``; they return
  device tensors without a host sync.  ``conf["ransac_th"]`` may be a number or a ``[B]`` tensor.
* ``eval_homography_robust`` on a batch estimates a homography per pair (the reference's batched branch
  dispatches to the relative-pose evaluator, which cannot have been meant); it reads
  ``num_keypoints0/1`` for ragged batches, as ``match_eval`` does, and also returns ``M_0to1`` and
  ``inliers`` (in ``keypoints0`` slot order).
* ``PointLineHomographyEstimator`` (``load_estimator("homography", "homography_est")``; the reference wraps
  the external ``homography_est`` library) is ``lg_ransac_homography_lines`` (csrc/ransac_homography_lines.hip,
  DESIGN.md §10p): the same sampler, rounds, local optimisation and stopping rule over point and line
  matches together, a general 8x9 minimal solver in one fixed normalising frame per image, a line an
  inlier when both mapped endpoints lie within the threshold of the matched segment's line.  Its ``options``
  have ``seed`` and ``min_line_length`` (px; shorter segments are not used).  With no lines it is still that
  general solver, not the closed form above: the two agree in what they find, not bit for bit.
* Inputs that are not on the device raise; there is no CPU path.
* ``load_estimator("relative_pose", ...)`` raises here: this module is the homography side.  Robust
  relative pose lives in :mod:`lightglue_amd.relative_pose`, whose ``load_estimator``
  resolves both types.
"""
import ctypes

import torch

from . import _lib
from ._native import _ptr
from .lightglue import LightGlue, merge_conf

INFO_FIELDS = ("success", "num_matches", "num_inliers", "best_t", "best_minimal_count", "rounds", "valid_hypotheses")
LINES_INFO_FIELDS = ("success", "num_point_matches", "num_line_matches", "num_point_inliers", "num_line_inliers", "best_t",
                     "best_minimal_count", "rounds", "valid_hypotheses")
_PRED_KEYS = ("keypoints0", "keypoints1", "matches0", "matching_scores0")
_NO_CPU = "lightglue_amd: inputs must be on a HIP (cuda) device; there is no CPU path"


def __getattr__(name):
    # LDS_MATCHES: matches of a pair the kernel keeps in LDS (csrc/kernels.h: RH_LDS_MATCHES), asked of
    # the library on first use; pairs with more run the same arithmetic from global memory
    if name == "LDS_MATCHES":
        globals()[name] = int(_lib.load().lg_ransac_lds_matches())
        return globals()[name]
    # LDS_POINTS, LDS_LINES: the same for the point-and-line kernel (csrc/kernels.h: RL_LDS_POINTS, RL_LDS_LINES)
    if name in ("LDS_POINTS", "LDS_LINES"):
        p, n = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().lg_ransac_lines_lds_capacity(ctypes.byref(p), ctypes.byref(n)), "lg_ransac_lines_lds_capacity")
        globals()["LDS_POINTS"], globals()["LDS_LINES"] = int(p.value), int(n.value)
        return globals()[name]
    raise AttributeError(name)


def _need(d, keys, what):
    for k in keys:
        if k not in d:
            raise KeyError(f"robust: {what} has no '{k}'")


def ransac_homography(kpts0, kpts1, matches0=None, ransac_th=3.0, num0=None, num1=None, max_iters=3000,
                      confidence=0.995, seed=0, min_area=1.0, H_gt=None, image_size0=None):
    """One launch of ``lg_ransac_homography``.  kpts0 [B,M,2], kpts1 [B,N,2]; matches0 [B,M] int64, or
    None: M == N and slot i matches slot i.  Returns device tensors: ``H`` [B,3,3], ``inliers`` [B,M]
    bool, ``info`` [B,8] int32 (``INFO_FIELDS``), ``m_kpts`` [B,M,4] (rows below ``num_matches`` are
    the matched points, the rest is unspecified) and, with ``H_gt`` and ``image_size0``, ``H_error``."""
    if not torch.is_tensor(kpts0) or not torch.is_tensor(kpts1):
        raise TypeError("robust: keypoints must be tensors")
    dev = kpts0.device
    if dev.type != "cuda" or kpts1.device != dev or (matches0 is not None and matches0.device != dev):
        raise RuntimeError(_NO_CPU)
    if kpts0.dim() != 3 or kpts1.dim() != 3 or kpts0.shape[-1] != 2 or kpts1.shape[-1] != 2 or \
            kpts0.shape[0] != kpts1.shape[0]:
        raise ValueError(f"robust: keypoints: expected [B, M, 2] and [B, N, 2], got {list(kpts0.shape)} and "
                         f"{list(kpts1.shape)}")
    B, M = kpts0.shape[:2]
    N = kpts1.shape[1]
    if matches0 is None:
        if M != N:
            raise ValueError(f"robust: matched points need the same number on both sides, got {M} and {N}")
    elif tuple(matches0.shape) != (B, M):
        raise ValueError(f"robust: matches0: expected [{B}, {M}], got {list(matches0.shape)}")
    if (H_gt is None) != (image_size0 is None):
        raise ValueError("robust: H_gt and image_size0 go together")
    if int(max_iters) < 1 or not 0.0 < float(confidence) < 1.0 or not float(min_area) >= 0.0:
        raise ValueError(f"robust: max_iters >= 1, 0 < confidence < 1 and min_area >= 0 are required, got {max_iters}, "
                         f"{confidence}, {min_area}")
    num0, num1 = LightGlue._check_counts(num0, num1, B)
    kpts0 = kpts0.detach().to(torch.float32).contiguous()
    kpts1 = kpts1.detach().to(torch.float32).contiguous()
    if matches0 is not None:
        matches0 = matches0.detach().to(torch.int64).contiguous()
    if num0 is not None:
        num0 = num0.to(device=dev, dtype=torch.int32).contiguous()
        num1 = num1.to(device=dev, dtype=torch.int32).contiguous()
    if torch.is_tensor(ransac_th):
        if tuple(ransac_th.shape) not in ((), (B,)):
            raise ValueError(f"robust: ransac_th: expected a number or [{B}], got {list(ransac_th.shape)}")
        th = ransac_th.detach().to(device=dev, dtype=torch.float32).expand(B).contiguous()
    else:
        th = torch.full((B,), float(ransac_th), dtype=torch.float32, device=dev)
    if H_gt is not None:
        for name, t, shape in (("H_gt", H_gt, (B, 3, 3)), ("image_size0", image_size0, (B, 2))):
            if tuple(t.shape) != shape:
                raise ValueError(f"robust: {name}: expected {list(shape)}, got {list(t.shape)}")
            if t.device != dev:
                raise RuntimeError(f"robust: {name} is on {t.device}, the keypoints are on {dev}")
        H_gt = H_gt.detach().to(torch.float32).contiguous()
        image_size0 = image_size0.detach().to(torch.float32).contiguous()

    H = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    inl = torch.empty((B, M), dtype=torch.uint8, device=dev)
    info = torch.empty((B, 8), dtype=torch.int32, device=dev)
    m_kpts = torch.empty((B, M, 4), dtype=torch.float32, device=dev)
    err = torch.empty((B,), dtype=torch.float32, device=dev) if H_gt is not None else None
    if B == 0 or M == 0:  # nothing is launched: the empty set's values
        H.copy_(torch.eye(3, device=dev).expand(B, 3, 3))
        info.zero_()
        info[:, 3] = -1
        if err is not None:
            err.fill_(float("inf"))
    else:
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(
                lib.lg_ransac_homography(_ptr(kpts0), _ptr(kpts1), _ptr(matches0), B, M, N, _ptr(num0), _ptr(num1),
                                         _ptr(th), int(max_iters), float(confidence), int(seed) & (2**64 - 1),
                                         float(min_area), _ptr(H_gt), _ptr(image_size0), _ptr(H), _ptr(inl), _ptr(info),
                                         _ptr(m_kpts), _ptr(err), ctypes.c_void_p(stream)),
                "lg_ransac_homography",
            )
    out = {"H": H, "inliers": inl.bool(), "info": info, "m_kpts": m_kpts}
    if err is not None:
        out["H_error"] = err
    return out


class HomographyEstimator:
    """The reference's ``BaseEstimator`` contract (``__call__(data) -> dict``) on the device."""
    default_conf = {
        "ransac_th": 3.0,
        "options": {"max_iters": 3000, "confidence": 0.995, "seed": 0, "min_area": 1.0},
    }
    required_data_keys = ["m_kpts0", "m_kpts1"]

    def __init__(self, conf=None):
        self.conf = merge_conf({"name": "hip"}, self.default_conf, conf or {})
        unknown = set(self.conf.options) - set(self.default_conf["options"])
        if unknown:
            raise ValueError(f"robust: unknown options {sorted(unknown)}; known: {sorted(self.default_conf['options'])}")
        self.required_data_keys = list(self.required_data_keys)

    def __call__(self, data):
        return self._forward(data)

    def _forward(self, data):
        _need(data, self.required_data_keys, "data")
        p0, p1 = data["m_kpts0"], data["m_kpts1"]
        if not torch.is_tensor(p0) or not torch.is_tensor(p1):
            raise TypeError("robust: m_kpts0 and m_kpts1 must be tensors")
        if p0.shape != p1.shape or p0.dim() not in (2, 3) or p0.shape[-1] != 2:
            raise ValueError(f"robust: m_kpts0 and m_kpts1: expected two [K, 2] or [B, K, 2] tensors, got "
                             f"{list(p0.shape)} and {list(p1.shape)}")
        single = p0.dim() == 2
        nm = data.get("num_matches")
        if single:
            if nm is not None:
                raise ValueError("robust: num_matches belongs to the batched form")
            p0, p1 = p0[None], p1[None]
        o = self.conf.options
        r = ransac_homography(p0, p1, None, self.conf.ransac_th, nm, nm, o.max_iters, o.confidence, o.seed, o.min_area)
        success = r["info"][:, 0] > 0
        if single:  # as the reference: a Python bool through one sync
            return {"success": bool(success[0]), "M_0to1": r["H"][0].to(data["m_kpts0"].dtype), "inliers": r["inliers"][0]}
        return {"success": success, "M_0to1": r["H"], "inliers": r["inliers"], "info": r["info"]}


def ransac_homography_lines(kpts0, kpts1, matches0=None, lines0=None, lines1=None, line_matches0=None, ransac_th=2.0,
                            num0=None, num1=None, num_lines0=None, num_lines1=None, max_iters=3000, confidence=0.995,
                            seed=0, min_line_length=1.0, H_gt=None, image_size0=None):
    """One launch of ``lg_ransac_homography_lines``.  kpts0 [B,M,2], kpts1 [B,N,2] and
    matches0 as for :func:`ransac_homography`; lines0 [B,L0,2,2], lines1 [B,L1,2,2] (endpoints x, y);
    line_matches0 [B,L0] int64, or None: L0 == L1 and slot i matches slot i.  Either set may be empty
    (M == 0 or L0 == 0).  Returns device tensors: ``H`` [B,3,3], ``inliers`` [B,M] and ``line_inliers``
    [B,L0] bool, ``info`` [B,12] int32 (``LINES_INFO_FIELDS``), ``m_kpts`` [B,M,4] and ``m_lines``
    [B,L0,8] (rows below the match counts are the live features, the rest is unspecified) and, with
    ``H_gt`` and ``image_size0``, ``H_error``."""
    for name, t in (("keypoints", kpts0), ("keypoints", kpts1), ("lines", lines0), ("lines", lines1)):
        if not torch.is_tensor(t):
            raise TypeError(f"robust: {name} must be tensors")
    dev = kpts0.device
    if dev.type != "cuda" or any(t is not None and t.device != dev for t in (kpts1, matches0, lines0, lines1, line_matches0)):
        raise RuntimeError(_NO_CPU)
    if kpts0.dim() != 3 or kpts1.dim() != 3 or kpts0.shape[-1] != 2 or kpts1.shape[-1] != 2 or \
            kpts0.shape[0] != kpts1.shape[0]:
        raise ValueError(f"robust: keypoints: expected [B, M, 2] and [B, N, 2], got {list(kpts0.shape)} and "
                         f"{list(kpts1.shape)}")
    B, M = kpts0.shape[:2]
    N = kpts1.shape[1]
    if lines0.dim() != 4 or lines1.dim() != 4 or tuple(lines0.shape[2:]) != (2, 2) or tuple(lines1.shape[2:]) != (2, 2) or \
            lines0.shape[0] != B or lines1.shape[0] != B:
        raise ValueError(f"robust: lines: expected [{B}, L0, 2, 2] and [{B}, L1, 2, 2], got {list(lines0.shape)} and "
                         f"{list(lines1.shape)}")
    L0, L1 = lines0.shape[1], lines1.shape[1]
    if matches0 is None:
        if M != N:
            raise ValueError(f"robust: matched points need the same number on both sides, got {M} and {N}")
    elif tuple(matches0.shape) != (B, M):
        raise ValueError(f"robust: matches0: expected [{B}, {M}], got {list(matches0.shape)}")
    if line_matches0 is None:
        if L0 != L1:
            raise ValueError(f"robust: matched lines need the same number on both sides, got {L0} and {L1}")
    elif tuple(line_matches0.shape) != (B, L0):
        raise ValueError(f"robust: line_matches0: expected [{B}, {L0}], got {list(line_matches0.shape)}")
    if (H_gt is None) != (image_size0 is None):
        raise ValueError("robust: H_gt and image_size0 go together")
    if int(max_iters) < 1 or not 0.0 < float(confidence) < 1.0 or not 0.0 <= float(min_line_length) < float("inf"):
        raise ValueError(f"robust: max_iters >= 1, 0 < confidence < 1 and a finite min_line_length >= 0 are required, got "
                         f"{max_iters}, {confidence}, {min_line_length}")
    num0, num1 = LightGlue._check_counts(num0, num1, B)
    num_lines0, num_lines1 = LightGlue._check_counts(num_lines0, num_lines1, B)
    f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    i32 = lambda t: None if t is None else t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
    i64 = lambda t: None if t is None else t.detach().to(torch.int64).contiguous()  # noqa: E731
    kpts0, kpts1, lines0, lines1 = f32(kpts0), f32(kpts1), f32(lines0), f32(lines1)
    matches0, line_matches0 = i64(matches0), i64(line_matches0)
    num0, num1, num_lines0, num_lines1 = i32(num0), i32(num1), i32(num_lines0), i32(num_lines1)
    if torch.is_tensor(ransac_th):
        if tuple(ransac_th.shape) not in ((), (B,)):
            raise ValueError(f"robust: ransac_th: expected a number or [{B}], got {list(ransac_th.shape)}")
        th = ransac_th.detach().to(device=dev, dtype=torch.float32).expand(B).contiguous()
    else:
        th = torch.full((B,), float(ransac_th), dtype=torch.float32, device=dev)
    if H_gt is not None:
        for name, t, shape in (("H_gt", H_gt, (B, 3, 3)), ("image_size0", image_size0, (B, 2))):
            if tuple(t.shape) != shape:
                raise ValueError(f"robust: {name}: expected {list(shape)}, got {list(t.shape)}")
            if t.device != dev:
                raise RuntimeError(f"robust: {name} is on {t.device}, the keypoints are on {dev}")
        H_gt, image_size0 = f32(H_gt), f32(image_size0)

    H = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    inl = torch.empty((B, M), dtype=torch.uint8, device=dev)
    linl = torch.empty((B, L0), dtype=torch.uint8, device=dev)
    info = torch.empty((B, 12), dtype=torch.int32, device=dev)
    m_kpts = torch.empty((B, M, 4), dtype=torch.float32, device=dev)
    m_lines = torch.empty((B, L0, 8), dtype=torch.float32, device=dev)
    err = torch.empty((B,), dtype=torch.float32, device=dev) if H_gt is not None else None
    if B == 0 or (M == 0 and L0 == 0):  # nothing is launched: the empty set's values
        H.copy_(torch.eye(3, device=dev).expand(B, 3, 3))
        info.zero_()
        info[:, 5] = -1
        if err is not None:
            err.fill_(float("inf"))
    else:
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(
                lib.lg_ransac_homography_lines(
                    _ptr(kpts0), _ptr(kpts1), _ptr(matches0), B, M, N, _ptr(num0), _ptr(num1), _ptr(lines0), _ptr(lines1),
                    _ptr(line_matches0), L0, L1, _ptr(num_lines0), _ptr(num_lines1), _ptr(th), int(max_iters),
                    float(confidence), int(seed) & (2**64 - 1), float(min_line_length), _ptr(H_gt), _ptr(image_size0),
                    _ptr(H), _ptr(inl), _ptr(linl), _ptr(info), _ptr(m_kpts), _ptr(m_lines), _ptr(err),
                    ctypes.c_void_p(stream)),
                "lg_ransac_homography_lines",
            )
    out = {"H": H, "inliers": inl.bool(), "line_inliers": linl.bool(), "info": info, "m_kpts": m_kpts, "m_lines": m_lines}
    if err is not None:
        out["H_error"] = err
    return out


class PointLineHomographyEstimator:
    """The reference's ``PointLineHomographyEstimator`` (``robust_estimators/homography/homography_est.py``)
    on the device: ``m_kpts0/1`` and ``m_lines0/1``, either pair of which may be missing."""
    default_conf = {
        "ransac_th": 2.0,
        "options": {"max_iters": 3000, "confidence": 0.995, "seed": 0, "min_line_length": 1.0},
    }
    required_data_keys = []

    def __init__(self, conf=None):
        self.conf = merge_conf({"name": "homography_est"}, self.default_conf, conf or {})
        unknown = set(self.conf.options) - set(self.default_conf["options"])
        if unknown:
            raise ValueError(f"robust: unknown options {sorted(unknown)}; known: {sorted(self.default_conf['options'])}")
        self.required_data_keys = list(self.required_data_keys)

    def __call__(self, data):
        return self._forward(data)

    def _forward(self, data):
        have_p, have_l = "m_kpts0" in data or "m_kpts1" in data, "m_lines0" in data or "m_lines1" in data
        if not have_p and not have_l:
            raise KeyError("robust: data has neither 'm_kpts0' / 'm_kpts1' nor 'm_lines0' / 'm_lines1'")
        if have_p:
            _need(data, ["m_kpts0", "m_kpts1"], "data")
        if have_l:
            _need(data, ["m_lines0", "m_lines1"], "data")
        p0, p1, l0, l1 = data.get("m_kpts0"), data.get("m_kpts1"), data.get("m_lines0"), data.get("m_lines1")
        if any(t is not None and not torch.is_tensor(t) for t in (p0, p1, l0, l1)):
            raise TypeError("robust: m_kpts0/1 and m_lines0/1 must be tensors")
        if have_p and (p0.shape != p1.shape or p0.dim() not in (2, 3) or p0.shape[-1] != 2):
            raise ValueError(f"robust: m_kpts0 and m_kpts1: expected two [K, 2] or [B, K, 2] tensors, got "
                             f"{list(p0.shape)} and {list(p1.shape)}")
        if have_l and (l0.shape != l1.shape or l0.dim() not in (3, 4) or tuple(l0.shape[-2:]) != (2, 2)):
            raise ValueError(f"robust: m_lines0 and m_lines1: expected two [K, 2, 2] or [B, K, 2, 2] tensors, got "
                             f"{list(l0.shape)} and {list(l1.shape)}")
        single = p0.dim() == 2 if have_p else l0.dim() == 3
        if have_p and have_l and (l0.dim() == 3) != single:
            raise ValueError("robust: m_kpts0/1 and m_lines0/1 must both be batched or both be single")
        nm, nlm = data.get("num_matches"), data.get("num_line_matches")
        if single:
            if nm is not None or nlm is not None:
                raise ValueError("robust: num_matches and num_line_matches belong to the batched form")
            p0, p1, l0, l1 = (None if t is None else t[None] for t in (p0, p1, l0, l1))
        ref_t = p0 if have_p else l0
        if not have_p:
            p0 = p1 = ref_t.new_zeros((ref_t.shape[0], 0, 2))
        if not have_l:
            l0 = l1 = ref_t.new_zeros((ref_t.shape[0], 0, 2, 2))
        o = self.conf.options
        r = ransac_homography_lines(p0, p1, None, l0, l1, None, self.conf.ransac_th, nm, nm, nlm, nlm, o.max_iters,
                                    o.confidence, o.seed, o.min_line_length)
        success = r["info"][:, 0] > 0
        if single:  # as the reference: a Python bool through one sync
            return {"success": bool(success[0]), "M_0to1": r["H"][0].to(ref_t.dtype), "inliers": r["inliers"][0],
                    "line_inliers": r["line_inliers"][0]}
        return {"success": success, "M_0to1": r["H"], "inliers": r["inliers"], "line_inliers": r["line_inliers"],
                "info": r["info"]}


def load_estimator(type, estimator):
    """``robust_estimators/__init__.py``: the estimator class of a type and a name."""
    if type == "relative_pose":
        raise NotImplementedError("robust: relative pose estimation is out of scope (DESIGN.md §11)")
    if type != "homography":
        raise ValueError(f"robust: unknown estimator type '{type}'")
    if estimator == "homography_est":
        return PointLineHomographyEstimator
    if estimator != "hip":
        raise ValueError(f"robust: unknown homography estimator '{estimator}'; this project has 'hip' and "
                         f"'homography_est'")
    return HomographyEstimator


def _eval_point_line(est, data, pred):
    """The ``homography_est`` branch of :func:`eval_homography_robust` (``eval/utils.py:146-157``)."""
    _need(data, ["H_0to1", "view0"], "data")
    _need(data["view0"], ["image_size"], "data['view0']")
    have_l = "lines0" in pred
    have_p = not have_l or any(k in pred for k in _PRED_KEYS[:3])
    H_gt, size0 = data["H_0to1"], torch.as_tensor(data["view0"]["image_size"])
    named = [("H_0to1", H_gt)]
    if have_p:
        _need(pred, _PRED_KEYS, "pred")
        named += [(k, pred[k]) for k in _PRED_KEYS[:3]]
    if have_l:
        _need(pred, ["lines1", "line_matches0"], "pred")
        if "orig_lines0" in pred:  # the segments in the original image's pixels take precedence
            _need(pred, ["orig_lines1"], "pred")
            named += [("lines0", pred["orig_lines0"]), ("lines1", pred["orig_lines1"])]
        else:
            named += [("lines0", pred["lines0"]), ("lines1", pred["lines1"])]
        named.append(("line_matches0", pred["line_matches0"]))
    for name, t in named:
        if not torch.is_tensor(t):
            raise TypeError(f"robust: {name} must be a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
    t = dict(named)
    single = H_gt.dim() == 2
    counts = [pred.get(k, data.get(k)) for k in ("num_keypoints0", "num_keypoints1", "num_lines0", "num_lines1")]
    if single:
        t = {k: v[None] for k, v in t.items()}
        size0 = size0[None]
        counts = [None if c is None else torch.as_tensor(c).reshape(1) for c in counts]
    B, dev = t["H_0to1"].shape[0], H_gt.device
    kp0, kp1, m0 = (t[k] for k in _PRED_KEYS[:3]) if have_p else (H_gt.new_zeros((B, 0, 2)),) * 2 + (None,)
    l0, l1, lm0 = (t[k] for k in ("lines0", "lines1", "line_matches0")) if have_l else (H_gt.new_zeros((B, 0, 2, 2)),) * 2 + (None,)
    nk0, nk1 = counts[:2] if have_p and None not in counts[:2] else (None, None)
    nl0, nl1 = counts[2:] if have_l and None not in counts[2:] else (None, None)
    o = est.conf.options
    r = ransac_homography_lines(kp0, kp1, m0, l0, l1, lm0, est.conf.ransac_th, nk0, nk1, nl0, nl1, o.max_iters, o.confidence,
                                o.seed, o.min_line_length, H_gt=t["H_0to1"], image_size0=size0.to(dev))
    info = r["info"]
    inl, linl = (info[:, 3] + info[:, 4]).to(torch.float32), info[:, 4].to(torch.float32)
    out = {"H_error_ransac": r["H_error"], "ransac_inl": inl,
           "ransac_inl%": inl / (info[:, 1] + info[:, 2]).clamp(min=1).to(torch.float32), "ransac_line_inl": linl,
           "M_0to1": r["H"], "inliers": r["inliers"], "line_inliers": r["line_inliers"]}
    if single:
        keys = ("H_error_ransac", "ransac_inl", "ransac_inl%", "ransac_line_inl")
        vals = torch.stack([out[k][0].to(torch.float64) for k in keys]).tolist()
        out = {**dict(zip(keys, vals)), "M_0to1": r["H"][0], "inliers": r["inliers"][0], "line_inliers": r["line_inliers"][0]}
    return out


def eval_homography_robust(data, pred, conf=None):
    """``eval/utils.py:132-173`` for points: H_error_ransac, ransac_inl, ransac_inl%, and M_0to1 and
    inliers.  ``conf``: ``ransac_th``, ``options`` and ``estimator``: ``"hip"`` (points, §10k) or
    ``"homography_est"`` (points and lines, §10p).  With the latter and ``lines0`` in ``pred`` the lines
    enter as in the reference (``orig_lines0/1`` before ``lines0/1``, then ``line_matches0``; ``num_lines0/1``
    if present; the point keys may be missing), ``ransac_inl`` and ``ransac_inl%`` count both kinds of
    feature, and ``ransac_line_inl`` and ``line_inliers`` are returned as well.

    A batch ``[B, ...]`` gives ``[B]`` device tensors without a host sync, one homography per pair; an
    unbatched pair gives Python numbers through one sync.  (The reference's batched branch calls the
    relative-pose evaluator per item, a slip: the intended per-pair homography evaluation is done here.)"""
    conf = dict(conf or {})
    est = load_estimator("homography", conf.pop("estimator", "hip"))(conf)
    if isinstance(est, PointLineHomographyEstimator):
        return _eval_point_line(est, data, pred)
    _need(pred, _PRED_KEYS, "pred")
    _need(data, ["H_0to1", "view0"], "data")
    _need(data["view0"], ["image_size"], "data['view0']")
    kp0, kp1, m0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"]
    H_gt, size0 = data["H_0to1"], torch.as_tensor(data["view0"]["image_size"])
    for name, t in (("keypoints0", kp0), ("keypoints1", kp1), ("matches0", m0), ("H_0to1", H_gt)):
        if not torch.is_tensor(t):
            raise TypeError(f"robust: {name} must be a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
    single = kp0.dim() == 2
    nk0 = pred.get("num_keypoints0", data.get("num_keypoints0"))
    nk1 = pred.get("num_keypoints1", data.get("num_keypoints1"))
    if single:
        kp0, kp1, m0, H_gt, size0 = kp0[None], kp1[None], m0[None], H_gt[None], size0[None]
        if nk0 is not None and nk1 is not None:
            nk0, nk1 = torch.as_tensor(nk0).reshape(1), torch.as_tensor(nk1).reshape(1)
    o = est.conf.options
    r = ransac_homography(kp0, kp1, m0, est.conf.ransac_th, nk0, nk1, o.max_iters, o.confidence, o.seed, o.min_area,
                          H_gt=H_gt, image_size0=size0.to(kp0.device))
    info = r["info"]
    inl = info[:, 2].to(torch.float32)
    out = {"H_error_ransac": r["H_error"], "ransac_inl": inl,
           "ransac_inl%": inl / info[:, 1].clamp(min=1).to(torch.float32), "M_0to1": r["H"], "inliers": r["inliers"]}
    if single:
        keys = ("H_error_ransac", "ransac_inl", "ransac_inl%")
        vals = torch.stack([out[k][0].to(torch.float64) for k in keys]).tolist()
        out = {**dict(zip(keys, vals)), "M_0to1": r["H"][0], "inliers": r["inliers"][0]}
    return out


def as_export_callback(conf=None):
    """A ``callback_fn`` for :func:`export.export_predictions`: adds the per-pair robust results to ``pred``."""
    def callback(pred, data):
        return eval_homography_robust(data, pred, conf)

    return callback
