"""Robust relative pose on the HIP library: the reference's ``robust_estimators`` package for relative
poses (``gluefactory/robust_estimators/relative_pose/``) and its ``eval_relative_pose_robust``
(``gluefactory/eval/utils.py:94-129``), which produces ``rel_pose_error``, the quantity behind the
MegaDepth-1500 pose AUC.

The reference hands each pair to OpenCV, PoseLib or pycolmap on the host.  Here ``lg_ransac_relpose``
(csrc/ransac_relpose.hip) runs a deterministic five-point LO-RANSAC for every pair of a
batch in one launch, one workgroup per pair, in float64: :mod:`robust`'s counter-based sampler with five
matches, Nistér's five-point solver (which, unlike the seven- and eight-point ones, is not degenerate on
planes), rounds of 256 samples whose every candidate is scored, a linear eight-point local optimisation
projected onto the essential manifold, the confidence stopping rule, and the cheirality vote among the
four decompositions.  The returned mask is the classification under the returned fp32 pose ("Sampson
inlier and in front of both cameras"), so the two are consistent with each other.

Differences from the reference:

* The sampler is this project's own: pose errors agree with OpenCV's in distribution, not pair by pair.
* The threshold is OpenCV's convention for every pair: ``ransac_th`` in pixels over the mean of the four
  focal lengths.  Distortion is ignored, as ``Camera.image2cam`` does.
* ``options`` has ``max_iters``, ``confidence`` and ``seed`` and no ``method``; pycolmap's
  bundle-adjusted variant is out of scope.
* Batched inputs ``[B, K, 2]`` are accepted, with an optional ``num_matches`` ``[B]``; they return
  device tensors without a host sync.  ``conf["ransac_th"]`` may be a number or a ``[B]`` tensor.
* ``eval_relative_pose_robust`` accepts a batch, reads ``num_keypoints0/1`` for ragged batches and also
  returns ``M_0to1`` and ``inliers`` (in ``keypoints0`` slot order).
* Inputs that are not on the device raise; there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from .depth_matcher import Pose, _rows
from .lightglue import LightGlue, merge_conf
from .robust import _NO_CPU, _PRED_KEYS, HomographyEstimator, PointLineHomographyEstimator, _need, _ptr

INFO_FIELDS = ("success", "num_matches", "num_inliers", "best_t", "best_minimal_count", "rounds", "valid_samples",
               "candidates_scored")


def _cameras(cam, B, dev):
    """Camera rows (w, h, fx, fy, cx, cy, ...) in any accepted form -> [B, 4] fx, fy, cx, cy."""
    return _rows(cam, B, dev, "camera")[:, 2:6].contiguous()


def ransac_relpose(kpts0, kpts1, matches0=None, camera0=None, camera1=None, ransac_th=1.0, num0=None, num1=None,
                   max_iters=2000, confidence=0.9999, seed=0, T_gt=None):
    """One launch of ``lg_ransac_relpose``.  kpts0 [B,M,2], kpts1 [B,N,2]; matches0 [B,M] int64, or
    None: M == N and slot i matches slot i; camera0 / camera1: the reference's ``Camera``, this
    project's holder or ``[B, 6|8|10]`` rows; T_gt: a ``Pose``, ``[B, 12]`` or ``[B, 4, 4]``.  Returns
    device tensors: ``R`` [B,3,3], ``t`` [B,3], ``inliers`` [B,M] bool, ``info`` [B,8] int32
    (``INFO_FIELDS``), ``m_kpts`` [B,M,4] (rows below ``num_matches`` are the matched points, the rest is
    unspecified) and, with ``T_gt``, ``t_err``, ``r_err`` and ``rel_pose_error`` [B] in degrees."""
    if not torch.is_tensor(kpts0) or not torch.is_tensor(kpts1):
        raise TypeError("relative_pose: keypoints must be tensors")
    if camera0 is None or camera1 is None:
        raise ValueError("relative_pose: camera0 and camera1 are required")
    dev = kpts0.device
    if dev.type != "cuda" or kpts1.device != dev or (matches0 is not None and matches0.device != dev):
        raise RuntimeError(_NO_CPU)
    if kpts0.dim() != 3 or kpts1.dim() != 3 or kpts0.shape[-1] != 2 or kpts1.shape[-1] != 2 or \
            kpts0.shape[0] != kpts1.shape[0]:
        raise ValueError(f"relative_pose: keypoints: expected [B, M, 2] and [B, N, 2], got {list(kpts0.shape)} and "
                         f"{list(kpts1.shape)}")
    B, M = kpts0.shape[:2]
    N = kpts1.shape[1]
    if matches0 is None:
        if M != N:
            raise ValueError(f"relative_pose: matched points need the same number on both sides, got {M} and {N}")
    elif tuple(matches0.shape) != (B, M):
        raise ValueError(f"relative_pose: matches0: expected [{B}, {M}], got {list(matches0.shape)}")
    if int(max_iters) < 1 or not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"relative_pose: max_iters >= 1 and 0 < confidence < 1 are required, got {max_iters}, "
                         f"{confidence}")
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
            raise ValueError(f"relative_pose: ransac_th: expected a number or [{B}], got {list(ransac_th.shape)}")
        th = ransac_th.detach().to(device=dev, dtype=torch.float32).expand(B).contiguous()
    else:
        th = torch.full((B,), float(ransac_th), dtype=torch.float32, device=dev)
    cam0, cam1 = _cameras(camera0, B, dev), _cameras(camera1, B, dev)
    T = _rows(T_gt, B, dev, "pose") if T_gt is not None else None

    R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((B, 3), dtype=torch.float32, device=dev)
    inl = torch.empty((B, M), dtype=torch.uint8, device=dev)
    info = torch.empty((B, 8), dtype=torch.int32, device=dev)
    m_kpts = torch.empty((B, M, 4), dtype=torch.float32, device=dev)
    err = torch.empty((B, 3), dtype=torch.float32, device=dev) if T is not None else None
    if B == 0 or M == 0:  # nothing is launched: the empty set's values
        R.copy_(torch.eye(3, device=dev).expand(B, 3, 3))
        t.zero_()
        info.zero_()
        info[:, 3] = -1
        if err is not None:
            err.fill_(float("inf"))
    else:
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(
                lib.lg_ransac_relpose(_ptr(kpts0), _ptr(kpts1), _ptr(matches0), B, M, N, _ptr(num0), _ptr(num1),
                                      _ptr(cam0), _ptr(cam1), _ptr(th), int(max_iters), float(confidence),
                                      int(seed) & (2**64 - 1), _ptr(T), _ptr(R), _ptr(t), _ptr(inl), _ptr(info),
                                      _ptr(m_kpts), _ptr(err), ctypes.c_void_p(stream)),
                "lg_ransac_relpose",
            )
    out = {"R": R, "t": t, "inliers": inl.bool(), "info": info, "m_kpts": m_kpts}
    if err is not None:
        out["t_err"], out["r_err"], out["rel_pose_error"] = err[:, 0], err[:, 1], err[:, 2]
    return out


class RelativePoseEstimator:
    """The reference's ``BaseEstimator`` contract (``__call__(data) -> dict``) on the device."""
    default_conf = {
        "ransac_th": 1.0,
        "options": {"max_iters": 2000, "confidence": 0.9999, "seed": 0},
    }
    required_data_keys = ["m_kpts0", "m_kpts1", "camera0", "camera1"]

    def __init__(self, conf=None):
        self.conf = merge_conf({"name": "hip"}, self.default_conf, conf or {})
        unknown = set(self.conf.options) - set(self.default_conf["options"])
        if unknown:
            raise ValueError(f"relative_pose: unknown options {sorted(unknown)}; known: "
                             f"{sorted(self.default_conf['options'])}")
        self.required_data_keys = list(self.required_data_keys)

    def __call__(self, data):
        return self._forward(data)

    def _forward(self, data):
        _need(data, self.required_data_keys, "data")
        p0, p1 = data["m_kpts0"], data["m_kpts1"]
        if not torch.is_tensor(p0) or not torch.is_tensor(p1):
            raise TypeError("relative_pose: m_kpts0 and m_kpts1 must be tensors")
        if p0.shape != p1.shape or p0.dim() not in (2, 3) or p0.shape[-1] != 2:
            raise ValueError(f"relative_pose: m_kpts0 and m_kpts1: expected two [K, 2] or [B, K, 2] tensors, got "
                             f"{list(p0.shape)} and {list(p1.shape)}")
        single = p0.dim() == 2
        nm = data.get("num_matches")
        if single:
            if nm is not None:
                raise ValueError("relative_pose: num_matches belongs to the batched form")
            p0, p1 = p0[None], p1[None]
        o = self.conf.options
        r = ransac_relpose(p0, p1, None, data["camera0"], data["camera1"], self.conf.ransac_th, nm, nm, o.max_iters,
                           o.confidence, o.seed)
        success = r["info"][:, 0] > 0
        M = Pose.from_Rt(r["R"], r["t"])
        if single:  # as the reference: a Python bool through one sync
            return {"success": bool(success[0]), "M_0to1": M[0], "inliers": r["inliers"][0]}
        return {"success": success, "M_0to1": M, "inliers": r["inliers"], "info": r["info"]}


def load_estimator(type, estimator):
    """``robust_estimators/__init__.py`` for both types this project has: ``"hip"`` for either, and
    ``"homography_est"`` for the point-and-line homography estimator.  (``robust.load_estimator`` is the
    homography-only one that the package exports.)"""
    if type not in ("relative_pose", "homography"):
        raise ValueError(f"relative_pose: unknown estimator type '{type}'")
    if type == "homography" and estimator == "homography_est":
        return PointLineHomographyEstimator
    if estimator != "hip":
        raise ValueError(f"relative_pose: unknown {type} estimator '{estimator}'; this project has 'hip'")
    return RelativePoseEstimator if type == "relative_pose" else HomographyEstimator


def eval_relative_pose_robust(data, pred, conf=None):
    """``eval/utils.py:94-129``: rel_pose_error, ransac_inl, ransac_inl% (the mask's mean over the pair's
    matches), and M_0to1 and inliers.  ``conf``: ``ransac_th``, ``options`` and ``estimator``.

    A batch ``[B, ...]`` gives ``[B]`` device tensors without a host sync; an unbatched pair gives Python
    numbers through one sync."""
    conf = dict(conf or {})
    est = load_estimator("relative_pose", conf.pop("estimator", "hip"))(conf)
    _need(pred, _PRED_KEYS, "pred")
    _need(data, ["view0", "view1", "T_0to1"], "data")
    _need(data["view0"], ["camera"], "data['view0']")
    _need(data["view1"], ["camera"], "data['view1']")
    kp0, kp1, m0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"]
    for name, t in (("keypoints0", kp0), ("keypoints1", kp1), ("matches0", m0)):
        if not torch.is_tensor(t):
            raise TypeError(f"relative_pose: {name} must be a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
    single = kp0.dim() == 2
    nk0 = pred.get("num_keypoints0", data.get("num_keypoints0"))
    nk1 = pred.get("num_keypoints1", data.get("num_keypoints1"))
    cam0, cam1, T = data["view0"]["camera"], data["view1"]["camera"], data["T_0to1"]
    if single:
        kp0, kp1, m0 = kp0[None], kp1[None], m0[None]
        if nk0 is not None and nk1 is not None:
            nk0, nk1 = torch.as_tensor(nk0).reshape(1), torch.as_tensor(nk1).reshape(1)
        cam0, cam1, T = (getattr(x, "_data", x) for x in (cam0, cam1, T))
        cam0, cam1 = cam0.reshape(1, -1), cam1.reshape(1, -1)
        T = T[None] if T.shape[-2:] == (4, 4) else T.reshape(1, -1)
    o = est.conf.options
    r = ransac_relpose(kp0, kp1, m0, cam0, cam1, est.conf.ransac_th, nk0, nk1, o.max_iters, o.confidence, o.seed, T_gt=T)
    info = r["info"]
    inl = info[:, 2].to(torch.float32)
    M = Pose.from_Rt(r["R"], r["t"])
    out = {"rel_pose_error": r["rel_pose_error"], "ransac_inl": inl,
           "ransac_inl%": inl / info[:, 1].clamp(min=1).to(torch.float32), "M_0to1": M, "inliers": r["inliers"]}
    if single:
        keys = ("rel_pose_error", "ransac_inl", "ransac_inl%")
        vals = torch.stack([out[k][0].to(torch.float64) for k in keys]).tolist()
        out = {**dict(zip(keys, vals)), "M_0to1": M[0], "inliers": r["inliers"][0]}
    return out


def as_export_callback(conf=None):
    """A ``callback_fn`` for :func:`export.export_predictions`: adds the per-pair robust results to ``pred``."""
    def callback(pred, data):
        return eval_relative_pose_robust(data, pred, conf)

    return callback
