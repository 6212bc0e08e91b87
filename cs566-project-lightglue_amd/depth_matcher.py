"""Pose-and-depth ground truth for training: the reference's ``matchers.depth_matcher``
(``gluefactory/models/matchers/depth_matcher.py``), the ``ground_truth`` component of its posed-pair
(MegaDepth) training configs, on the HIP library.

``gt_matches_from_pose_depth`` (``geometry/gt_generation.py:13-106``) is four ``grid_sample`` calls
(eight with ``th_consistency``), the homography chain's dense [B, M, N] passes, a visibility mask, an
all-pairs epipolar distance and, with ``th_epi``, one more masked pass; here it is
``lg_gt_matches_from_pose_depth`` (csrc/gt_depth.hip): a point pass, statistics passes that write
nothing of size M*N and a write pass for the assignment and the reward.

Cameras and poses are taken duck-typed: any object with a ``_data`` tensor (the reference's ``Camera``
/ ``Pose``, or the two small holders below), a plain tensor ``[B, 6|8|10]`` / ``[B, 12]``, a pose as
``[B, 4, 4]``; an unbatched row broadcasts over B.

Differences from the reference:

* ``reward`` (default True): ``False`` skips the [B, M, N] fp32 reward and omits the key.
* ``use_lines: True`` raises at construction under this name (its tests pin that).  The pose-and-depth
  line ground truth (``gt_line_matches_from_pose_depth``) is ``matchers.line_depth_matcher``
  (:class:`~lightglue_amd.line_gt.LineDepthMatcher`): this matcher with ``use_lines`` on by default, its
  samples projected by the same device helpers as the keypoints here (csrc/gt_depth_common.h).
* With no keypoints in either image the reference returns a tuple its pipeline cannot merge; here the
  dict comes back with that tuple's contents (all-false assignment, matches -1) and empty / zero rest.
"""
import ctypes

import torch

from . import _lib
from ._native import _ptr
from .pipeline import BaseModel


class _Rows:
    """A tensor of parameter rows under ``_data``, as the reference's ``TensorWrapper``."""

    def __init__(self, data):
        self._data = data

    def to(self, *args, **kwargs):
        return self.__class__(self._data.to(*args, **kwargs))

    @property
    def shape(self):
        return self._data.shape[:-1]

    def __getitem__(self, index):
        return self.__class__(self._data[index])

    def __repr__(self):
        return f"{self.__class__.__name__} {tuple(self.shape)} {self._data.dtype} {self._data.device}"


class Pose(_Rows):
    """``geometry/wrappers.py:111-177``: rows of 9 (R, row-major) + 3 (t).  A holder, not a geometry
    library: construction and ``inv`` only."""

    def __init__(self, data):
        assert data.shape[-1] == 12
        super().__init__(data)

    @classmethod
    def from_Rt(cls, R, t):
        assert R.shape[-2:] == (3, 3) and t.shape[-1] == 3 and R.shape[:-2] == t.shape[:-1]
        return cls(torch.cat([R.flatten(start_dim=-2), t], -1))

    @classmethod
    def from_4x4mat(cls, T):
        assert T.shape[-2:] == (4, 4)
        return cls.from_Rt(T[..., :3, :3], T[..., :3, 3])

    @property
    def R(self):
        return self._data[..., :9].reshape(self._data.shape[:-1] + (3, 3))

    @property
    def t(self):
        return self._data[..., -3:]

    def inv(self):
        R = self.R.transpose(-1, -2)
        t = -(R @ self.t.unsqueeze(-1)).squeeze(-1)
        return self.__class__.from_Rt(R, t)


class Camera(_Rows):
    """``geometry/wrappers.py:238-311``: rows of w, h, fx, fy, cx, cy and 0, 2 (k1, k2) or 4
    (k1, k2, p1, p2) distortion terms."""

    def __init__(self, data):
        assert data.shape[-1] in {6, 8, 10}
        super().__init__(data)

    @classmethod
    def from_calibration_matrix(cls, K):
        cx, cy = K[..., 0, 2], K[..., 1, 2]
        fx, fy = K[..., 0, 0], K[..., 1, 1]
        return cls(torch.stack([2 * cx, 2 * cy, fx, fy, cx, cy], -1))


def _rows(x, B, dev, what):
    """Camera or pose rows as a contiguous fp32 [B, W] tensor on ``dev``."""
    x = getattr(x, "_data", x)
    if not torch.is_tensor(x):
        raise TypeError(f"{what}: expected a tensor or an object with a _data tensor, got {type(x).__name__}")
    if what == "pose" and x.shape[-2:] == (4, 4):
        x = torch.cat([x[..., :3, :3].flatten(start_dim=-2), x[..., :3, 3]], -1)
    if x.dim() == 1:
        x = x[None].expand(B, -1)
    widths = (12,) if what == "pose" else (6, 8, 10)
    if x.dim() != 2 or x.shape[0] != B or x.shape[1] not in widths:
        raise ValueError(f"{what}: expected [{B}, {'|'.join(map(str, widths))}] rows, got {tuple(x.shape)}")
    if x.device != dev:
        raise RuntimeError(f"{what}: on {x.device}, the keypoints are on {dev}")
    return x.detach().to(torch.float32).contiguous()


def _depth(d, B, dev):
    if d is None:
        return None
    if d.dim() == 4 and d.shape[1] == 1:
        d = d[:, 0]
    assert d.dim() == 3 and d.shape[0] == B, f"depth: expected [{B}, H, W], got {tuple(d.shape)}"
    if d.device != dev:
        raise RuntimeError(f"depth: on {d.device}, the keypoints are on {dev}")
    return d.detach().to(torch.float32).contiguous()


def gt_matches_from_pose_depth(kp0, kp1, data, pos_th=3, neg_th=5, epi_th=None, cc_th=None, reward=True, **kw):
    """``gt_generation.py:13-106`` on the device.  kp0 [B,M,2], kp1 [B,N,2]; ``data`` holds
    ``view0`` / ``view1`` (``camera``, ``depth``), ``T_0to1`` and ``T_1to0``; ``kw`` may carry
    ``depth_keypoints0/1`` and ``valid_depth_keypoints0/1`` (:31-33)."""
    dev = kp0.device
    if dev.type != "cuda" or kp1.device != dev:
        raise RuntimeError("lightglue_amd: inputs must be on a HIP (cuda) device; there is no CPU path")
    kp0 = kp0.detach().to(torch.float32).contiguous()
    kp1 = kp1.detach().to(torch.float32).contiguous()
    B, M = kp0.shape[:2]
    N = kp1.shape[1]
    assert kp0.shape == (B, M, 2) and kp1.shape == (B, N, 2)
    pre = "depth_keypoints0" in kw and "depth_keypoints1" in kw

    def empty(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    out = {"assignment": empty((B, M, N), torch.bool)}
    if reward:
        out["reward"] = empty((B, M, N), torch.float32)
    out["matches0"] = empty((B, M), torch.int64)
    out["matches1"] = empty((B, N), torch.int64)
    out["matching_scores0"] = empty((B, M), torch.float32)
    out["matching_scores1"] = empty((B, N), torch.float32)
    if pre:
        out["depth_keypoints0"], out["depth_keypoints1"] = kw["depth_keypoints0"], kw["depth_keypoints1"]
    else:
        out["depth_keypoints0"] = empty((B, M), torch.float32)
        out["depth_keypoints1"] = empty((B, N), torch.float32)
    out["proj_0to1"] = empty((B, M, 2), torch.float32)
    out["proj_1to0"] = empty((B, N, 2), torch.float32)
    out["visible0"] = empty((B, M), torch.bool)
    out["visible1"] = empty((B, N), torch.bool)
    if M == 0 or N == 0:  # :17-25: nothing to compare; the tuple's contents, as the dict
        out["matches0"].fill_(-1)
        out["matches1"].fill_(-1)
        for k in ("matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0", "visible0", "visible1"):
            out[k].zero_()
        if not pre:
            out["depth_keypoints0"].zero_()
            out["depth_keypoints1"].zero_()
        return out

    cam0 = _rows(data["view0"]["camera"], B, dev, "camera")
    cam1 = _rows(data["view1"]["camera"], B, dev, "camera")
    if cam0.shape[1] != cam1.shape[1]:
        raise ValueError("the two cameras must have the same number of distortion terms")
    T01, T10 = _rows(data["T_0to1"], B, dev, "pose"), _rows(data["T_1to0"], B, dev, "pose")
    depth0, depth1 = _depth(data["view0"].get("depth"), B, dev), _depth(data["view1"].get("depth"), B, dev)
    if pre:
        dk0 = kw["depth_keypoints0"].detach().to(torch.float32).contiguous()
        dk1 = kw["depth_keypoints1"].detach().to(torch.float32).contiguous()
        v0 = kw["valid_depth_keypoints0"].detach().to(torch.bool).contiguous()
        v1 = kw["valid_depth_keypoints1"].detach().to(torch.bool).contiguous()
        assert dk0.shape == (B, M) and dk1.shape == (B, N) and v0.shape == (B, M) and v1.shape == (B, N)
    else:
        assert depth0 is not None and depth1 is not None  # :35-36
        dk0, dk1, v0, v1 = out["depth_keypoints0"], out["depth_keypoints1"], None, None
    if cc_th is not None and (depth0 is None or depth1 is None):
        cc_th = None  # depth.py:58: without the other map there is no consistency check
    H0, W0 = depth0.shape[1:] if depth0 is not None else (0, 0)
    H1, W1 = depth1.shape[1:] if depth1 is not None else (0, 0)

    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_gt_depth_workspace_bytes(B, M, N, ctypes.byref(nb)), "lg_gt_depth_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    nan = float("nan")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(
            lib.lg_gt_matches_from_pose_depth(
                _ptr(kp0), _ptr(kp1), _ptr(depth0), H0, W0, _ptr(depth1), H1, W1, _ptr(cam0), _ptr(cam1),
                cam0.shape[1] - 6, _ptr(T01), _ptr(T10), B, M, N, float(pos_th), float(neg_th),
                nan if epi_th is None else float(epi_th), nan if cc_th is None else float(cc_th),
                _ptr(dk0), _ptr(dk1), _ptr(v0), _ptr(v1), _ptr(out["assignment"]), _ptr(out.get("reward")),
                _ptr(out["matches0"]), _ptr(out["matches1"]), _ptr(out["matching_scores0"]),
                _ptr(out["matching_scores1"]), _ptr(out["proj_0to1"]), _ptr(out["proj_1to0"]), _ptr(out["visible0"]),
                _ptr(out["visible1"]), _ptr(ws), nb.value, ctypes.c_void_p(stream)),
            "lg_gt_matches_from_pose_depth",
        )
    return out


class DepthMatcher(BaseModel):
    default_conf = {  # depth_matcher.py:11-24
        # GT parameters for points
        "use_points": True,
        "th_positive": 3.0,
        "th_negative": 5.0,
        "th_epi": None,  # add some more epi outliers
        "th_consistency": None,  # check for projection consistency in px
        # GT parameters for lines
        "use_lines": False,
        "n_line_sampled_pts": 50,
        "line_perp_dist_th": 5,
        "overlap_th": 0.2,
        "min_visibility_th": 0.5,
        # no reference counterpart: False skips the [B, M, N] fp32 reward and omits the key
        "reward": True,
    }

    required_data_keys = ["view0", "view1", "T_0to1", "T_1to0"]

    def _init(self, conf):
        if conf.use_lines:
            raise NotImplementedError(
                "depth_matcher: use_lines is not served under this name; use matchers.line_depth_matcher")
        if conf.use_points:  # :30-31
            self.required_data_keys += ["keypoints0", "keypoints1"]

    def _forward(self, data):
        if not self.conf.use_points:
            return {}
        kw = {}
        if "depth_keypoints0" in data:  # :44-51
            keys = ["depth_keypoints0", "valid_depth_keypoints0", "depth_keypoints1", "valid_depth_keypoints1"]
            kw = {k: data[k] for k in keys}
        return gt_matches_from_pose_depth(data["keypoints0"], data["keypoints1"], data, pos_th=self.conf.th_positive,
                                          neg_th=self.conf.th_negative, epi_th=self.conf.th_epi,
                                          cc_th=self.conf.th_consistency, reward=bool(self.conf.reward), **kw)

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = DepthMatcher
