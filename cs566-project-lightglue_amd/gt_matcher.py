"""Homography ground truth for training: the reference's ``matchers.homography_matcher``
(``gluefactory/models/matchers/homography_matcher.py``), the ``ground_truth`` component of its
homography training configs, on the HIP library.

``gt_matches_from_homography`` (``geometry/gt_generation.py:109-161``) is a chain of dense
[B, M, N] torch passes, two of them through [B, M, N, 2]; here it is ``lg_gt_matches_from_homography``
(csrc/gt_match.hip): a statistics pass that writes nothing of size M*N and a write pass for the
assignment and the reward.

Differences from the reference:

* ``reward`` (default True): ``False`` skips the reward (4 of the 5 bytes written per entry; neither
  LightGlue.loss nor SuperGlue.loss reads it) and omits the key.
* ``use_lines: True`` raises at construction under this name (its tests pin that).  Line ground truth from
  homographies is ``matchers.line_homography_matcher`` (:mod:`~lightglue_amd.line_gt`): this matcher with
  ``use_lines`` on, the assignment solved on the device.
* With no keypoints in either image the reference returns a tuple its pipeline cannot merge; here the
  dict comes back with that tuple's contents (all-false assignment, matches -1) and empty / zero rest.
"""
import ctypes

import torch

from . import _lib
from ._native import _ptr
from .pipeline import BaseModel


def gt_matches_from_homography(kp0, kp1, H, pos_th=3, neg_th=6, reward=True):
    """``gt_generation.py:109-161`` on the device.  kp0 [B,M,2], kp1 [B,N,2], H [B,3,3] or [3,3]."""
    dev = kp0.device
    if dev.type != "cuda" or kp1.device.type != "cuda" or H.device.type != "cuda":
        raise RuntimeError("lightglue_amd: inputs must be on a HIP (cuda) device; there is no CPU path")
    kp0 = kp0.detach().to(torch.float32).contiguous()
    kp1 = kp1.detach().to(torch.float32).contiguous()
    B, M = kp0.shape[:2]
    N = kp1.shape[1]
    H = H.detach().to(torch.float32)
    if H.dim() == 2:
        H = H[None].expand(B, 3, 3)
    H = H.contiguous()
    assert kp0.shape == (B, M, 2) and kp1.shape == (B, N, 2) and H.shape == (B, 3, 3)
    out = {"assignment": torch.empty((B, M, N), dtype=torch.bool, device=dev)}
    if reward:
        out["reward"] = torch.empty((B, M, N), dtype=torch.float32, device=dev)
    out["matches0"] = torch.empty((B, M), dtype=torch.int64, device=dev)
    out["matches1"] = torch.empty((B, N), dtype=torch.int64, device=dev)
    out["matching_scores0"] = torch.empty((B, M), dtype=torch.float32, device=dev)
    out["matching_scores1"] = torch.empty((B, N), dtype=torch.float32, device=dev)
    out["proj_0to1"] = torch.empty((B, M, 2), dtype=torch.float32, device=dev)
    out["proj_1to0"] = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
    if M == 0 or N == 0:  # :111-119: nothing to compare; the tuple's contents, as the dict
        out["matches0"].fill_(-1)
        out["matches1"].fill_(-1)
        for k in ("matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0"):
            out[k].zero_()
        return out
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_gt_homography_workspace_bytes(B, M, N, ctypes.byref(nb)), "lg_gt_homography_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(
            lib.lg_gt_matches_from_homography(
                _ptr(kp0), _ptr(kp1), _ptr(H), B, M, N, float(pos_th), float(neg_th), _ptr(out["assignment"]),
                _ptr(out.get("reward")), _ptr(out["matches0"]), _ptr(out["matches1"]), _ptr(out["matching_scores0"]),
                _ptr(out["matching_scores1"]), _ptr(out["proj_0to1"]), _ptr(out["proj_1to0"]), _ptr(ws), nb.value,
                ctypes.c_void_p(stream)),
            "lg_gt_matches_from_homography",
        )
    return out


class HomographyMatcher(BaseModel):
    default_conf = {  # homography_matcher.py:9-20
        # GT parameters for points
        "use_points": True,
        "th_positive": 3.0,
        "th_negative": 3.0,
        # GT parameters for lines
        "use_lines": False,
        "n_line_sampled_pts": 50,
        "line_perp_dist_th": 5,
        "overlap_th": 0.2,
        "min_visibility_th": 0.5,
        # no reference counterpart: False skips the [B, M, N] fp32 reward and omits the key
        "reward": True,
    }

    required_data_keys = ["H_0to1", "keypoints0", "keypoints1"]

    def _init(self, conf):
        if conf.use_lines:
            raise NotImplementedError(
                "homography_matcher: use_lines is not served under this name; use matchers.line_homography_matcher")
        if not conf.use_points:  # :26-27: the keypoints are required only with use_points
            self.required_data_keys = ["H_0to1"]

    def _forward(self, data):
        if not self.conf.use_points:
            return {}
        return gt_matches_from_homography(data["keypoints0"], data["keypoints1"], data["H_0to1"],
                                          pos_th=self.conf.th_positive, neg_th=self.conf.th_negative,
                                          reward=bool(self.conf.reward))

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = HomographyMatcher
