"""Nearest-neighbour matcher: the reference's ``matchers.nearest_neighbor_matcher``
(``gluefactory/models/matchers/nearest_neighbor_matcher.py``), the baseline of its ``*+NN.yaml``
configs, on the HIP library.

The reference is a chain of dense torch passes over the [B, M, N] similarity (``:16-72``: the einsum,
a transposed view, two ``topk``, two ``log_softmax``); here it is ``lg_nn_match`` (csrc/nn_match.hip):
one fp16x3 tile pass that keeps each row's and column's two best values and the index of the best,
the thresholds and the mutual check on those, and a second tile pass only for ``log_assignment``.

Differences from the reference:

* ``similarity`` / ``log_assignment`` (default True): ``False`` omits the key, and with both off
  nothing of size M*N is written.
* Exact ties pick the lowest index (``torch.topk`` leaves the order of equal values undefined); a tied
  best also counts as the second best, so the ratio test rejects it for ``ratio_thresh < 1``.
* ``data["num_keypoints0/1"]`` (optional, as for LightGlue): per-pair counts of a padded batch.  Padded
  points never win a search, their matches are -1 and scores 0; ``similarity`` is 0 and
  ``log_assignment`` -inf outside a pair's real block (its last row and column stay 0).  A pair with
  fewer than two real candidates on a side has no matches on the side that scans it while
  ``ratio_thresh`` is set.
* M or N equal to 0 returns all -1 matches, zero scores, an empty ``similarity`` and a zero
  ``log_assignment`` (the reference fails in ``topk``); a side of size 1 with ``ratio_thresh`` set
  raises ValueError (the reference's ``topk(2)`` fails too).
* ``loss: "N_pair"`` raises at construction: it needs a backward through the similarity.
"""
import ctypes

import torch

from . import _lib
from ._native import _ptr
from .lightglue import LightGlue
from .pipeline import BaseModel

LG_NN_RATIO, LG_NN_DISTANCE, LG_NN_MUTUAL = 1, 2, 4


def nn_match(desc0, desc1, ratio_thresh=None, distance_thresh=None, mutual_check=True, similarity=True,
             log_assignment=True, num_keypoints0=None, num_keypoints1=None):
    """``nearest_neighbor_matcher.py:16-72`` on the device.  desc0 [B,M,D], desc1 [B,N,D]."""
    dev = desc0.device
    if dev.type != "cuda" or desc1.device.type != "cuda":
        raise RuntimeError("lightglue_amd: inputs must be on a HIP (cuda) device; there is no CPU path")
    desc0 = desc0.detach().to(torch.float32).contiguous()
    desc1 = desc1.detach().to(torch.float32).contiguous()
    assert desc0.dim() == 3 and desc1.dim() == 3 and desc0.shape[0] == desc1.shape[0] and desc0.shape[2] == desc1.shape[2]
    B, M, D = desc0.shape
    N = desc1.shape[1]
    nk0, nk1 = LightGlue._check_counts(num_keypoints0, num_keypoints1, B)
    if nk0 is not None:  # any integer dtype, CPU or device -> int32 on the device
        nk0 = nk0.to(device=dev, dtype=torch.int32).contiguous()
        nk1 = nk1.to(device=dev, dtype=torch.int32).contiguous()
    flags = (LG_NN_RATIO if ratio_thresh else 0) | (LG_NN_DISTANCE if distance_thresh else 0) | (
        LG_NN_MUTUAL if mutual_check else 0)
    if ratio_thresh and M > 0 and N > 0 and min(M, N) < 2:
        raise ValueError("nearest_neighbor_matcher: ratio_thresh needs at least two candidates on each side "
                         f"(got M = {M}, N = {N})")
    out = {
        "matches0": torch.empty((B, M), dtype=torch.int64, device=dev),
        "matches1": torch.empty((B, N), dtype=torch.int64, device=dev),
        "matching_scores0": torch.empty((B, M), dtype=torch.float32, device=dev),
        "matching_scores1": torch.empty((B, N), dtype=torch.float32, device=dev),
    }
    if similarity:
        out["similarity"] = torch.empty((B, M, N), dtype=torch.float32, device=dev)
    if log_assignment:
        out["log_assignment"] = torch.empty((B, M + 1, N + 1), dtype=torch.float32, device=dev)
    if B == 0 or M == 0 or N == 0 or D == 0:  # nothing to compare
        out["matches0"].fill_(-1)
        out["matches1"].fill_(-1)
        for k in ("matching_scores0", "matching_scores1", "similarity", "log_assignment"):
            if k in out:
                out[k].zero_()
        return out
    if D % 32 == 0:  # read in place as 16-byte vectors: a view into a larger buffer may start off that alignment
        desc0 = desc0.clone() if desc0.data_ptr() % 16 else desc0
        desc1 = desc1.clone() if desc1.data_ptr() % 16 else desc1
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_nn_workspace_bytes(B, M, N, D, flags, ctypes.byref(nb)), "lg_nn_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(
            lib.lg_nn_match(
                _ptr(desc0), _ptr(desc1), B, M, N, D, float(ratio_thresh) ** 2 if ratio_thresh else 0.0,
                float(distance_thresh) ** 2 if distance_thresh else 0.0, flags, _ptr(nk0), _ptr(nk1),
                _ptr(out.get("similarity")), _ptr(out.get("log_assignment")), _ptr(out["matches0"]), _ptr(out["matches1"]),
                _ptr(out["matching_scores0"]), _ptr(out["matching_scores1"]), _ptr(ws), nb.value, ctypes.c_void_p(stream)),
            "lg_nn_match",
        )
    return out


class NearestNeighborMatcher(BaseModel):
    default_conf = {  # nearest_neighbor_matcher.py:39-44
        "ratio_thresh": None,
        "distance_thresh": None,
        "mutual_check": True,
        "loss": None,
        # no reference counterpart: False omits the key; with both off nothing of size M*N is written
        "similarity": True,
        "log_assignment": True,
    }
    required_data_keys = ["descriptors0", "descriptors1"]

    def _init(self, conf):
        if conf.loss == "N_pair":
            raise NotImplementedError(
                "nearest_neighbor_matcher: loss 'N_pair' (a backward through the similarity) is out of scope")

    def _forward(self, data):
        c = self.conf
        return nn_match(data["descriptors0"], data["descriptors1"], ratio_thresh=c.ratio_thresh,
                        distance_thresh=c.distance_thresh, mutual_check=bool(c.mutual_check),
                        similarity=bool(c.similarity), log_assignment=bool(c.log_assignment),
                        num_keypoints0=data.get("num_keypoints0"), num_keypoints1=data.get("num_keypoints1"))

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = NearestNeighborMatcher
