"""Wireframe extractor in front of GlueStick: the reference's ``lines.wireframe``
(``gluefactory/models/lines/wireframe.py``), the ``extractor`` of its ``superpoint+lsd+gluestick*``
configs, on the HIP library, and the ``lines.lsd`` host wrapper (``models/lines/lsd.py``).

The reference copies the line endpoints to the host, runs ``sklearn.cluster.DBSCAN(eps=nms_radius,
min_samples=1)`` and a Python loop of ``scatter_reduce_`` / ``grid_sample`` per image.  With
``min_samples=1`` every point is a core point, so the clusters are the connected components of
"distance <= eps" numbered by their lowest point index; here that, the junction means and scores,
the rewritten lines, the keypoint merge, the descriptor sampling and the connectivity matrices are
``lg_wireframe_forward`` (csrc/wireframe.hip).

Differences from the reference:

* ``line_extractor.name: None``: the segments come with the data (``data["lines"]`` [B, L, 2, 2],
  ``data["line_scores"]`` [B, L], optional ``data["valid_lines"]``); the reference fails in
  ``get_model(None)``.
* Random fills: removed keypoint (b, k) takes row (b, k) of ``data.get("fill_keypoints")`` [B, K, 2]
  and junction slot j >= n_true of image b takes row j - n_true of ``fill_junctions`` /
  ``data.get("fill_junctions")`` [B, 2 * max_num_lines, 2]; both default to ``torch.rand`` on the
  device scaled by (w - 1, h - 1).  The reference draws ``torch.rand`` rows in batch-major order of
  removal (keypoints) and from the CPU generator (junctions).
* Forced mode (``force_num_keypoints`` and ``force_num_lines``) does no device-to-host copy:
  ``num_junctions`` is a [B] device tensor.  Free mode reads the junction and kept-keypoint counts in
  one copy and returns ``num_junctions`` on the CPU like the reference.
* ``torch.cuda.empty_cache()`` is not called and the caller's ``line_scores`` is not modified in place.
* ``lines_to_wireframe`` returns ``junc_scores`` and ``connectivity`` as [B, ...] tensors (the
  reference: lists of per-image tensors), and takes the dense map as [B, D, Hc, Wc] like the reference
  (an NHWC-contiguous permuted view is read in place).
* Sub-extractor configs: keys whose value is None are left to the sub-extractor's own default.
* At most ``MAX_LINES`` (2048) lines per image; CPU inputs raise.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._native import _ptr
from .pipeline import BaseModel, get_model

MAX_LINES = _lib.LG_WIREFRAME_MAX_LINES


def _need_device(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("lightglue_amd: inputs must be on a HIP (cuda) device; there is no CPU path")


def _f32(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


def _nhwc(dense):
    """[B, D, Hc, Wc] -> an NHWC-contiguous [B, Hc, Wc, D] tensor (the extractors' permuted view as it is)."""
    assert dense.dim() == 4, "dense descriptors must be [B, D, Hc, Wc]"
    d = dense.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
    if d.shape[3] % 4 != 0 or d.shape[3] > _lib.LG_WIREFRAME_MAX_DIM:
        raise ValueError(f"descriptor width must be a multiple of 4 up to {_lib.LG_WIREFRAME_MAX_DIM}, got {d.shape[3]}")
    return d.clone() if d.data_ptr() % 16 else d


def sample_descriptors_corner_conv(keypoints, descriptors, s: int = 8):
    """``wireframe.py:8-19``: keypoints [B, P, 2] pixels, descriptors [B, D, Hc, Wc] -> [B, D, P]."""
    _need_device(keypoints, descriptors)
    dense = _nhwc(descriptors)
    pts = _f32(keypoints)
    B, Hc, Wc, D = dense.shape
    assert pts.dim() == 3 and pts.shape[0] == B and pts.shape[2] == 2
    P = pts.shape[1]
    out = torch.empty((B, P, D), dtype=torch.float32, device=dense.device)
    with torch.cuda.device(dense.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dense.device).cuda_stream)
        _lib.check(_lib.load().lg_sample_descriptors_corner(_ptr(pts), _ptr(dense), B, P, Hc, Wc, D, int(s), _ptr(out), stream),
                   "lg_sample_descriptors_corner")
    return out.transpose(1, 2)


def _connectivity(lib, idx, B, L, N, identity_only, device, stream):
    out = torch.empty((B, N, N), dtype=torch.bool, device=device)
    _lib.check(lib.lg_wireframe_connectivity(_ptr(idx), B, L, N, int(identity_only), _ptr(out), stream),
               "lg_wireframe_connectivity")
    return out


def _wireframe(lines, line_scores, dense, s, nms_radius, *, merge_points, merge_line_endpoints, force_num_keypoints,
               force_num_lines, max_num_lines, keypoints=None, keypoint_scores=None, descriptors=None, fill_junctions=None,
               fill_keypoints=None, want_connectivity=False, want_pl=True):
    """The whole step.  Returns a dict of the combined [junction slots | keypoints] tensors, the lines
    and the counts (``n_true`` / ``n_kept``: device tensors when every shape is static, else ints)."""
    _need_device(lines, line_scores, dense, keypoints, keypoint_scores, descriptors)
    dev = lines.device
    dense = _nhwc(dense)
    B, Hc, Wc, D = dense.shape
    lines = _f32(lines)
    line_scores = _f32(line_scores)
    assert lines.dim() == 4 and lines.shape[0] == B and lines.shape[2:] == (2, 2), "lines must be [B, L, 2, 2]"
    L = lines.shape[1]
    assert line_scores.shape == (B, L), "line_scores must be [B, L]"
    if L > MAX_LINES:
        raise ValueError(f"lines.wireframe: at most {MAX_LINES} lines per image, got {L}")
    K = 0 if keypoints is None else keypoints.shape[1]
    if K:
        keypoints, keypoint_scores, descriptors = _f32(keypoints), _f32(keypoint_scores), _f32(descriptors)
        assert keypoints.shape == (B, K, 2) and keypoint_scores.shape == (B, K) and descriptors.shape == (B, K, D)
        if descriptors.data_ptr() % 16:
            descriptors = descriptors.clone()
    merge_line_endpoints = bool(merge_line_endpoints) and L > 0  # wireframe.py:220-223
    fill_slots = bool(force_num_lines) and merge_line_endpoints
    force_kp = bool(force_num_keypoints) or not merge_points
    if fill_slots:
        J = 2 * int(max_num_lines)
        if J < 2 * L:
            raise ValueError(f"lines.wireframe: {L} lines exceed max_num_lines = {max_num_lines}")
    else:
        J = 2 * L
    static = (fill_slots or not merge_line_endpoints) and force_kp
    if not static and B != 1:
        raise ValueError("lines.wireframe: only a batch size of 1 is accepted for non padded inputs")
    wh = torch.tensor([Wc * s - 1, Hc * s - 1], dtype=torch.float32, device=dev)
    if fill_slots:
        if fill_junctions is None:
            fill_junctions = torch.rand((B, J, 2), device=dev) * wh
        fill_junctions = _f32(fill_junctions.to(dev))
        assert fill_junctions.shape == (B, J, 2), "fill_junctions must be [B, 2 * max_num_lines, 2]"
    else:
        fill_junctions = None
    if force_num_keypoints and merge_points and K:
        if fill_keypoints is None:
            fill_keypoints = torch.rand((B, K, 2), device=dev) * wh
        fill_keypoints = _f32(fill_keypoints.to(dev))
        assert fill_keypoints.shape == (B, K, 2), "fill_keypoints must be [B, K, 2]"
    else:
        fill_keypoints = None
    N = J + K
    out = {
        "points": torch.empty((B, N, 2), dtype=torch.float32, device=dev),
        "scores": torch.empty((B, N), dtype=torch.float32, device=dev),
        "descriptors": torch.empty((B, N, D), dtype=torch.float32, device=dev),
        "lines": torch.empty((B, L, 2, 2), dtype=torch.float32, device=dev),
        "lines_junc_idx": torch.empty((B, L, 2), dtype=torch.int64, device=dev),
        "counts": torch.empty((2, B), dtype=torch.int32, device=dev),
        "removed": torch.empty((B, K), dtype=torch.bool, device=dev),
    }
    conn = pl = None
    if static:
        if want_connectivity:
            conn = torch.empty((B, J, J), dtype=torch.bool, device=dev)
        if want_pl:
            pl = torch.empty((B, N, N), dtype=torch.bool, device=dev)
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.lg_wireframe_workspace_bytes(B, L, K, ctypes.byref(nb)), "lg_wireframe_workspace_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    cfg = _lib.WFConfig(float(nms_radius), int(bool(merge_points)), int(merge_line_endpoints), int(bool(force_num_keypoints)),
                        int(bool(force_num_lines)), int(s), 0)
    inp = _lib.WFInputs(B, L, K, J, D, Hc, Wc, 0, _ptr(lines), _ptr(line_scores), _ptr(keypoints) if K else None,
                        _ptr(keypoint_scores) if K else None, _ptr(descriptors) if K else None, _ptr(dense),
                        _ptr(fill_junctions), _ptr(fill_keypoints))
    o = _lib.WFOutputs(_ptr(out["points"]), _ptr(out["scores"]), _ptr(out["descriptors"]), _ptr(out["lines"]),
                       _ptr(out["lines_junc_idx"]), _ptr(out["counts"]), _ptr(out["removed"]) if K else None, _ptr(conn),
                       _ptr(pl))
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.lg_wireframe_forward(ctypes.byref(cfg), ctypes.byref(inp), ctypes.byref(o), _ptr(ws), nb.value, stream),
                   "lg_wireframe_forward")
        if static:
            n_true, n_kept, nJ = out["counts"][0].long(), out["counts"][1].long(), J
        else:
            n_true, n_kept = (int(v) for v in out["counts"][:, 0].cpu())  # the one device-to-host copy
            nJ = J if fill_slots else n_true
            if (nJ, n_kept) != (J, K):
                for k in ("points", "scores", "descriptors"):
                    out[k] = torch.cat([out[k][:, :nJ], out[k][:, J:J + n_kept]], dim=1)
            if want_connectivity:
                conn = _connectivity(lib, out["lines_junc_idx"], B, L, nJ, not merge_line_endpoints, dev, stream)
            if want_pl:
                pl = _connectivity(lib, out["lines_junc_idx"], B, L, nJ + n_kept, not merge_line_endpoints, dev, stream)
    out.update(connectivity=conn, pl_associativity=pl, n_true=n_true, n_kept=n_kept, J=nJ, static=static)
    return out


def lines_to_wireframe(lines, line_scores, dense_desc, s, nms_radius, force_num_lines, max_num_lines, fill_junctions=None):
    """``wireframe.py:22-128`` on the device.  Returns (junctions [B, J, 2], junc_scores [B, J],
    junc_descs [B, J, D], connectivity [B, J, J], new_lines, lines_junc_idx, num_true_junctions); J is
    ``2 * max_num_lines`` with ``force_num_lines`` (slot j >= n_true of image b takes
    ``fill_junctions[b, j - n_true]``) and the junction count otherwise (B = 1)."""
    if lines.shape[1] == 0:
        raise ValueError("lines_to_wireframe needs at least one line")
    r = _wireframe(lines, line_scores, dense_desc, s, nms_radius, merge_points=False, merge_line_endpoints=True,
                   force_num_keypoints=True, force_num_lines=force_num_lines, max_num_lines=max_num_lines,
                   fill_junctions=fill_junctions, want_connectivity=True, want_pl=False)
    n_true = r["n_true"] if r["static"] else [r["n_true"]]
    return (r["points"], r["scores"], r["descriptors"], r["connectivity"], r["lines"], r["lines_junc_idx"], n_true)


def _sub_conf(conf):
    return {k: v for k, v in dict(conf).items() if v is not None or k == "name"}


class WireframeExtractor(BaseModel):
    default_conf = {  # wireframe.py:132-152
        "point_extractor": {
            "name": None,
            "trainable": False,
            "dense_outputs": True,
            "max_num_keypoints": None,
            "force_num_keypoints": False,
        },
        "line_extractor": {
            "name": None,
            "trainable": False,
            "max_num_lines": None,
            "force_num_lines": False,
            "min_length": 15,
        },
        "wireframe_params": {
            "merge_points": True,
            "merge_line_endpoints": True,
            "nms_radius": 3,
        },
    }
    required_data_keys = ["image"]

    def _init(self, conf):
        self.point_extractor = get_model(conf.point_extractor.name)(_sub_conf(conf.point_extractor))
        # name None: the segments come with the data (no reference counterpart)
        self.line_extractor = None
        if conf.line_extractor.name is not None:
            self.line_extractor = get_model(conf.line_extractor.name)(_sub_conf(conf.line_extractor))
        if conf.line_extractor.force_num_lines:
            assert conf.line_extractor.max_num_lines is not None, "Missing max_num_lines parameter"

    def _forward(self, data):
        c = self.conf
        image = data["image"]
        b_size, _, h, w = image.shape
        forced_kp, forced_lines = bool(c.point_extractor.force_num_keypoints), bool(c.line_extractor.force_num_lines)
        if not forced_kp or not forced_lines:
            assert b_size == 1, "Only batch size of 1 accepted for non padded inputs"
        _need_device(image)

        # Line detection
        if self.line_extractor is not None:
            pred = dict(self.line_extractor(data))
        else:
            for k in ("lines", "line_scores"):
                assert k in data, f"Missing key {k} in data (line_extractor.name is None)"
            pred = {"lines": data["lines"], "line_scores": data["line_scores"]}
            if "valid_lines" in data:
                pred["valid_lines"] = data["valid_lines"]
        _need_device(pred["lines"], pred["line_scores"])
        pred["lines"] = pred["lines"].to(torch.float32)
        if pred["line_scores"].shape[-1] != 0:  # out of place: the caller's tensor stays as it was
            pred["line_scores"] = pred["line_scores"] / (pred["line_scores"].max(dim=1)[0][:, None] + 1e-8)

        # Keypoint prediction
        pred = {**pred, **self.point_extractor(data)}
        assert "dense_descriptors" in pred, "The KP extractor should return dense descriptors"
        dense = pred.pop("dense_descriptors")  # dropped from the outputs
        s_desc = image.shape[2] // dense.shape[2]

        wp = c.wireframe_params
        r = _wireframe(pred["lines"], pred["line_scores"], dense, s_desc, wp.nms_radius, merge_points=bool(wp.merge_points),
                       merge_line_endpoints=bool(wp.merge_line_endpoints), force_num_keypoints=forced_kp,
                       force_num_lines=forced_lines, max_num_lines=c.line_extractor.max_num_lines,
                       keypoints=pred["keypoints"], keypoint_scores=pred["keypoint_scores"], descriptors=pred["descriptors"],
                       fill_junctions=data.get("fill_junctions"), fill_keypoints=data.get("fill_keypoints"))
        pred["orig_lines"] = pred["lines"]
        pred["lines"] = r["lines"]
        pred["keypoints"] = r["points"]
        pred["keypoint_scores"] = r["scores"]
        pred["descriptors"] = r["descriptors"]
        pred["pl_associativity"] = r["pl_associativity"]
        pred["num_junctions"] = r["n_true"] if r["static"] else torch.tensor([r["n_true"]])
        pred["lines_junc_idx"] = r["lines_junc_idx"]
        return pred

    def loss(self, pred, data):
        raise NotImplementedError

    def metrics(self, _pred, _data):
        return {}


def _pytlsd(img):
    try:
        from pytlsd import lsd
    except ImportError as e:
        raise ImportError("lines.lsd needs the pytlsd package (the LSD detector itself runs on the host and is not "
                          "part of this library); install it or set LSD.detector to a callable "
                          "img [H, W] uint8 -> segments [n, 5] (x1, y1, x2, y2, nfa)") from e
    return lsd(img)


class LSD(BaseModel):
    """``models/lines/lsd.py``: host plumbing around a CPU line-segment detector, as in the reference."""

    default_conf = {  # lsd.py:10-15
        "min_length": 15,
        "max_num_lines": None,
        "force_num_lines": False,
        "n_jobs": 4,
    }
    required_data_keys = ["image"]
    detector = staticmethod(_pytlsd)  # img [H, W] uint8 -> [n, >= 5] rows (x1, y1, x2, y2, ..., nfa)

    def _init(self, conf):
        if conf.force_num_lines:
            assert conf.max_num_lines is not None, "Missing max_num_lines parameter"

    def detect_lines(self, img):  # lsd.py:24-53
        segs = np.asarray(self.__dict__.get("detector", type(self).detector)(img))
        segs = segs.reshape(-1, segs.shape[-1] if segs.ndim == 2 else 5)
        lengths = np.linalg.norm(segs[:, 2:4] - segs[:, 0:2], axis=1)
        to_keep = lengths >= self.conf.min_length
        segs, lengths = segs[to_keep], lengths[to_keep]
        scores = segs[:, -1] * np.sqrt(lengths)
        segs = segs[:, :4].reshape(-1, 2, 2)
        indices = np.argsort(-scores)
        if self.conf.max_num_lines is not None:
            indices = indices[: self.conf.max_num_lines]
            segs = segs[indices]
            scores = scores[indices]
        n = len(segs)
        valid_mask = np.ones(n, dtype=bool)
        if self.conf.force_num_lines:
            pad = self.conf.max_num_lines - n
            segs = np.concatenate([segs, np.zeros((pad, 2, 2), dtype=np.float32)], axis=0)
            scores = np.concatenate([scores, np.zeros(pad, dtype=np.float32)], axis=0)
            valid_mask = np.concatenate([valid_mask, np.zeros(pad, dtype=bool)], axis=0)
        return segs, scores, valid_mask

    def _forward(self, data):  # lsd.py:55-85
        image = data["image"]
        if image.shape[1] == 3:
            scale = image.new_tensor([0.299, 0.587, 0.114]).view(1, 3, 1, 1)
            image = (image * scale).sum(1, keepdim=True)
        device = image.device
        b_size = len(image)
        image = np.uint8(image.squeeze(1).cpu().numpy() * 255)
        lines, line_scores, valid_lines = zip(*(self.detect_lines(img) for img in image))
        if b_size == 1 or self.conf.force_num_lines:
            lines = torch.tensor(np.stack(lines), dtype=torch.float, device=device)
            line_scores = torch.tensor(np.stack(line_scores), dtype=torch.float, device=device)
            valid_lines = torch.tensor(np.stack(valid_lines), dtype=torch.bool, device=device)
        return {"lines": lines, "line_scores": line_scores, "valid_lines": valid_lines}

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = WireframeExtractor
