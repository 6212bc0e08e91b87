"""Batched match evaluation on the HIP library: the reference's ``eval_matches_homography``,
``eval_matches_epipolar`` and ``eval_homography_dlt`` (``gluefactory/eval/utils.py:40-91,176-196``),
which turn a matcher's ``matches0`` / ``matching_scores0`` into the reported numbers.

The reference evaluates one pair at a time through boolean-mask gathers, small matrix products, an
SVD and ``.item()``; here one launch of ``lg_eval_matches`` (csrc/match_eval.hip)
evaluates every pair of a batch, one workgroup per pair, in float64, and nothing returns to the host
until the caller asks for the numbers.

The same keys are read as in the reference: ``data`` supplies ``H_0to1``, ``view0.image_size``,
``view0/1.camera`` and ``T_0to1``; ``pred`` supplies ``keypoints0/1``, ``matches0`` and
``matching_scores0``.  Cameras and poses come in the forms ``depth_matcher`` accepts (the reference's
wrappers, ``depth_matcher.Camera`` / ``Pose``, plain rows, a pose as ``[B, 4, 4]``); only the first six
camera columns are used, as ``image2cam`` applies no undistortion.

Batched inputs ``[B, ...]`` give ``[B]`` device tensors (``H_dlt`` ``[B, 3, 3]``) without a host
sync.  An unbatched pair (``keypoints0.ndim == 2``) gives Python numbers through one sync, like the
reference, so the module drops into a per-pair loop.

Differences from the reference:

* ``pinverse(H_0to1)`` of the symmetric transfer error is the 3x3 adjugate inverse; the two are equal
  for the invertible homographies the datasets produce.
* ``pred`` or ``data`` ``["num_keypoints0/1"]`` (optional, as for the matchers) make the batch ragged:
  slots past a pair's counts are padding, whatever they hold, and ``num_keypoints`` becomes
  ``(num_keypoints0 + num_keypoints1) / 2``.  A match index at or beyond the partner count is not a match.
* With no matches ``prec@*`` is 0 (the reference's ``nan_to_num``) and ``epi_prec@*`` NaN (the
  reference does not guard it); with fewer than 4 matches ``H_dlt`` is all ``inf`` and ``H_error_dlt``
  NaN, which is what ``hpatches_metrics.eval_homography_dlt`` returns.
* Inputs that are not on the device raise; ``hpatches_metrics`` remains the CPU route.
"""
import ctypes

import torch

from . import _lib
from .depth_matcher import _ptr, _rows
from .lightglue import LightGlue

LG_EVAL_HOMOGRAPHY, LG_EVAL_EPIPOLAR, LG_EVAL_DLT = 1, 2, 4
METRICS = {"homography": LG_EVAL_HOMOGRAPHY, "epipolar": LG_EVAL_EPIPOLAR, "dlt": LG_EVAL_DLT}
_PRED_KEYS = ("keypoints0", "keypoints1", "matches0", "matching_scores0")


def _need(d, keys, what):
    for k in keys:
        if k not in d:
            raise KeyError(f"match_eval: {what} has no '{k}'")


def _f32(t, shape, name, dev):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"match_eval: {name}: expected {list(shape)}, got {list(t.shape)}")
    if t.device != dev:
        raise RuntimeError(f"match_eval: {name} is on {t.device}, the keypoints are on {dev}")
    return t.detach().to(torch.float32).contiguous()


def eval_matches(data, pred, metrics=("homography", "epipolar", "dlt")):
    """Any subset of the three metrics in one launch; the union of their result dicts."""
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    unknown = [m for m in metrics if m not in METRICS]
    if unknown or not metrics:
        raise ValueError(f"match_eval: metrics must be a non-empty subset of {sorted(METRICS)}, got {list(metrics)}")
    flags = 0
    for m in metrics:
        flags |= METRICS[m]
    hom, epi, dlt = (bool(flags & f) for f in (LG_EVAL_HOMOGRAPHY, LG_EVAL_EPIPOLAR, LG_EVAL_DLT))
    _need(pred, _PRED_KEYS, "pred")
    if hom or dlt:
        _need(data, ["H_0to1"], "data")
    if dlt:
        _need(data, ["view0"], "data")
        _need(data["view0"], ["image_size"], "data['view0']")
    if epi:
        _need(data, ["view0", "view1", "T_0to1"], "data")
        _need(data["view0"], ["camera"], "data['view0']")
        _need(data["view1"], ["camera"], "data['view1']")

    kp0, kp1, m0, sc = (pred[k] for k in _PRED_KEYS)
    single = kp0.dim() == 2
    if single:
        kp0, kp1, m0, sc = kp0[None], kp1[None], m0[None], sc[None]
    if kp0.dim() != 3 or kp1.dim() != 3 or kp0.shape[-1] != 2 or kp1.shape[-1] != 2 or kp0.shape[0] != kp1.shape[0]:
        raise ValueError(f"match_eval: keypoints: expected [B, M, 2] and [B, N, 2], got {list(kp0.shape)} and "
                         f"{list(kp1.shape)}")
    B, M = kp0.shape[:2]
    N = kp1.shape[1]
    if tuple(m0.shape) != (B, M) or tuple(sc.shape) != (B, M):
        raise ValueError(f"match_eval: matches0 and matching_scores0: expected [{B}, {M}], got {list(m0.shape)} and "
                         f"{list(sc.shape)}")
    nk0 = pred.get("num_keypoints0", data.get("num_keypoints0"))
    nk1 = pred.get("num_keypoints1", data.get("num_keypoints1"))
    if single and nk0 is not None and nk1 is not None:
        nk0, nk1 = torch.as_tensor(nk0).reshape(1), torch.as_tensor(nk1).reshape(1)
    nk0, nk1 = LightGlue._check_counts(nk0, nk1, B)
    dev = kp0.device
    if dev.type != "cuda":
        raise RuntimeError("lightglue_amd: inputs must be on a HIP (cuda) device; there is no CPU path")
    for name, t in (("keypoints1", kp1), ("matches0", m0), ("matching_scores0", sc)):
        if t.device != dev:
            raise RuntimeError(f"match_eval: {name} is on {t.device}, the keypoints are on {dev}")

    kp0 = kp0.detach().to(torch.float32).contiguous()
    kp1 = kp1.detach().to(torch.float32).contiguous()
    m0 = m0.detach().to(torch.int64).contiguous()
    sc = sc.detach().to(torch.float32).contiguous()
    if nk0 is not None:
        nk0 = nk0.to(device=dev, dtype=torch.int32).contiguous()
        nk1 = nk1.to(device=dev, dtype=torch.int32).contiguous()
    H = size0 = cam0 = cam1 = T = None
    if hom or dlt:
        H = data["H_0to1"]
        H = _f32(H[None] if single else H, (B, 3, 3), "H_0to1", dev)
    if dlt:
        size0 = torch.as_tensor(data["view0"]["image_size"])
        size0 = _f32(size0[None] if single else size0, (B, 2), "view0.image_size", dev)
    if epi:
        cam0 = _rows(data["view0"]["camera"], B, dev, "camera")[:, :6].contiguous()
        cam1 = _rows(data["view1"]["camera"], B, dev, "camera")[:, :6].contiguous()
        T = _rows(data["T_0to1"], B, dev, "pose")

    def empty(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    hc = empty((B, 3), torch.int32) if hom else None
    ec = empty((B, 4), torch.int32) if epi else None
    Hd = empty((B, 3, 3), torch.float32) if dlt else None
    He = empty((B,), torch.float32) if dlt else None
    if M == 0:  # no query keypoint: nothing is launched; the empty set's values
        for t in (hc, ec):
            if t is not None:
                t.zero_()
        if dlt:
            Hd.fill_(float("inf"))
            He.fill_(float("nan"))
    elif B > 0:
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(
                lib.lg_eval_matches(_ptr(kp0), _ptr(kp1), _ptr(m0), _ptr(sc), B, M, N, _ptr(nk0), _ptr(nk1), _ptr(H),
                                    _ptr(cam0), _ptr(cam1), _ptr(T), _ptr(size0), flags, _ptr(hc), _ptr(ec), _ptr(Hd),
                                    _ptr(He), ctypes.c_void_p(stream)),
                "lg_eval_matches",
            )

    out = {}
    if nk0 is None:
        nkp = torch.full((B,), (M + N) / 2.0, dtype=torch.float32, device=dev)
    else:
        nkp = (nk0 + nk1).to(torch.float32) / 2.0
    if hom:
        n = hc[:, 0].to(torch.float32)
        out["prec@1px"] = (hc[:, 1].to(torch.float32) / n).nan_to_num()
        out["prec@3px"] = (hc[:, 2].to(torch.float32) / n).nan_to_num()
        out["num_matches"], out["num_keypoints"] = hc[:, 0], nkp
    if epi:
        n = ec[:, 0].to(torch.float32)
        for i, k in enumerate(("epi_prec@1e-4", "epi_prec@5e-4", "epi_prec@1e-3")):
            out[k] = ec[:, i + 1].to(torch.float32) / n
        out["num_matches"], out["num_keypoints"] = ec[:, 0], nkp
    if dlt:
        out["H_error_dlt"], out["H_dlt"] = He, Hd
    if single:  # Python numbers through one copy, as the reference's .item()
        keys = [k for k in out if k != "H_dlt"]
        vals = torch.stack([out[k][0].to(torch.float64) for k in keys]).tolist()
        for k, v in zip(keys, vals):
            out[k] = int(v) if k == "num_matches" else v
        if dlt:
            out["H_dlt"] = Hd[0]
    return out


def _pick(out, keys):
    return {k: out[k] for k in keys}


def eval_matches_homography(data, pred):
    """``eval/utils.py:72-91``: prec@1px, prec@3px, num_matches, num_keypoints."""
    return _pick(eval_matches(data, pred, ("homography",)), ("prec@1px", "prec@3px", "num_matches", "num_keypoints"))


def eval_matches_epipolar(data, pred):
    """``eval/utils.py:40-69``: epi_prec@1e-4, epi_prec@5e-4, epi_prec@1e-3, num_matches, num_keypoints."""
    return _pick(eval_matches(data, pred, ("epipolar",)),
                 ("epi_prec@1e-4", "epi_prec@5e-4", "epi_prec@1e-3", "num_matches", "num_keypoints"))


def eval_homography_dlt(data, pred):
    """``eval/utils.py:176-196``: H_error_dlt, and the estimated homography as H_dlt."""
    return _pick(eval_matches(data, pred, ("dlt",)), ("H_error_dlt", "H_dlt"))


def as_export_callback(metrics=("homography", "dlt")):
    """A ``callback_fn`` for :func:`export.export_predictions`: adds the per-pair metric tensors to
    ``pred``, so they are written per pair with the predictions."""
    def callback(pred, data):
        return eval_matches(data, pred, metrics)

    return callback
