"""Callers on either side of the matcher: the two-view pipeline and the
model registry that resolve the matcher by name.

* :func:`get_model` — name -> model class, like ``gluefactory.models.get_model``
  (``models/__init__.py:7-30``): ``"matchers.lightglue"`` (and ``"lightglue"``) resolve to the HIP
  :class:`~lightglue_amd.lightglue.LightGlue` (the reference module's ``__main_model__``,
  ``lightglue.py:666``); ``"matchers.lightglue_pretrained_MINE"`` to the wrapper below;
  ``"two_view_pipeline"`` to :class:`TwoViewPipeline`; ``"matchers.homography_matcher"`` to the
  HIP ground-truth matcher (:mod:`~lightglue_amd.gt_matcher`); ``"matchers.line_homography_matcher"`` to
  the same with line ground truth (:mod:`~lightglue_amd.line_gt`); ``"matchers.depth_matcher"`` to the
  pose-and-depth one (:mod:`~lightglue_amd.depth_matcher`) and ``"matchers.line_depth_matcher"`` to that
  with line ground truth (:mod:`~lightglue_amd.line_gt`); ``"matchers.nearest_neighbor_matcher"`` to
  the nearest-neighbour baseline (:mod:`~lightglue_amd.nn_matcher`); ``"extractors.superpoint_open"`` to
  the open SuperPoint (:mod:`~lightglue_amd.superpoint_open`); ``"extractors.aliked"`` to ALIKED
  (:mod:`~lightglue_amd.aliked`); ``"matchers.gluestick"`` to the point-and-line matcher
  (:mod:`~lightglue_amd.gluestick`); ``"lines.wireframe"`` to the wireframe extractor in front of it and
  ``"lines.lsd"`` to the LSD host wrapper (:mod:`~lightglue_amd.wireframe`).  Other components (filters,
  solvers) are supplied by the caller through :func:`register_model`.
* :class:`LightGluePreTrainedMINE` — the reference's BaseModel wrapper
  (``matchers/lightglue_pretrained_MINE.py:8-36``): builds the matcher from its config and forwards
  ``data`` unchanged.
* :class:`TwoViewPipeline` — ``models/two_view_pipeline.py:21-121``: extractor per view (or the
  view's ``cache`` when ``allow_no_extract``), then matcher / filter / solver, each called on the
  merged dict ``{**data, **pred}`` and its outputs merged into ``pred``; ``loss`` runs the
  ``ground_truth`` component and sums the components' losses, which is what the reference's trainer
  calls (``train.py``: ``loss_fn = model.loss``).

Plain host-side plumbing: no arithmetic happens here beyond summing the components' totals; the
components' forward, loss and backward are the HIP paths.
"""
from torch import nn

from .lightglue import LightGlue, merge_conf

BASE_DEFAULT_CONF = {  # models/base_model.py:54-59
    "name": None,
    "trainable": True,
    "freeze_batch_normalization": False,
    "timeit": False,
}


class BaseModel(nn.Module):
    """The reference's BaseModel contract (``models/base_model.py:40-114``): class-level
    ``default_conf`` merged under the given config, ``required_data_keys`` checked recursively
    before ``_forward``; ``trainable: False`` freezes the parameters."""

    default_conf = {}
    required_data_keys = []

    def __init__(self, conf):
        super().__init__()
        self.conf = conf = merge_conf(BASE_DEFAULT_CONF, self.default_conf, conf)
        self.required_data_keys = list(self.required_data_keys)
        self._init(conf)
        if not conf.trainable:
            for p in self.parameters():
                p.requires_grad = False

    def _init(self, conf):
        raise NotImplementedError

    def _forward(self, data):
        raise NotImplementedError

    def forward(self, data):
        def check(expected, given):  # base_model.py:107-112
            for key in expected:
                assert key in given, f"Missing key {key} in data"
                if isinstance(expected, dict):
                    check(expected[key], given[key])

        check(self.required_data_keys, data)
        return self._forward(data)

    def loss(self, pred, data):
        raise NotImplementedError


class LightGluePreTrainedMINE(BaseModel):
    """matchers/lightglue_pretrained_MINE.py:8-36."""

    default_conf = {"features": "superpoint", **LightGlue.default_conf}
    required_data_keys = ["view0", "keypoints0", "descriptors0", "view1", "keypoints1", "descriptors1"]

    def _init(self, conf):
        self.net = LightGlue(dict(conf))

    def _forward(self, data):
        return self.net(data)

    def loss(self, pred, data):
        return self.net.loss(pred, data)


class TwoViewPipeline(BaseModel):
    """models/two_view_pipeline.py:21-121."""

    default_conf = {
        "extractor": {"name": None, "trainable": False},
        "matcher": {"name": None},
        "filter": {"name": None},
        "solver": {"name": None},
        "ground_truth": {"name": None},
        "allow_no_extract": False,
        "run_gt_in_forward": False,
    }
    required_data_keys = ["view0", "view1"]
    components = ["extractor", "matcher", "filter", "solver", "ground_truth"]

    def _init(self, conf):  # :44-60
        for k in self.components:
            if conf[k].name:
                setattr(self, k, get_model(conf[k].name)(dict(conf[k])))

    def extract_view(self, data, i):  # :62-77
        data_i = data[f"view{i}"]
        pred_i = data_i.get("cache", {})
        skip_extract = len(pred_i) > 0 and self.conf.allow_no_extract
        if self.conf.extractor.name and not skip_extract:
            pred_i = {**pred_i, **self.extractor(data_i)}
        elif self.conf.extractor.name and not self.conf.allow_no_extract:
            pred_i = {**pred_i, **self.extractor({**data_i, **pred_i})}
        return pred_i

    def _forward(self, data):  # :79-97
        pred0 = self.extract_view(data, "0")
        pred1 = self.extract_view(data, "1")
        pred = {**{k + "0": v for k, v in pred0.items()}, **{k + "1": v for k, v in pred1.items()}}
        for k in ("matcher", "filter", "solver"):
            if self.conf[k].name:
                pred = {**pred, **getattr(self, k)({**data, **pred})}
        if self.conf.ground_truth.name and self.conf.run_gt_in_forward:
            gt_pred = self.ground_truth({**data, **pred})
            pred.update({f"gt_{k}": v for k, v in gt_pred.items()})
        return pred

    def loss(self, pred, data):  # :99-121
        losses = {}
        metrics = {}
        total = 0

        # get labels
        if self.conf.ground_truth.name and not self.conf.run_gt_in_forward:
            gt_pred = self.ground_truth({**data, **pred})
            pred.update({f"gt_{k}": v for k, v in gt_pred.items()})

        for k in self.components:
            apply = True
            if "apply_loss" in self.conf[k].keys():
                apply = self.conf[k].apply_loss
            if self.conf[k].name and apply:
                try:
                    out = getattr(self, k).loss(pred, {**pred, **data})
                except NotImplementedError:
                    continue
                # the reference unpacks (losses, metrics) here, which its own SuperGlue.loss
                # (superglue.py:309-339, a bare dict of losses) does not survive: a dict is taken as
                # the losses with no metrics
                losses_, metrics_ = (out, {}) if isinstance(out, dict) else out
                losses = {**losses, **losses_}
                metrics = {**metrics, **metrics_}
                total = losses_["total"] + total
        return {**losses, "total": total}, metrics


def _superpoint():
    from .superpoint import SuperPoint

    return SuperPoint


def _superpoint_open():
    from .superpoint_open import SuperPoint

    return SuperPoint


def _superglue():
    from .superglue import SuperGlue

    return SuperGlue


def _homography_matcher():
    from .gt_matcher import HomographyMatcher

    return HomographyMatcher


def _line_homography_matcher():
    from .line_gt import LineHomographyMatcher

    return LineHomographyMatcher


def _depth_matcher():
    from .depth_matcher import DepthMatcher

    return DepthMatcher


def _line_depth_matcher():
    from .line_gt import LineDepthMatcher

    return LineDepthMatcher


def _nn_matcher():
    from .nn_matcher import NearestNeighborMatcher

    return NearestNeighborMatcher


def _aliked():
    from .aliked import ALIKED

    return ALIKED


def _gluestick():
    from .gluestick import GlueStick

    return GlueStick


def _wireframe():
    from .wireframe import WireframeExtractor

    return WireframeExtractor


def _lsd():
    from .wireframe import LSD

    return LSD


_LAZY = (_superpoint, _superpoint_open, _aliked, _superglue, _gluestick, _homography_matcher, _line_homography_matcher,
         _depth_matcher, _line_depth_matcher, _nn_matcher, _wireframe, _lsd)

_REGISTRY = {
    "lightglue": LightGlue,
    "matchers.lightglue": LightGlue,
    "lightglue_pretrained_MINE": LightGluePreTrainedMINE,
    "matchers.lightglue_pretrained_MINE": LightGluePreTrainedMINE,
    "two_view_pipeline": TwoViewPipeline,
    # the extractor (gluefactory_nonfree/superpoint.py), resolved lazily
    "gluefactory_nonfree.superpoint": _superpoint,
    "extractors.superpoint": _superpoint,
    "superpoint": _superpoint,
    # the open (MIT) SuperPoint (models/extractors/superpoint_open.py), resolved lazily
    "extractors.superpoint_open": _superpoint_open,
    "superpoint_open": _superpoint_open,
    # ALIKED (models/extractors/aliked.py), resolved lazily
    "extractors.aliked": _aliked,
    "aliked": _aliked,
    # the SuperGlue matcher (gluefactory_nonfree/superglue.py), resolved lazily
    "gluefactory_nonfree.superglue": _superglue,
    "superglue": _superglue,
    # the GlueStick point-and-line matcher (models/matchers/gluestick.py), resolved lazily
    "matchers.gluestick": _gluestick,
    "gluestick": _gluestick,
    # the wireframe extractor in front of GlueStick (models/lines/wireframe.py) and the LSD host
    # wrapper (models/lines/lsd.py), resolved lazily
    "lines.wireframe": _wireframe,
    "wireframe": _wireframe,
    "gluefactory.models.lines.wireframe": _wireframe,
    "lines.lsd": _lsd,
    "gluefactory.models.lines.lsd": _lsd,
    # the homography ground truth (matchers/homography_matcher.py), resolved lazily
    "matchers.homography_matcher": _homography_matcher,
    "homography_matcher": _homography_matcher,
    # the same with line ground truth (use_lines, which the two names above refuse), resolved lazily
    "matchers.line_homography_matcher": _line_homography_matcher,
    "line_homography_matcher": _line_homography_matcher,
    # the pose-and-depth ground truth (matchers/depth_matcher.py), resolved lazily
    "matchers.depth_matcher": _depth_matcher,
    "depth_matcher": _depth_matcher,
    # the same with line ground truth (use_lines, which the two names above refuse), resolved lazily
    "matchers.line_depth_matcher": _line_depth_matcher,
    "line_depth_matcher": _line_depth_matcher,
    # the nearest-neighbour baseline (matchers/nearest_neighbor_matcher.py), resolved lazily
    "matchers.nearest_neighbor_matcher": _nn_matcher,
    "nearest_neighbor_matcher": _nn_matcher,
}


def register_model(name, cls):
    """Make ``cls`` resolvable by :func:`get_model` (extractors, filters, solvers, ground truth)."""
    _REGISTRY[name] = cls


def get_model(name):
    """models/__init__.py:7-30: the name as given, or with the ``matchers.`` / ``extractors.``
    prefix the reference also tries (backward compatibility), or with ``lines.``."""
    for path in (name, f"matchers.{name}", f"extractors.{name}", f"lines.{name}"):
        if path in _REGISTRY:
            obj = _REGISTRY[path]
            return obj() if obj in _LAZY else obj
    paths = [name, f"gluefactory.models.{name}", f"gluefactory.models.extractors.{name}",
             f"gluefactory.models.matchers.{name}", f"gluefactory.models.lines.{name}"]
    raise RuntimeError(f'Model {name} not found in any of [{" ".join(paths)}]')
