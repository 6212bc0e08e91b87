"""TwoViewPipeline.loss (reference models/two_view_pipeline.py:99-121), the homography ground-truth
component's registry names and the host checks of its two C entries -- no GPU needed: the
components here are small stand-ins registered through ``register_model``."""
import ctypes

import pytest
import torch

import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.pipeline import BaseModel, LightGluePreTrainedMINE, TwoViewPipeline, get_model, register_model


class _Matcher(BaseModel):
    default_conf = {"scale": 1.0}
    seen = None

    def _init(self, conf):
        pass

    def _forward(self, data):
        return {"score": data["view0"]["x"] * self.conf.scale}

    def loss(self, pred, data):
        type(self).seen = (dict(pred), dict(data))
        total = pred["score"] + pred["gt_label"]
        return {"total": total, "matcher_term": total * 2}, {"matcher_metric": pred["score"]}


class _Solver(BaseModel):
    def _init(self, conf):
        pass

    def _forward(self, data):
        return {"solved": data["score"] + 1}

    def loss(self, pred, data):
        return {"total": pred["solved"] * 10, "solver_term": pred["solved"]}, {"solver_metric": pred["solved"]}


class _NoLoss(BaseModel):
    def _init(self, conf):
        pass

    def _forward(self, data):
        return {"filtered": data["score"]}

    def loss(self, pred, data):
        raise NotImplementedError


class _DictLoss(_Solver):
    """A component whose loss returns the bare dict of losses (the reference's SuperGlue.loss)."""

    def loss(self, pred, data):
        return {"total": pred["solved"] * 100, "dict_term": pred["solved"]}


class _GT(BaseModel):
    calls = 0

    def _init(self, conf):
        pass

    def _forward(self, data):
        type(self).calls += 1
        assert "score" in data, "the ground truth sees the predictions"
        return {"label": data["view1"]["x"] * 3}

    def loss(self, pred, data):
        raise NotImplementedError


for _n, _c in (("test.matcher", _Matcher), ("test.solver", _Solver), ("test.noloss", _NoLoss), ("test.gt", _GT),
               ("test.dictloss", _DictLoss)):
    register_model(_n, _c)


def _data():
    return {"view0": {"x": torch.tensor([1.0, 2.0])}, "view1": {"x": torch.tensor([0.5, 0.25])}}


def _pipe(**over):
    conf = {"matcher": {"name": "test.matcher"}, "filter": {"name": "test.noloss"}, "solver": {"name": "test.solver"},
            "ground_truth": {"name": "test.gt"}}
    for k, v in over.items():
        conf[k] = {**conf.get(k, {}), **v} if isinstance(v, dict) else v
    return TwoViewPipeline(conf)


def test_total_is_the_sum_of_component_totals_and_notimplemented_is_skipped():
    pipe, data = _pipe(), _data()
    _GT.calls = 0
    pred = pipe(data)
    assert _GT.calls == 0 and not any(k.startswith("gt_") for k in pred)  # not in forward
    losses, metrics = pipe.loss(pred, data)
    assert _GT.calls == 1
    torch.testing.assert_close(pred["gt_label"], data["view1"]["x"] * 3)  # gt_-prefixed, merged into pred
    m_total = pred["score"] + pred["gt_label"]
    s_total = pred["solved"] * 10
    torch.testing.assert_close(losses["total"], m_total + s_total, rtol=0, atol=0)
    torch.testing.assert_close(losses["matcher_term"], m_total * 2)
    torch.testing.assert_close(losses["solver_term"], pred["solved"])
    assert set(losses) == {"total", "matcher_term", "solver_term"}  # the filter and the ground truth raised
    assert set(metrics) == {"matcher_metric", "solver_metric"}
    # the component saw (pred, {**pred, **data})
    spred, sdata = _Matcher.seen
    assert "gt_label" in spred and "gt_label" in sdata and "view0" in sdata and "view0" not in spred


def test_apply_loss_false_is_honoured():
    pipe, data = _pipe(solver={"apply_loss": False}), _data()
    pred = pipe(data)
    losses, metrics = pipe.loss(pred, data)
    torch.testing.assert_close(losses["total"], pred["score"] + pred["gt_label"], rtol=0, atol=0)
    assert "solver_term" not in losses and "solver_metric" not in metrics


def test_run_gt_in_forward_moves_the_ground_truth():
    pipe, data = _pipe(run_gt_in_forward=True), _data()
    _GT.calls = 0
    pred = pipe(data)
    assert _GT.calls == 1 and "gt_label" in pred
    pipe.loss(pred, data)
    assert _GT.calls == 1  # not again in loss


def test_no_component_with_a_loss_gives_a_zero_total():
    pipe = TwoViewPipeline({"filter": {"name": "test.noloss"}})
    losses, metrics = pipe.loss({"score": torch.ones(1)}, _data())
    assert losses == {"total": 0} and metrics == {}


def test_a_bare_dict_of_losses_counts_with_no_metrics():
    pipe, data = _pipe(solver={"name": "test.dictloss"}), _data()
    pred = pipe(data)
    losses, metrics = pipe.loss(pred, data)
    torch.testing.assert_close(losses["total"], pred["score"] + pred["gt_label"] + pred["solved"] * 100, rtol=0, atol=0)
    assert "dict_term" in losses and set(metrics) == {"matcher_metric"}


def test_base_model_loss_is_a_plain_notimplemented():
    class _Bare(BaseModel):
        def _init(self, conf):
            pass

    with pytest.raises(NotImplementedError) as ei:
        _Bare({}).loss({}, {})
    assert "out of scope" not in str(ei.value)


def test_pretrained_wrapper_forwards_loss_to_its_net():
    w = LightGluePreTrainedMINE({"n_layers": 1})
    seen = {}
    w.net.loss = lambda pred, data: seen.setdefault("args", (pred, data)) and ("L", "M")
    assert w.loss({"p": 1}, {"d": 2}) == ("L", "M") and seen["args"] == ({"p": 1}, {"d": 2})


def test_homography_matcher_resolves_by_both_names():
    from lightglue_amd.gt_matcher import HomographyMatcher

    assert get_model("matchers.homography_matcher") is HomographyMatcher
    assert get_model("homography_matcher") is HomographyMatcher
    m = HomographyMatcher({})
    # the reference's defaults (homography_matcher.py:9-20) plus the one extra key
    assert {k: m.conf[k] for k in HomographyMatcher.default_conf} == {
        "use_points": True, "th_positive": 3.0, "th_negative": 3.0, "use_lines": False, "n_line_sampled_pts": 50,
        "line_perp_dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.5, "reward": True}
    assert m.required_data_keys == ["H_0to1", "keypoints0", "keypoints1"]
    with pytest.raises(NotImplementedError):
        m.loss({}, {})
    pipe = TwoViewPipeline({"ground_truth": {"name": "matchers.homography_matcher", "th_negative": 5.0}})
    assert isinstance(pipe.ground_truth, HomographyMatcher) and pipe.ground_truth.conf.th_negative == 5.0


def test_homography_matcher_use_lines_raises_at_construction():
    with pytest.raises(NotImplementedError):
        get_model("homography_matcher")({"use_lines": True})


def test_homography_matcher_rejects_cpu_inputs():
    m = get_model("homography_matcher")({})
    with pytest.raises(RuntimeError, match="HIP"):
        m({"H_0to1": torch.eye(3), "keypoints0": torch.zeros(1, 4, 2), "keypoints1": torch.zeros(1, 4, 2)})


def test_gt_c_entries_check_their_arguments():
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.lg_gt_homography_workspace_bytes(2, 300, 257, ctypes.byref(nb)) == _lib.LG_OK
    assert nb.value >= 12 * 2 * (300 + 257)  # three 4-byte statistics per keypoint
    assert lib.lg_gt_homography_workspace_bytes(2, 300, 257, None) == _lib.LG_E_INVALID
    assert b"null" in lib.lg_last_error()
    assert lib.lg_gt_homography_workspace_bytes(2, -1, 257, ctypes.byref(nb)) == _lib.LG_E_INVALID
    assert b"negative" in lib.lg_last_error()

    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(B, M, N, ptrs=None, ws=p, ws_bytes=1 << 30):
        a = [p] * 11 if ptrs is None else ptrs
        return lib.lg_gt_matches_from_homography(a[0], a[1], a[2], B, M, N, 3.0, 3.0, *a[3:], ws, ws_bytes, None)

    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10):  # every pointer but the nullable reward (index 4)
        ptrs = [p] * 11
        ptrs[k] = None
        assert call(1, 4, 4, ptrs) == _lib.LG_E_INVALID, k
        assert b"null" in lib.lg_last_error()
    assert call(1, -4, 4) == _lib.LG_E_INVALID and b"negative" in lib.lg_last_error()
    assert call(1, 4, 4, ws_bytes=8) == _lib.LG_E_INVALID and b"workspace" in lib.lg_last_error()
    assert call(1, 4, 4, ws=None) == _lib.LG_E_INVALID and b"workspace" in lib.lg_last_error()
    assert call(1, 70000, 70000) == _lib.LG_E_INVALID and b"2^31" in lib.lg_last_error()
    # an empty side: OK, nothing launched (no workspace needed either)
    assert call(3, 0, 7, ws=None, ws_bytes=0) == _lib.LG_OK
    assert call(3, 7, 0, ws=None, ws_bytes=0) == _lib.LG_OK
