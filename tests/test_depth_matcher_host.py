"""Host side of the pose-and-depth ground truth (lightglue_amd.depth_matcher): registry names, the
reference's configuration, the Camera / Pose holders, duck-typed camera and pose inputs, the argument
checks of the two C entries and the pipeline picking up the ``gt_*`` keys -- no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import gt_depth_ref as R
import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.pipeline import BaseModel, TwoViewPipeline, get_model, register_model


def test_depth_matcher_resolves_by_both_names_with_the_reference_configuration():
    from lightglue_amd.depth_matcher import DepthMatcher

    assert get_model("matchers.depth_matcher") is DepthMatcher
    assert get_model("depth_matcher") is DepthMatcher
    m = DepthMatcher({})
    # depth_matcher.py:11-24 plus the one extra key
    assert {k: m.conf[k] for k in DepthMatcher.default_conf} == {
        "use_points": True, "th_positive": 3.0, "th_negative": 5.0, "th_epi": None, "th_consistency": None,
        "use_lines": False, "n_line_sampled_pts": 50, "line_perp_dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.5,
        "reward": True}
    assert list(DepthMatcher.default_conf)[:-1] == [
        "use_points", "th_positive", "th_negative", "th_epi", "th_consistency", "use_lines", "n_line_sampled_pts",
        "line_perp_dist_th", "overlap_th", "min_visibility_th"]
    assert m.required_data_keys == ["view0", "view1", "T_0to1", "T_1to0", "keypoints0", "keypoints1"]
    assert DepthMatcher({"use_points": False}).required_data_keys == ["view0", "view1", "T_0to1", "T_1to0"]
    assert DepthMatcher.required_data_keys == ["view0", "view1", "T_0to1", "T_1to0"]  # the class list is not grown
    with pytest.raises(NotImplementedError):
        m.loss({}, {})
    pipe = TwoViewPipeline({"ground_truth": {"name": "matchers.depth_matcher", "th_epi": 1.0, "th_consistency": 4.0}})
    assert isinstance(pipe.ground_truth, DepthMatcher)
    assert pipe.ground_truth.conf.th_epi == 1.0 and pipe.ground_truth.conf.th_consistency == 4.0


def test_depth_matcher_use_lines_raises_at_construction():
    with pytest.raises(NotImplementedError, match="use_lines"):
        get_model("depth_matcher")({"use_lines": True})


def test_depth_matcher_rejects_cpu_inputs_and_missing_keys():
    m = get_model("depth_matcher")({})
    cam, T = torch.tensor([8.0, 8.0, 4.0, 4.0, 4.0, 4.0]), torch.cat([torch.eye(3).flatten(), torch.zeros(3)])
    data = {"view0": {"camera": cam, "depth": torch.ones(1, 8, 8)}, "view1": {"camera": cam, "depth": torch.ones(1, 8, 8)},
            "T_0to1": T, "T_1to0": T, "keypoints0": torch.zeros(1, 4, 2), "keypoints1": torch.zeros(1, 4, 2)}
    with pytest.raises(RuntimeError, match="HIP"):
        m(data)
    with pytest.raises(AssertionError, match="T_1to0"):
        m({k: v for k, v in data.items() if k != "T_1to0"})


def test_holders_agree_with_the_restatement():
    from lightglue_amd.depth_matcher import Camera, Pose

    g = torch.Generator().manual_seed(3)
    A = torch.linalg.qr(torch.randn(4, 3, 3, generator=g, dtype=torch.float64)).Q
    t = torch.randn(4, 3, generator=g, dtype=torch.float64)
    P = Pose.from_Rt(A, t)
    assert P._data.shape == (4, 12) and tuple(P.shape) == (4,)
    assert torch.equal(P._data, R.pose_from_Rt(A, t))
    assert torch.equal(P.inv()._data, R.pose_inv(P._data))
    assert torch.equal(P.R, A) and torch.equal(P.t, t)
    T = torch.eye(4, dtype=torch.float64).repeat(4, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = A, t
    assert torch.equal(Pose.from_4x4mat(T)._data, P._data)
    torch.testing.assert_close(P.inv().inv()._data, P._data)
    assert P.to(torch.float32)._data.dtype == torch.float32 and isinstance(P.to(torch.float32), Pose)
    assert torch.equal(P[1]._data, P._data[1])
    K = torch.tensor([[[300.0, 0.0, 161.5], [0.0, 310.0, 117.5], [0.0, 0.0, 1.0]]])
    C = Camera.from_calibration_matrix(K)
    assert C._data.tolist() == [[323.0, 235.0, 300.0, 310.0, 161.5, 117.5]]
    assert torch.equal(R.calibration_matrix(C._data), K)
    assert isinstance(C.to(torch.float64), Camera) and C.to(torch.float64)._data.dtype == torch.float64
    with pytest.raises(AssertionError):
        Camera(torch.zeros(1, 7))
    with pytest.raises(AssertionError):
        Pose(torch.zeros(1, 16))


def test_duck_typed_cameras_and_poses_become_rows():
    from lightglue_amd.depth_matcher import Camera, Pose, _rows

    dev = torch.device("cpu")
    cam = torch.arange(16, dtype=torch.float64).reshape(2, 8)

    class Wrapped:  # what the reference's Camera / Pose look like from outside
        def __init__(self, d):
            self._data = d

    for x in (cam, Camera(cam), Wrapped(cam)):
        r = _rows(x, 2, dev, "camera")
        assert r.dtype == torch.float32 and r.is_contiguous() and torch.equal(r, cam.float())
    assert torch.equal(_rows(cam[0], 2, dev, "camera"), cam[:1].float().expand(2, 8))  # an unbatched row broadcasts
    T = torch.eye(4).repeat(2, 1, 1)
    T[:, :3, 3] = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    rows = Pose.from_4x4mat(T)._data
    for x in (rows, Pose(rows), Wrapped(rows), T):
        assert torch.equal(_rows(x, 2, dev, "pose"), rows)
    assert torch.equal(_rows(T[1], 2, dev, "pose"), rows[1:].expand(2, 12))
    assert torch.equal(_rows(rows[1], 2, dev, "pose"), rows[1:].expand(2, 12))
    with pytest.raises(ValueError):
        _rows(torch.zeros(2, 7), 2, dev, "camera")
    with pytest.raises(ValueError):
        _rows(torch.zeros(3, 12), 2, dev, "pose")
    with pytest.raises(TypeError):
        _rows([1.0] * 6, 2, dev, "camera")


def test_gt_depth_c_entries_check_their_arguments():
    lib = _lib.load()
    assert {"lg_gt_depth_workspace_bytes", "lg_gt_matches_from_pose_depth"} <= set(_lib.EXPORTED_SYMBOLS)
    nb = ctypes.c_size_t()
    assert lib.lg_gt_depth_workspace_bytes(2, 300, 257, ctypes.byref(nb)) == _lib.LG_OK
    assert 34 * 2 * (300 + 257) <= nb.value < 34 * 2 * (300 + 257) + 14 * 256  # O(B (M + N)): nothing of size M * N
    assert lib.lg_gt_depth_workspace_bytes(2, 300, 257, None) == _lib.LG_E_INVALID and b"null" in lib.lg_last_error()
    assert lib.lg_gt_depth_workspace_bytes(2, -1, 257, ctypes.byref(nb)) == _lib.LG_E_INVALID
    assert b"negative" in lib.lg_last_error()

    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(128)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)
    nan = float("nan")
    # kp0 kp1 depth0 depth1 cam0 cam1 T01 T10 | dk0 dk1 valid0 valid1 assignment reward m0 m1 s0 s1 p01 p10 vis0 vis1
    NULLABLE = {2, 3, 10, 11, 13}

    def call(B=1, M=4, N=4, ptrs=None, nd=0, hw=(8, 8, 8, 8), epi=nan, cc=nan, ws=p, ws_bytes=1 << 30):
        a = [p] * 22 if ptrs is None else ptrs
        return lib.lg_gt_matches_from_pose_depth(a[0], a[1], a[2], hw[0], hw[1], a[3], hw[2], hw[3], a[4], a[5], nd, a[6], a[7],
                                                 B, M, N, 3.0, 5.0, epi, cc, *a[8:], ws, ws_bytes, None)

    def with_(**at):
        ptrs = [p] * 22
        for k, v in at.items():
            ptrs[int(k[1:])] = v
        return ptrs

    for k in sorted(set(range(22)) - NULLABLE):
        assert call(ptrs=with_(**{f"i{k}": None})) == _lib.LG_E_INVALID, k
        assert b"null" in lib.lg_last_error()
    assert call(M=-4) == _lib.LG_E_INVALID and b"negative" in lib.lg_last_error()
    assert call(hw=(8, -8, 8, 8)) == _lib.LG_E_INVALID and b"negative" in lib.lg_last_error()
    assert call(M=70000, N=70000) == _lib.LG_E_INVALID and b"2^31" in lib.lg_last_error()
    assert call(ws_bytes=8) == _lib.LG_E_INVALID and b"workspace" in lib.lg_last_error()
    assert call(ws=None) == _lib.LG_E_INVALID and b"workspace" in lib.lg_last_error()
    assert call(ws=ctypes.c_void_p(base + 8)) == _lib.LG_E_INVALID and b"aligned" in lib.lg_last_error()
    for nd in (1, 3, 5, -2, 6):
        assert call(nd=nd) == _lib.LG_E_INVALID and b"n_dist" in lib.lg_last_error()
    for nd in (0, 2, 4):  # the count itself is fine: the next check (the short workspace) answers
        assert call(nd=nd, ws_bytes=8) == _lib.LG_E_INVALID and b"workspace" in lib.lg_last_error()
    off4, off2 = ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    assert call(ptrs=with_(i0=off4)) == _lib.LG_E_INVALID and b"8-byte" in lib.lg_last_error()  # keypoints
    assert call(ptrs=with_(i19=off4)) == _lib.LG_E_INVALID and b"8-byte" in lib.lg_last_error()  # projections
    assert call(ptrs=with_(i14=off4)) == _lib.LG_E_INVALID and b"misaligned" in lib.lg_last_error()  # matches0
    assert call(ptrs=with_(i4=off2)) == _lib.LG_E_INVALID and b"misaligned" in lib.lg_last_error()  # camera rows
    assert call(ptrs=with_(i2=off2)) == _lib.LG_E_INVALID and b"misaligned" in lib.lg_last_error()  # a depth map
    assert call(ptrs=with_(i13=off2)) == _lib.LG_E_INVALID and b"reward" in lib.lg_last_error()
    # a depth map where one is needed: sampling (no precomputed depths), or th_consistency
    assert call(ptrs=with_(i2=None, i10=None, i11=None)) == _lib.LG_E_INVALID and b"depth map" in lib.lg_last_error()
    assert call(ptrs=with_(i3=None, i10=None, i11=None)) == _lib.LG_E_INVALID and b"depth map" in lib.lg_last_error()
    assert call(ptrs=with_(i10=None, i11=None), hw=(8, 8, 0, 8)) == _lib.LG_E_INVALID and b"depth map" in lib.lg_last_error()
    assert call(ptrs=with_(i2=None, i3=None), cc=1.0) == _lib.LG_E_INVALID and b"depth map" in lib.lg_last_error()
    assert call(ptrs=with_(i10=None)) == _lib.LG_E_INVALID and b"both" in lib.lg_last_error()  # one valid array alone
    # precomputed depths need no maps: accepted up to the next check
    assert call(ptrs=with_(i2=None, i3=None), hw=(0, 0, 0, 0), ws_bytes=8) == _lib.LG_E_INVALID
    assert b"workspace" in lib.lg_last_error()
    # an empty side: OK, nothing launched (no workspace needed either)
    for B, M, N in ((0, 4, 4), (3, 0, 7), (3, 7, 0)):
        assert call(B, M, N, ptrs=with_(i10=None, i11=None, i13=None), ws=None, ws_bytes=0) == _lib.LG_OK


def test_abi_version_is_unchanged():
    assert _lib.load().lg_abi_version() == 12


class _Matcher(BaseModel):
    def _init(self, conf):
        pass

    def _forward(self, data):
        return {"score": data["keypoints0"].sum()}

    def loss(self, pred, data):
        assert "gt_matches0" in data and "view0" in data
        return {"total": pred["score"] + pred["gt_matches0"].sum() + pred["gt_visible0"].sum()}, {}


class _StandInDepthGT(BaseModel):
    """The depth matcher's interface (required keys, the twelve outputs) with the restatement inside."""
    required_data_keys = ["view0", "view1", "T_0to1", "T_1to0", "keypoints0", "keypoints1"]

    def _init(self, conf):
        pass

    def _forward(self, data):
        assert "score" in data, "the ground truth sees the predictions"
        return R.gt_matches_from_pose_depth(data["keypoints0"], data["keypoints1"], data)

    def loss(self, pred, data):
        raise NotImplementedError


register_model("test.depth_matcher_user", _Matcher)
register_model("test.depth_gt", _StandInDepthGT)


def test_pipeline_picks_up_the_gt_keys():
    from lightglue_amd.depth_matcher import Camera, Pose

    g = R.plane_scene(5, 1, 24, 20, width=64, height=48, holes=2, hole_max=(12, 10))
    data = R.feed_of(g)
    data["view0"]["camera"], data["view1"]["camera"] = Camera(data["view0"]["camera"]), Camera(data["view1"]["camera"])
    data["T_0to1"], data["T_1to0"] = Pose(data["T_0to1"]), Pose(data["T_1to0"])
    pipe = TwoViewPipeline({"matcher": {"name": "test.depth_matcher_user"}, "ground_truth": {"name": "test.depth_gt"}})
    pred = pipe(data)
    assert not any(k.startswith("gt_") for k in pred)
    losses, _ = pipe.loss(pred, data)
    assert sorted(k for k in pred if k.startswith("gt_")) == sorted("gt_" + k for k in R.KEYS)
    want = pred["score"] + pred["gt_matches0"].sum() + pred["gt_visible0"].sum()
    assert torch.equal(losses["total"], want)
    assert np.isin(pred["gt_matches0"].numpy(), np.arange(-2, 20)).all()
