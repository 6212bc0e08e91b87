"""Host side of the pose-and-depth line ground truth (lightglue_amd.line_gt): the registry names and the
reference's configuration, the two older matchers still refusing ``use_lines``, CPU inputs refused, the
argument checks of the new C entries, and the integer thresholds derived on the host against the torch
expressions the reference evaluates -- no GPU needed."""
import ctypes

import pytest
import torch

import line_gt_depth_ref as R
import line_gt_ref as LR
import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.pipeline import TwoViewPipeline, get_model

ENTRIES = ["lg_gt_line_depth_thresholds", "lg_gt_line_counts_pose_depth_workspace_bytes", "lg_gt_line_counts_pose_depth",
           "lg_gt_line_labels_visibility_workspace_bytes", "lg_gt_line_labels_visibility"]


def test_line_depth_matcher_resolves_by_both_names_with_the_reference_configuration():
    from lightglue_amd.depth_matcher import DepthMatcher
    from lightglue_amd.line_gt import LineDepthMatcher

    assert get_model("matchers.line_depth_matcher") is LineDepthMatcher
    assert get_model("line_depth_matcher") is LineDepthMatcher
    assert issubclass(LineDepthMatcher, DepthMatcher)
    m = LineDepthMatcher({})
    # depth_matcher.py:11-24 with use_lines on, plus the existing extra key
    assert {k: m.conf[k] for k in LineDepthMatcher.default_conf} == {
        "use_points": True, "th_positive": 3.0, "th_negative": 5.0, "th_epi": None, "th_consistency": None,
        "use_lines": True, "n_line_sampled_pts": 50, "line_perp_dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.5,
        "reward": True}
    assert list(LineDepthMatcher.default_conf) == list(DepthMatcher.default_conf)
    base = ["view0", "view1", "T_0to1", "T_1to0"]
    lines = ["lines0", "lines1", "valid_lines0", "valid_lines1"]
    assert m.required_data_keys == base + ["keypoints0", "keypoints1"] + lines  # depth_matcher.py:28-38
    assert LineDepthMatcher({"use_points": False}).required_data_keys == base + lines
    assert LineDepthMatcher({"use_lines": False}).required_data_keys == base + ["keypoints0", "keypoints1"]
    assert LineDepthMatcher.required_data_keys == base  # the class list is not grown
    with pytest.raises(NotImplementedError):
        m.loss({}, {})
    pipe = TwoViewPipeline({"ground_truth": {"name": "matchers.line_depth_matcher", "overlap_th": 0.3}})
    assert isinstance(pipe.ground_truth, LineDepthMatcher) and pipe.ground_truth.conf.overlap_th == 0.3


def test_the_older_matchers_still_refuse_use_lines():
    with pytest.raises(NotImplementedError, match="use_lines"):
        get_model("depth_matcher")({"use_lines": True})
    with pytest.raises(NotImplementedError, match="line_depth_matcher"):
        get_model("matchers.depth_matcher")({"use_lines": True})
    with pytest.raises(NotImplementedError):
        get_model("homography_matcher")({"use_lines": True})


def test_cpu_inputs_are_rejected():
    from lightglue_amd import line_gt

    lines, valid = torch.zeros(1, 4, 4), torch.ones(1, 4, dtype=torch.bool)
    view = {"camera": torch.tensor([[8.0, 8, 8, 8, 4, 4]]), "depth": torch.ones(1, 8, 8), "image": torch.zeros(1, 1, 8, 8)}
    T = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]])
    data = {"view0": view, "view1": view, "T_0to1": T, "T_1to0": T}
    with pytest.raises(RuntimeError, match="HIP"):
        line_gt.gt_line_matches_from_pose_depth(lines, lines, valid, valid, data)
    with pytest.raises(RuntimeError, match="HIP"):
        line_gt.close_point_counts_from_pose_depth(lines, lines, data)
    cnt = torch.zeros(1, 4, 4, dtype=torch.uint8)
    vis = torch.zeros(1, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP"):
        line_gt.line_labels_from_visibility_counts(cnt, cnt, ~valid, ~valid, ~valid, ~valid, vis, vis, valid, valid, 50, 0.2)
    m = get_model("line_depth_matcher")({"use_points": False})
    full = {**data, "lines0": lines, "lines1": lines, "valid_lines0": valid, "valid_lines1": valid}
    with pytest.raises(RuntimeError, match="HIP"):
        m(full)
    with pytest.raises(AssertionError, match="valid_lines1"):
        m({k: v for k, v in full.items() if k != "valid_lines1"})
    with pytest.raises(ValueError, match="npts"):
        line_gt.line_depth_thresholds(256, 0.5, 0.2)
    with pytest.raises(ValueError, match="npts"):
        line_gt.line_depth_thresholds(1, 0.5, 0.2)


def test_c_entries_check_their_arguments():
    lib = _lib.load()
    assert set(ENTRIES) <= set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, s) for s in ENTRIES)
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION  # additive
    nb = ctypes.c_size_t()
    INV, OK = _lib.LG_E_INVALID, _lib.LG_OK

    def err(word):
        return word in lib.lg_last_error()

    # the workspace companions; nothing of size B * n0 * n1 * npts is ever allocated
    B, n0, n1, npts = 32, 250, 250, 50
    assert lib.lg_gt_line_counts_pose_depth_workspace_bytes(B, n0, n1, npts, ctypes.byref(nb)) == OK
    per_line = 8 * npts + 32
    assert per_line * B * (n0 + n1) <= nb.value < per_line * B * (n0 + n1) + 4 * 256
    assert nb.value < B * n0 * n1 * npts
    assert lib.lg_gt_line_counts_pose_depth_workspace_bytes(1, 4, 4, 50, None) == INV and err(b"null")
    assert lib.lg_gt_line_counts_pose_depth_workspace_bytes(1, -4, 4, 50, ctypes.byref(nb)) == INV and err(b"negative")
    for bad in (1, 0, -3, 256):
        assert lib.lg_gt_line_counts_pose_depth_workspace_bytes(1, 4, 4, bad, ctypes.byref(nb)) == INV and err(b"npts")
    assert lib.lg_gt_line_labels_visibility_workspace_bytes(2, 250, 250, ctypes.byref(nb)) == OK
    assert nb.value >= 2 * 250 * 250 * 8  # the fp64 cost lives here
    assert lib.lg_gt_line_labels_visibility_workspace_bytes(2, 250, 250, None) == INV and err(b"null")
    assert lib.lg_gt_line_labels_visibility_workspace_bytes(2, 250, -1, ctypes.byref(nb)) == INV and err(b"negative")

    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(128)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, off4, off8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 8)
    big = 1 << 40

    def counts(ptrs=None, B=2, n0=5, n1=6, maps=(8, 8, 8, 8), images=(8, 8, 8, 8), nd=0, npts=50, ws=p, ws_bytes=big):
        a = list(ptrs or [p] * 16)  # lines0, lines1, depth0, depth1, cam0, cam1, T01, T10, then the eight outputs
        return lib.lg_gt_line_counts_pose_depth(a[0], a[1], a[2], maps[0], maps[1], a[3], maps[2], maps[3], *images, a[4], a[5],
                                                nd, a[6], a[7], B, n0, n1, npts, 5.0, 0.5, *a[8:], ws, ws_bytes, None)

    def labels(ptrs=None, B=2, n0=5, n1=6, npts=50, ws=p, ws_bytes=big):
        a = list(ptrs or [p] * 13)
        return lib.lg_gt_line_labels_visibility(*a[:10], B, n0, n1, npts, 0.2, *a[10:], ws, ws_bytes, None)

    def with_(n, k, v):
        a = [p] * n
        a[k] = v
        return a

    for call, n in ((counts, 16), (labels, 13)):
        for k in range(n):
            assert call(ptrs=with_(n, k, None)) == INV and err(b"null"), (call.__name__, k)
        assert call(B=-1) == INV and err(b"negative")
        assert call(n0=-5) == INV and err(b"negative")
        assert call(n1=-6) == INV and err(b"negative")
        for shape in ((0, 5, 6), (2, 0, 6), (2, 5, 0)):  # an empty side: OK, nothing launched, no workspace needed
            assert call(None, *shape, ws=None, ws_bytes=0) == OK
        for bad in (1, 256, -1):
            assert call(npts=bad) == INV and err(b"npts")
        assert call(npts=2, ws_bytes=8) == INV and err(b"workspace")  # 2 and 255 pass on to the next check
        assert call(npts=255, ws_bytes=8) == INV and err(b"workspace")
        assert call(n0=70000, n1=70000) == INV and err(b"2^31")
        assert call(ws=None) == INV and err(b"workspace")
        assert call(ws=off8) == INV and err(b"16-byte")
    assert counts(maps=(8, 8, -8, 8)) == INV and err(b"negative")
    assert counts(images=(8, -8, 8, 8)) == INV and err(b"negative")
    assert counts(maps=(8, 0, 8, 8)) == INV and err(b"empty")
    assert counts(maps=(65536, 65536, 8, 8)) == INV and err(b"2^31")
    for nd in (1, 3, 5, -2):
        assert counts(nd=nd) == INV and err(b"n_dist")
    for k in range(8):  # every fp32 input
        assert counts(ptrs=with_(16, k, ctypes.c_void_p(base + 2))) == INV and err(b"4-byte"), k
    assert labels(ptrs=with_(13, 11, off4)) == INV and err(b"8-byte")
    assert labels(ptrs=with_(13, 12, off4)) == INV and err(b"8-byte")
    tab = (ctypes.c_int32 * 256)()
    a, b = ctypes.c_int32(), ctypes.c_int32()
    assert lib.lg_gt_line_depth_thresholds(50, 0.5, 0.2, None, ctypes.byref(a), ctypes.byref(b)) == INV and err(b"null")
    assert lib.lg_gt_line_depth_thresholds(50, 0.5, 0.2, tab, None, ctypes.byref(b)) == INV and err(b"null")
    assert lib.lg_gt_line_depth_thresholds(50, 0.5, 0.2, tab, ctypes.byref(a), None) == INV and err(b"null")
    assert lib.lg_gt_line_depth_thresholds(1, 0.5, 0.2, tab, ctypes.byref(a), ctypes.byref(b)) == INV and err(b"npts")
    assert lib.lg_gt_line_depth_thresholds(256, 0.5, 0.2, tab, ctypes.byref(a), ctypes.byref(b)) == INV and err(b"npts")


@pytest.mark.parametrize("npts", [2, 7, 50, 255])
@pytest.mark.parametrize("overlap_th, min_visibility_th", [(0.2, 0.5), (0.5, 0.2), (0.0, 0.0), (1.0, 1.0), (0.3, 0.8), (0.7, 0.1)])
def test_host_thresholds_equal_the_torch_expressions_for_every_count(npts, overlap_th, min_visibility_th):
    """``count > visible.float().sum(-1) * overlap_th`` (gt_generation.py:329-336), ``mean(out) >= 1 -
    min_visibility_th`` (:297) and ``mean(valid) < min_visibility_th`` (:345-347), for every count."""
    from lightglue_amd.line_gt import line_depth_thresholds

    table, out_min, valid_min = line_depth_thresholds(npts, min_visibility_th, overlap_th)
    assert table == R.min_close_table(npts, overlap_th)
    assert out_min == LR.min_out_count(npts, min_visibility_th)
    assert valid_min == R.min_valid_count(npts, min_visibility_th)
    counts = torch.arange(npts + 1)
    for v in (0, 1, npts // 2, npts):
        want = counts > torch.tensor(float(v)) * overlap_th  # an int64 tensor against an fp32 one
        assert torch.equal(counts >= table[v], want), v
    rows = (torch.arange(npts)[None] < counts[:, None]).float()  # row c holds c ones
    assert torch.equal(counts >= valid_min, ~(rows.mean(dim=-1) < min_visibility_th))
