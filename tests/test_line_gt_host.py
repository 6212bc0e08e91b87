"""Host side of the line ground truth (lightglue_amd.line_gt): the registry names and the reference's
configuration, the two older matchers still refusing ``use_lines``, CPU inputs refused, the argument
checks of the C entries, and the integer thresholds derived on the host against the torch expressions
the reference evaluates -- no GPU needed."""
import ctypes

import pytest
import torch

import line_gt_ref as R
import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.pipeline import TwoViewPipeline, get_model

ENTRIES = ["lg_gt_line_thresholds", "lg_gt_line_counts_workspace_bytes", "lg_gt_line_counts_homography",
           "lg_gt_line_labels_workspace_bytes", "lg_gt_line_labels", "lg_linear_sum_assignment_workspace_bytes",
           "lg_linear_sum_assignment"]


def test_line_homography_matcher_resolves_by_both_names_with_the_reference_configuration():
    from lightglue_amd.gt_matcher import HomographyMatcher
    from lightglue_amd.line_gt import LineHomographyMatcher

    assert get_model("matchers.line_homography_matcher") is LineHomographyMatcher
    assert get_model("line_homography_matcher") is LineHomographyMatcher
    assert issubclass(LineHomographyMatcher, HomographyMatcher)
    m = LineHomographyMatcher({})
    # homography_matcher.py:9-20 with use_lines on, plus the existing extra key
    assert {k: m.conf[k] for k in LineHomographyMatcher.default_conf} == {
        "use_points": True, "th_positive": 3.0, "th_negative": 3.0, "use_lines": True, "n_line_sampled_pts": 50,
        "line_perp_dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.5, "reward": True}
    assert list(LineHomographyMatcher.default_conf) == list(HomographyMatcher.default_conf)
    lines = ["lines0", "lines1", "valid_lines0", "valid_lines1"]
    assert m.required_data_keys == ["H_0to1", "keypoints0", "keypoints1"] + lines
    assert LineHomographyMatcher({"use_points": False}).required_data_keys == ["H_0to1"] + lines
    assert LineHomographyMatcher({"use_lines": False}).required_data_keys == ["H_0to1", "keypoints0", "keypoints1"]
    assert LineHomographyMatcher.required_data_keys == ["H_0to1"]  # the class list is not grown
    with pytest.raises(NotImplementedError):
        m.loss({}, {})
    pipe = TwoViewPipeline({"ground_truth": {"name": "matchers.line_homography_matcher", "overlap_th": 0.3}})
    assert isinstance(pipe.ground_truth, LineHomographyMatcher) and pipe.ground_truth.conf.overlap_th == 0.3


def test_the_older_matchers_still_refuse_use_lines():
    with pytest.raises(NotImplementedError):
        get_model("homography_matcher")({"use_lines": True})
    with pytest.raises(NotImplementedError):
        get_model("matchers.homography_matcher")({"use_lines": True})
    with pytest.raises(NotImplementedError, match="use_lines"):
        get_model("depth_matcher")({"use_lines": True})


def test_cpu_inputs_are_rejected():
    from lightglue_amd import line_gt

    lines, valid, H = torch.zeros(1, 4, 4), torch.ones(1, 4, dtype=torch.bool), torch.eye(3)
    with pytest.raises(RuntimeError, match="HIP"):
        line_gt.gt_line_matches_from_homography(lines, lines, valid, valid, (8, 8), (8, 8), H)
    with pytest.raises(RuntimeError, match="HIP"):
        line_gt.close_point_counts_from_homography(lines, lines, (8, 8), (8, 8), H)
    cnt = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP"):
        line_gt.line_labels_from_counts(cnt, cnt, ~valid, ~valid, valid, valid, 50, 0.2)
    with pytest.raises(RuntimeError, match="HIP"):
        line_gt.linear_sum_assignment(torch.zeros(3, 3))
    m = get_model("line_homography_matcher")({"use_points": False})
    data = {"H_0to1": H, "lines0": lines, "lines1": lines, "valid_lines0": valid, "valid_lines1": valid,
            "view0": {"image": torch.zeros(1, 1, 8, 8)}, "view1": {"image": torch.zeros(1, 1, 8, 8)}}
    with pytest.raises(RuntimeError, match="HIP"):
        m(data)
    with pytest.raises(AssertionError, match="valid_lines1"):
        m({k: v for k, v in data.items() if k != "valid_lines1"})
    with pytest.raises(ValueError, match="npts"):
        line_gt.line_count_thresholds(256, 0.5, 0.2)


def test_c_entries_check_their_arguments():
    lib = _lib.load()
    assert set(ENTRIES) <= set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, s) for s in ENTRIES)
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION  # additive
    nb = ctypes.c_size_t()
    INV, OK = _lib.LG_E_INVALID, _lib.LG_OK

    def err(word):
        return word in lib.lg_last_error()

    # the workspace companions
    assert lib.lg_gt_line_counts_workspace_bytes(32, 250, 250, 50, ctypes.byref(nb)) == OK
    per_line = 8 * 50 + 32
    assert per_line * 32 * 500 <= nb.value < per_line * 32 * 500 + 4 * 256  # nothing of size n0 * n1
    assert lib.lg_gt_line_counts_workspace_bytes(1, 4, 4, 50, None) == INV and err(b"null")
    assert lib.lg_gt_line_counts_workspace_bytes(1, -4, 4, 50, ctypes.byref(nb)) == INV and err(b"negative")
    for npts in (1, 0, -3, 256):
        assert lib.lg_gt_line_counts_workspace_bytes(1, 4, 4, npts, ctypes.byref(nb)) == INV and err(b"npts")
    assert lib.lg_gt_line_labels_workspace_bytes(2, 250, 250, ctypes.byref(nb)) == OK
    assert nb.value >= 2 * 250 * 250 * 8  # the fp64 cost lives here
    assert lib.lg_gt_line_labels_workspace_bytes(2, 250, 250, None) == INV and err(b"null")
    assert lib.lg_gt_line_labels_workspace_bytes(2, 250, -1, ctypes.byref(nb)) == INV and err(b"negative")
    assert lib.lg_linear_sum_assignment_workspace_bytes(4, 300, 257, ctypes.byref(nb)) == OK and nb.value == 0  # LDS
    assert lib.lg_linear_sum_assignment_workspace_bytes(4, 8, 2400, ctypes.byref(nb)) == OK
    assert nb.value >= 4 * (28 * 2400 + 12 * 8)  # too long for 64 KiB of LDS: the state moves to global memory
    assert lib.lg_linear_sum_assignment_workspace_bytes(4, 8, 8, None) == INV and err(b"null")
    assert lib.lg_linear_sum_assignment_workspace_bytes(-4, 8, 8, ctypes.byref(nb)) == INV and err(b"negative")

    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(128)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, off4, off8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 8)
    big = 1 << 40

    def counts(ptrs=None, B=2, n0=5, n1=6, hw=(8, 8, 8, 8), npts=50, ws=p, ws_bytes=big):
        a = list(ptrs or [p] * 7)
        return lib.lg_gt_line_counts_homography(a[0], a[1], a[2], B, n0, n1, *hw, npts, 5.0, 0.5, a[3], a[4], a[5], a[6], ws,
                                                ws_bytes, None)

    def labels(ptrs=None, B=2, n0=5, n1=6, npts=50, ws=p, ws_bytes=big):
        a = list(ptrs or [p] * 9)
        return lib.lg_gt_line_labels(*a[:6], B, n0, n1, npts, 0.2, *a[6:], ws, ws_bytes, None)

    def lsa(ptrs=None, B=2, nr=5, nc=6, ws=None, ws_bytes=0):
        a = list(ptrs or [p] * 3)
        return lib.lg_linear_sum_assignment(a[0], B, nr, nc, a[1], a[2], ws, ws_bytes, None)

    def with_(n, k, v):
        a = [p] * n
        a[k] = v
        return a

    for call, n in ((counts, 7), (labels, 9), (lsa, 3)):
        for k in range(n):
            assert call(ptrs=with_(n, k, None)) == INV and err(b"null"), (call.__name__, k)
        assert call(B=-1) == INV and err(b"negative")
        for shape in ((0, 5, 6), (2, 0, 6), (2, 5, 0)):  # an empty side: OK, nothing launched, no workspace needed
            assert call(None, *shape, ws=None, ws_bytes=0) == OK
    assert counts(n0=-5) == INV and err(b"negative")
    assert counts(hw=(8, 8, -8, 8)) == INV and err(b"negative")
    assert labels(n1=-6) == INV and err(b"negative")
    assert lsa(nc=-6) == INV and err(b"negative")
    for call in (counts, labels):
        for npts in (1, 256, -1):
            assert call(npts=npts) == INV and err(b"npts")
        assert call(npts=2, ws_bytes=8) == INV and err(b"workspace")  # 2 and 255 pass on to the next check
        assert call(npts=255, ws_bytes=8) == INV and err(b"workspace")
        assert call(n0=70000, n1=70000) == INV and err(b"2^31")
        assert call(ws=None) == INV and err(b"workspace")
        assert call(ws=off8) == INV and err(b"16-byte")
    assert lsa(nr=70000, nc=70000) == INV and err(b"2^31")
    assert lsa(nr=8, nc=2400) == INV and err(b"workspace")  # this shape needs one
    assert lsa(nr=2400, nc=8, ws=p, ws_bytes=8) == INV and err(b"workspace")
    assert lsa(nr=8, nc=2400, ws=off8, ws_bytes=big) == INV and err(b"16-byte")
    assert counts(ptrs=with_(7, 0, ctypes.c_void_p(base + 2))) == INV and err(b"4-byte")
    assert counts(ptrs=with_(7, 2, ctypes.c_void_p(base + 1))) == INV and err(b"4-byte")
    assert labels(ptrs=with_(9, 7, off4)) == INV and err(b"8-byte")
    assert labels(ptrs=with_(9, 8, off4)) == INV and err(b"8-byte")
    for k in range(3):
        assert lsa(ptrs=with_(3, k, off4)) == INV and err(b"misaligned")
    a, b = ctypes.c_int32(), ctypes.c_int32()
    assert lib.lg_gt_line_thresholds(50, 0.5, 0.2, None, ctypes.byref(b)) == INV and err(b"null")
    assert lib.lg_gt_line_thresholds(50, 0.5, 0.2, ctypes.byref(a), None) == INV and err(b"null")
    assert lib.lg_gt_line_thresholds(1, 0.5, 0.2, ctypes.byref(a), ctypes.byref(b)) == INV and err(b"npts")
    assert lib.lg_gt_line_thresholds(256, 0.5, 0.2, ctypes.byref(a), ctypes.byref(b)) == INV and err(b"npts")


@pytest.mark.parametrize("npts", [2, 7, 50, 64, 255])
@pytest.mark.parametrize("th", [0.2, 0.5, 0.8])
def test_host_thresholds_equal_the_torch_expressions_for_every_count(npts, th):
    """``mean(out) >= 1 - th`` over npts fp32 booleans and ``count > npts * th`` on an int64 count, as
    gt_generation.py:465 and :492 evaluate them, for every count 0..npts."""
    from lightglue_amd.line_gt import line_count_thresholds

    out_min, close_min = line_count_thresholds(npts, th, th)
    counts = torch.arange(npts + 1)
    rows = (torch.arange(npts)[None] < counts[:, None]).float()  # row c holds c ones
    want_out = rows.mean(dim=-1) >= (1 - th)
    want_close = counts > npts * th
    assert torch.equal(counts >= out_min, want_out)
    assert torch.equal(counts >= close_min, want_close)
    assert (out_min, close_min) == (R.min_out_count(npts, th), R.min_close_count(npts, th))
