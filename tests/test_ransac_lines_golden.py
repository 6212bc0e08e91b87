"""Hybrid point-and-line robust homography estimation without a GPU: the float64 restatement (tests/
ransac_lines_ref.py) against the fixture it produced (tests/golden/ransac_lines/ransac_lines.npz) and
against the true homography, the library's exports and argument checks, and the Python layer's checks
(lightglue_amd.robust)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import ransac_lines_ref as ref
from lightglue_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ransac_lines_golden as gen  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ransac_lines", "ransac_lines.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def case(g, name):
    inp = {k: g[f"{name}/{k}"] for k in gen.INPUTS}
    for k in ("num_lines0", "num_lines1"):
        if f"{name}/{k}" in g:
            inp[k] = int(g[f"{name}/{k}"])
    opt = {"th": float(g[f"{name}/th"]), "max_iters": int(g[f"{name}/max_iters"]), "confidence": float(g[f"{name}/confidence"]),
           "seed": int(g[f"{name}/seed"]), "min_line_length": float(g[f"{name}/min_line_length"])}
    return inp, opt


@pytest.fixture(scope="module")
def restated(golden):
    """Every case through the restatement, once."""
    return {name: gen.restate(*case(golden, name), H_gt=golden[f"{name}/H_gt"].astype(np.float64)) for name in golden["cases"]}


def test_restatement_reproduces_the_fixture(golden, restated):
    assert tuple(golden["cases"]) == gen.CASES and len(gen.CASES) == 11
    for name, o in restated.items():
        np.testing.assert_array_equal(ref.info_row(o), golden[f"{name}/info"], err_msg=name)
        np.testing.assert_array_equal(o["inliers_slots"], golden[f"{name}/inliers"], err_msg=name)
        np.testing.assert_array_equal(o["line_inliers_slots"], golden[f"{name}/line_inliers"], err_msg=name)
        np.testing.assert_array_equal(o["m_kpts"], golden[f"{name}/m_kpts"], err_msg=name)
        np.testing.assert_array_equal(o["m_lines"], golden[f"{name}/m_lines"], err_msg=name)
        if o["success"]:
            # another LAPACK may move the eigenvector's last bits, and with them an fp32 rounding of the matrix
            np.testing.assert_allclose(o["H"], golden[f"{name}/H"], rtol=0, atol=2e-7 * np.abs(o["H"]).max(), err_msg=name)
            assert abs(o["H_error"] - float(golden[f"{name}/H_error"])) <= 1e-4 * o["H_error"] + 1e-7
            assert o["H_error"] < float(golden[f"{name}/th"]) and bool(golden[f"{name}/meant_to_succeed"]), name
        else:
            np.testing.assert_array_equal(o["H"], np.eye(3, dtype=np.float32))
            assert math.isinf(o["H_error"]) and not o["inliers_slots"].any() and not o["line_inliers_slots"].any()
            assert o["num_point_inliers"] == 0 == o["num_line_inliers"] and not bool(golden[f"{name}/meant_to_succeed"])
        assert o["margin"] >= float(golden["min_margin"]) == 1e-7, name
        assert o["margin"] == pytest.approx(float(golden[f"{name}/margin"]), rel=1e-3) or math.isinf(o["margin"])
    assert os.path.getsize(GOLDEN) < 200 * 1024


def test_cases_reach_the_branches_they_are_there_for(golden):
    g = golden
    info = {name: dict(zip(ref.INFO_FIELDS, g[f"{name}/info"].tolist())) for name in g["cases"]}
    both = lambda i: i["num_point_matches"] > 0 and i["num_line_matches"] > 0  # noqa: E731
    assert info["mixed"]["rounds"] == 1 and both(info["mixed"]) and info["mixed"]["num_line_inliers"] > 0
    assert info["rounds"]["rounds"] > 1 and both(info["rounds"]) and float(g["rounds/th"]) == 1.0
    assert info["cap300"]["rounds"] == 2 and info["cap300"]["best_t"] < 300 == int(g["cap300/max_iters"])
    assert info["cap300"]["valid_hypotheses"] < 300  # some samples were two points with two lines
    assert info["lines_only"]["num_point_matches"] == 0 and info["lines_only"]["success"] == 1 and g["lines_only/kpts0"].shape == (0, 2)
    assert info["points_only"]["num_line_matches"] == 0 and info["points_only"]["success"] == 1
    assert g["points_only/lines0"].shape == (0, 2, 2)
    assert info["three_two"] == {**info["three_two"], "success": 1, "num_point_matches": 3, "num_line_matches": 2,
                                 "num_point_inliers": 3, "num_line_inliers": 2}
    # K = 5: the valid samples are the two with all three points; the other three are two plus two
    assert 0 < info["three_two"]["valid_hypotheses"] < 256
    assert info["two_two"] == {**info["two_two"], "success": 0, "num_point_matches": 2, "num_line_matches": 2,
                               "valid_hypotheses": 0, "best_t": -1, "rounds": 2}
    assert info["k3"] == {**info["k3"], "success": 0, "rounds": 0} and info["k3"]["num_point_matches"] + info["k3"]["num_line_matches"] == 3
    assert info["empty"] == {**info["empty"], "success": 0, "num_point_matches": 0, "num_line_matches": 0, "rounds": 0}
    # pieces: the image-1 segments of the inlier lines are no images of the image-0 segments: their endpoints
    # are far from the mapped endpoints, and every second one is given end first
    inp, _ = case(g, "pieces")
    mapped = gen.warp(gen.H_GT, inp["lines0"].reshape(-1, 2).astype(np.float64)).reshape(-1, 2, 2)
    far = np.linalg.norm(mapped - inp["lines1"], axis=-1).max(1)[g["pieces/line_inliers"]]
    assert info["pieces"]["num_line_inliers"] >= 16 and np.median(far) > 10 * float(g["pieces/th"])
    # ragged: counts below the array sizes, wild indices, zero-length segments on either side, NaN padding
    lm, n0, n1 = g["ragged/line_matches0"], int(g["ragged/num_lines0"]), int(g["ragged/num_lines1"])
    l0, l1 = g["ragged/lines0"], g["ragged/lines1"]
    assert n0 < len(l0) and n1 < len(l1) and len(l0) != len(l1) and len(g["ragged/kpts0"]) != len(g["ragged/kpts1"])
    assert (lm[:n0] < -1).any() and (lm[:n0] >= len(l1)).any() and ((lm[:n0] >= n1) & (lm[:n0] < len(l1))).any()
    assert (lm[n0:] >= 0).all() and np.isnan(l0[n0:]).all() and np.isnan(l1[n1:]).all()
    zero0 = [i for i in range(n0) if 0 <= lm[i] < n1 and (l0[i, 0] == l0[i, 1]).all()]
    zero1 = [i for i in range(n0) if 0 <= lm[i] < n1 and (l1[lm[i], 0] == l1[lm[i], 1]).all()]
    assert len(zero0) == 1 == len(zero1) and zero0 != zero1
    assert info["ragged"]["num_line_matches"] == sum(0 <= m < n1 for m in lm[:n0]) - 2 == 28


def test_restatement_pieces(golden):
    """The parts the specification singles out, each on its own."""
    # the 2+2 configuration: rank 7 on exact data, whatever the points and lines
    g = golden
    inp, _ = case(g, "two_two")
    pts = np.concatenate([inp["kpts0"], inp["kpts1"]], 1).astype(np.float64)
    lns = np.concatenate([inp["lines0"].reshape(-1, 4), inp["lines1"].reshape(-1, 4)], 1).astype(np.float64)
    A = np.concatenate([ref.point_rows(pts).reshape(-1, 9), ref.line_rows(lns[:, :4], ref.segment_line(lns[:, 4:])).reshape(-1, 9)])
    sv = np.linalg.svd(A / np.abs(A).max(1, keepdims=True), compute_uv=False)
    assert sv[6] / sv[0] > 1e-6 > 1e-9 > sv[7] / sv[0]
    # the line of a segment does not depend on the order of its endpoints, bit for bit
    seg = lns[:, 4:]
    np.testing.assert_array_equal(ref.segment_line(seg), ref.segment_line(seg[:, [2, 3, 0, 1]]))
    abc = ref.segment_line(seg)
    assert np.allclose(abc[:, 0] ** 2 + abc[:, 1] ** 2, 1) and np.allclose((abc[:, :2] * seg[:, :2]).sum(1) + abc[:, 2], 0, atol=1e-9)
    # complete pivoting: the null vector of a system with a known one, and a rank-deficient one rejected
    rng = np.random.default_rng(0)
    h = rng.normal(size=9)
    B = rng.normal(size=(8, 9))
    B -= np.outer(B @ h, h) / (h @ h)
    got = ref.minimal_solver(B, ref._Margin()).ravel()
    assert np.allclose(got / np.linalg.norm(got), h / np.linalg.norm(h) * np.sign(got @ h), atol=1e-12)
    assert (got == 1.0).sum() >= 1  # 1 on the free column
    B[7] = B[0] + B[1]
    m = ref._Margin()
    assert ref.minimal_solver(B, m) is None and m.value < 1.0
    # the frame: mean at the origin, mean distance sqrt 2
    xy = rng.uniform(0, 640, (50, 2))
    mean, s = ref.frame(xy)
    n = s * (xy - mean)
    assert np.allclose(n.mean(0), 0, atol=1e-12) and np.linalg.norm(n, axis=1).mean() == pytest.approx(math.sqrt(2), rel=1e-9)


def test_library_exports_the_entries_and_the_abi_version_does_not_move():
    from lightglue_amd import robust

    lib = _lib.load()
    for s in ("lg_ransac_homography_lines", "lg_ransac_lines_lds_capacity"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION  # additive
    p, n = ctypes.c_int32(), ctypes.c_int32()
    assert lib.lg_ransac_lines_lds_capacity(ctypes.byref(p), ctypes.byref(n)) == _lib.LG_OK
    src = open(os.path.join(os.path.dirname(HERE), "cs566-project-lightglue_amd", "csrc", "kernels.h")).read()
    declared = [int(src.split(f"constexpr int {k} = ")[1].split(";")[0]) for k in ("RL_LDS_POINTS", "RL_LDS_LINES")]
    assert [robust.LDS_POINTS, robust.LDS_LINES] == [p.value, n.value] == declared  # asked of the library, no second copy
    assert min(declared) > 0
    assert lib.lg_ransac_lines_lds_capacity(None, ctypes.byref(n)) == _lib.LG_E_INVALID
    assert robust.LDS_MATCHES == lib.lg_ransac_lds_matches()  # the point-only kernel's is untouched


def test_c_entry_checks_its_arguments_before_any_device_work():
    lib = _lib.load()
    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 255) & ~255
    p = ctypes.c_void_p(base)
    # 0 kpts0 1 kpts1 2 matches0 3 num0 4 num1 | 5 lines0 6 lines1 7 line_matches0 8 num_lines0 9 num_lines1 | 10 ransac_th
    # | 11 H_gt 12 size0 13 H 14 inliers 15 line_inliers 16 info 17 m_kpts 18 m_lines 19 H_error
    def call(B=1, M=4, N=4, L0=4, L1=4, max_iters=100, confidence=0.99, seed=0, min_line_length=1.0, **at):
        a = [p] * 20
        for k, v in at.items():
            a[int(k[1:])] = v
        return lib.lg_ransac_homography_lines(a[0], a[1], a[2], B, M, N, a[3], a[4], a[5], a[6], a[7], L0, L1, a[8], a[9], a[10],
                                              max_iters, confidence, seed, min_line_length, *a[11:], None)

    def invalid(word, **kw):
        assert call(**kw) == _lib.LG_E_INVALID, kw
        assert word in lib.lg_last_error(), (kw, lib.lg_last_error())

    for k in (0, 1, 5, 6, 10, 13, 14, 15, 16, 17, 18):
        invalid(b"null", **{f"i{k}": None})
    for dim in ("B", "M", "N", "L0", "L1"):
        invalid(b"negative", **{dim: -1})
    for bad in (0, -3, 2**30 + 1):
        invalid(b"max_iters", max_iters=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        invalid(b"confidence", confidence=bad)
    for bad in (-1.0, float("nan"), float("inf")):
        invalid(b"min_line_length", min_line_length=bad)
    invalid(b"num0 and num1", i3=None)
    invalid(b"num0 and num1", i4=None)
    invalid(b"num_lines0 and num_lines1", i8=None)
    invalid(b"num_lines0 and num_lines1", i9=None)
    invalid(b"H_error needs", i11=None)
    invalid(b"H_error needs", i12=None)
    invalid(b"M == N", i2=None, M=4, N=5)
    invalid(b"L0 == L1", i7=None, L0=4, L1=5)
    off8, off4, off2 = ctypes.c_void_p(base + 8), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    for k in (2, 7):  # int64 matches
        invalid(b"misaligned", **{f"i{k}": off4})
    for k in (5, 6, 17, 18):  # 16-byte rows
        invalid(b"misaligned", **{f"i{k}": off8})
    for k in (0, 1, 3, 4, 8, 9, 10, 11, 12, 13, 16, 19):
        invalid(b"misaligned", **{f"i{k}": off2})
    # what may be null: the matches (equal sizes), each pair of counts, H_gt / size0 / H_error together,
    # and the arrays of an empty set
    nulls = {f"i{k}": None for k in (2, 3, 4, 7, 8, 9, 11, 12, 19)}
    for B, M, L in ((0, 4, 4), (3, 0, 0)):  # nothing to estimate: OK without a launch
        assert call(B=B, M=M, N=M, L0=L, L1=L, **nulls) == _lib.LG_OK
        assert call(B=B, M=M, N=M, L0=L, L1=L) == _lib.LG_OK
    assert call(B=0, M=0, N=0, **nulls, i0=None, i1=None, i14=None, i17=None) == _lib.LG_OK  # no points: their arrays may be null
    assert call(B=0, L0=0, L1=0, **nulls, i5=None, i6=None, i15=None, i18=None) == _lib.LG_OK  # no lines likewise
    invalid(b"null", B=0, i13=None)  # the checks come first even then


def cpu_inputs(B=2, M=6, N=7, L0=5, L1=4):
    g = torch.Generator().manual_seed(0)
    pred = {"keypoints0": torch.rand(B, M, 2, generator=g) * 100, "keypoints1": torch.rand(B, N, 2, generator=g) * 100,
            "matches0": torch.randint(-1, N, (B, M), generator=g), "matching_scores0": torch.rand(B, M, generator=g),
            "lines0": torch.rand(B, L0, 2, 2, generator=g) * 100, "lines1": torch.rand(B, L1, 2, 2, generator=g) * 100,
            "line_matches0": torch.randint(-1, L1, (B, L0), generator=g)}
    data = {"H_0to1": torch.eye(3).repeat(B, 1, 1), "view0": {"image_size": torch.tensor([[100.0, 100.0]]).repeat(B, 1)}}
    return data, pred


def test_python_layer_checks_its_inputs():
    import lightglue_amd
    from lightglue_amd import robust

    assert lightglue_amd.PointLineHomographyEstimator is robust.PointLineHomographyEstimator
    assert lightglue_amd.ransac_homography_lines is robust.ransac_homography_lines
    assert robust.LINES_INFO_FIELDS == ref.INFO_FIELDS
    data, pred = cpu_inputs()
    conf = {"estimator": "homography_est", "ransac_th": 1.0}
    with pytest.raises(RuntimeError, match="no CPU path"):
        robust.eval_homography_robust(data, pred, conf)
    with pytest.raises(RuntimeError, match="no CPU path"):
        robust.as_export_callback(conf)(pred, data)
    with pytest.raises(RuntimeError, match="no CPU path"):  # lines only
        robust.eval_homography_robust(data, {k: v for k, v in pred.items() if "line" in k}, conf)
    with pytest.raises(RuntimeError, match="no CPU path"):  # no lines in pred: the points alone
        robust.eval_homography_robust(data, {k: v for k, v in pred.items() if "line" not in k}, conf)
    for k in ("lines1", "line_matches0", "keypoints1", "matches0"):
        with pytest.raises(KeyError, match=k):
            robust.eval_homography_robust(data, {q: v for q, v in pred.items() if q != k}, conf)
    with pytest.raises(KeyError, match="orig_lines1"):
        robust.eval_homography_robust(data, {**pred, "orig_lines0": pred["lines0"]}, conf)
    with pytest.raises(KeyError, match="H_0to1"):
        robust.eval_homography_robust({"view0": data["view0"]}, pred, conf)
    with pytest.raises(KeyError, match="image_size"):
        robust.eval_homography_robust({**data, "view0": {}}, pred, conf)
    with pytest.raises(ValueError, match="unknown options"):  # min_area is the point-only estimator's
        robust.eval_homography_robust(data, pred, {**conf, "options": {"min_area": 1.0}})

    k0, k1, l0, l1 = pred["keypoints0"], pred["keypoints1"], pred["lines0"], pred["lines1"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        robust.ransac_homography_lines(k0, k1, pred["matches0"], l0, l1, pred["line_matches0"])
    with pytest.raises(TypeError, match="lines must be tensors"):
        robust.ransac_homography_lines(k0, k1, pred["matches0"])

    est = robust.PointLineHomographyEstimator({"ransac_th": 1.5, "options": {"seed": 5}})
    assert est.conf.ransac_th == 1.5 and est.conf.options.seed == 5 and est.conf.options.max_iters == 3000
    assert robust.PointLineHomographyEstimator.default_conf == {
        "ransac_th": 2.0, "options": {"max_iters": 3000, "confidence": 0.995, "seed": 0, "min_line_length": 1.0}}
    with pytest.raises(ValueError, match="unknown options"):
        robust.PointLineHomographyEstimator({"options": {"min_area": 1.0}})
    p, l = torch.rand(9, 2), torch.rand(5, 2, 2)
    with pytest.raises(KeyError, match="neither"):
        est({})
    with pytest.raises(KeyError, match="m_kpts1"):
        est({"m_kpts0": p})
    with pytest.raises(KeyError, match="m_lines0"):
        est({"m_kpts0": p, "m_kpts1": p, "m_lines1": l})
    for data_ in ({"m_kpts0": p, "m_kpts1": p, "m_lines0": l, "m_lines1": l}, {"m_kpts0": p, "m_kpts1": p},
                  {"m_lines0": l, "m_lines1": l}, {"m_lines0": l[None], "m_lines1": l[None], "num_line_matches": torch.tensor([3])}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            est(data_)
    with pytest.raises(ValueError, match=r"\[K, 2\]"):
        est({"m_kpts0": p, "m_kpts1": p[:5]})
    with pytest.raises(ValueError, match=r"\[K, 2, 2\]"):
        est({"m_lines0": l, "m_lines1": l[:3]})
    with pytest.raises(ValueError, match=r"\[K, 2, 2\]"):
        est({"m_lines0": torch.rand(5, 4), "m_lines1": torch.rand(5, 4)})
    with pytest.raises(ValueError, match="both be batched"):
        est({"m_kpts0": p[None], "m_kpts1": p[None], "m_lines0": l, "m_lines1": l})
    with pytest.raises(ValueError, match="batched form"):
        est({"m_kpts0": p, "m_kpts1": p, "num_matches": torch.tensor([5])})
    with pytest.raises(ValueError, match="batched form"):
        est({"m_lines0": l, "m_lines1": l, "num_line_matches": torch.tensor([5])})


def test_load_estimator_names():
    from lightglue_amd import relative_pose, robust

    assert robust.load_estimator("homography", "homography_est") is robust.PointLineHomographyEstimator
    assert relative_pose.load_estimator("homography", "homography_est") is robust.PointLineHomographyEstimator
    assert robust.load_estimator("homography", "hip") is robust.HomographyEstimator  # unchanged
    assert relative_pose.load_estimator("homography", "hip") is robust.HomographyEstimator
    assert relative_pose.load_estimator("relative_pose", "hip") is relative_pose.RelativePoseEstimator
    # names that raised before still raise
    with pytest.raises(NotImplementedError, match="out of scope"):
        robust.load_estimator("relative_pose", "homography_est")
    with pytest.raises(ValueError, match="opencv"):
        robust.load_estimator("homography", "opencv")
    with pytest.raises(ValueError, match="lines"):
        robust.load_estimator("lines", "homography_est")
    with pytest.raises(ValueError, match="homography_est"):
        relative_pose.load_estimator("relative_pose", "homography_est")
    with pytest.raises(ValueError, match="poselib"):
        relative_pose.load_estimator("homography", "poselib")
