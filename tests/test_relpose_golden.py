"""Robust relative pose without a GPU: the float64 restatement (tests/relpose_ref.py) against the
fixture it produced (tests/golden/relpose/relpose.npz) and against the true poses, the library's
exports and argument checks, and the Python layer's checks (lightglue_amd.relative_pose)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import relpose_ref as ref
from lightglue_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relpose", "relpose.npz")
CASES = ["one_round", "several_rounds", "partial_round", "five_exact", "four", "none", "plane", "forward", "intrinsics",
         "keypoints", "lds", "lds_plus_1"]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def restate(g, name, route="kernel"):
    return ref.estimate_pair(g[f"{name}/kpts0"], g[f"{name}/kpts1"], g[f"{name}/matches0"], g[f"{name}/camera0"],
                             g[f"{name}/camera1"], float(g[f"{name}/th"]), T_gt=g[f"{name}/T_gt"], route=route,
                             max_iters=int(g[f"{name}/max_iters"]), confidence=float(g[f"{name}/confidence"]),
                             seed=int(g[f"{name}/seed"]))


@pytest.fixture(scope="module")
def restated(golden):
    """Every case through the restatement, once."""
    return {name: restate(golden, name) for name in golden["cases"]}


def test_restatement_reproduces_the_fixture(golden, restated):
    assert list(golden["cases"]) == CASES
    bar = float(golden["pose_abs_bar"])
    for name, o in restated.items():
        np.testing.assert_array_equal(ref.info_row(o), golden[f"{name}/info"], err_msg=name)
        np.testing.assert_array_equal(o["inliers_slots"], golden[f"{name}/inliers"], err_msg=name)
        err = np.array([o["t_err"], o["r_err"], o["rel_pose_error"]])
        if o["success"]:
            # another BLAS may move an SVD's last bits, and with them an fp32 rounding of the pose
            np.testing.assert_allclose(o["R"], golden[f"{name}/R"], rtol=0, atol=bar, err_msg=name)
            np.testing.assert_allclose(o["t"], golden[f"{name}/t"], rtol=0, atol=bar, err_msg=name)
            np.testing.assert_allclose(err, golden[f"{name}/errors"], rtol=1e-4, err_msg=name)
            assert min(o["t_err"], o["r_err"]) >= 0.01, name  # the arccos is well conditioned
        else:
            np.testing.assert_array_equal(o["R"], np.eye(3, dtype=np.float32))
            assert np.isinf(err).all() and not o["t"].any() and not o["inliers_slots"].any() and o["num_inliers"] == 0
        assert o["margin"] >= float(golden["min_margin"]) == 1e-7, name
        assert o["margin"] == pytest.approx(float(golden[f"{name}/margin"]), rel=1e-3) or math.isinf(o["margin"])
    assert bar == max(10 * float(golden["pose_route_diff"]), 2.0**-22)
    assert float(golden["solver_res_bar"]) == 1000 * float(golden["solver_res_companion"]) > 0


def test_two_root_routes_agree_on_a_case(golden, restated):
    """The generator's acceptance condition, once more on the smallest full case."""
    a, b = restated["one_round"], restate(golden, "one_round", "companion")
    np.testing.assert_array_equal(ref.info_row(a)[:7], ref.info_row(b)[:7])
    np.testing.assert_array_equal(a["inliers_slots"], b["inliers_slots"])
    assert a["trace"] == b["trace"]
    np.testing.assert_allclose(a["R"], b["R"], rtol=0, atol=float(golden["pose_abs_bar"]))


def test_cases_reach_the_branches_they_are_there_for(golden, restated):
    info = {name: dict(zip(ref.INFO_FIELDS, golden[f"{name}/info"].tolist())) for name in golden["cases"]}
    assert info["one_round"]["rounds"] == 1 and info["one_round"]["success"] == 1
    assert info["several_rounds"]["rounds"] > 2
    assert info["partial_round"]["rounds"] == 2 and info["partial_round"]["best_t"] < 300 == int(golden["partial_round/max_iters"])
    assert info["partial_round"]["valid_samples"] == 300
    assert info["five_exact"] == {**info["five_exact"], "success": 1, "num_matches": 5, "num_inliers": 5}
    assert info["four"] == {**info["four"], "success": 0, "num_matches": 4, "rounds": 0, "best_t": -1}
    assert info["none"] == {**info["none"], "success": 0, "num_matches": 0, "rounds": 0}
    for name in ("plane", "forward", "intrinsics", "keypoints", "lds", "lds_plus_1", "one_round", "several_rounds"):
        assert info[name]["success"] == 1 and float(golden[f"{name}/errors"][2]) < 2.0, name
    assert (golden["intrinsics/camera0"] != golden["intrinsics/camera1"]).all()
    np.testing.assert_array_equal(golden["forward/T_gt"][9:], [0, 0, 1])
    m = golden["keypoints/matches0"]
    assert (m < -1).any() and (m >= len(golden["keypoints/kpts1"])).any() and info["keypoints"]["num_matches"] == 90
    assert len(golden["keypoints/kpts0"]) != len(golden["keypoints/kpts1"])
    assert info["lds_plus_1"]["num_matches"] == info["lds"]["num_matches"] + 1 == _lib.load().lg_ransac_lds_matches() + 1
    for name in golden["cases"]:
        assert len(golden[f"{name}/kpts0"]) <= 300 or name.startswith("lds")
        assert int(golden[f"{name}/max_iters"]) <= 1024
    assert os.path.getsize(GOLDEN) < 256 * 1024


def test_plane_case_is_a_plane(golden):
    """All true matches of the plane case are views of one plane: they satisfy one homography."""
    g = golden
    pts = ref.normalise(np.concatenate([g["plane/kpts0"], g["plane/kpts1"]], 1), g["plane/camera0"], g["plane/camera1"])
    inl = pts[g["plane/inliers"]]
    x, y, u, v = inl.T
    z, o = np.zeros_like(x), np.ones_like(x)
    A = np.concatenate([np.stack([z, z, z, -x, -y, -o, v * x, v * y, v], 1), np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], 1)])
    H = np.linalg.svd(A)[2][-1].reshape(3, 3)
    p = np.stack([x, y, o], 1) @ H.T
    d = np.linalg.norm(p[:, :2] / p[:, 2:] - inl[:, 2:], axis=1)
    assert len(inl) > 90 and np.median(d) < 2 * ref.threshold_n(1.0, g["plane/camera0"], g["plane/camera1"])


def test_mask_is_the_returned_pose_s_own(golden, restated):
    for name, o in restated.items():
        if not o["success"]:
            continue
        g = golden
        pts, slots = ref.live_matches(g[f"{name}/kpts0"], g[f"{name}/kpts1"], g[f"{name}/matches0"])
        n = ref.normalise(pts, g[f"{name}/camera0"], g[f"{name}/camera1"])
        th = ref.threshold_n(float(g[f"{name}/th"]), g[f"{name}/camera0"], g[f"{name}/camera1"])
        R, t = o["R"].astype(np.float64), o["t"].astype(np.float64)
        again = (ref.sampson2(ref.essential_from(R, t), n) < th * th) & ref._front(R, t, n)
        np.testing.assert_array_equal(again, o["inliers_slots"][slots], err_msg=name)
        assert abs(np.linalg.norm(t) - 1) < 1e-6 and np.linalg.det(R) > 0
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6


def test_sampler_gives_five_distinct_indices():
    assert ref.mix64(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for state 0
    a = [ref.sample5(7, t, 100) for t in range(8)]
    assert a == [ref.sample5(7, t, 100) for t in range(8)] and a != [ref.sample5(8, t, 100) for t in range(8)]
    assert all(len(set(s)) == 5 and all(0 <= i < 100 for i in s) for s in a)
    assert all(len(set(ref.sample5(0, t, 5))) == 5 for t in range(256))  # K = 5: draws again until all five
    assert ref.sample5(0, 0, 4) is None  # five distinct indices do not exist: invalid after 64 draws
    # §10k's draw(t, d), unchanged: the first four indices are the homography sampler's
    import ransac_ref

    assert all(ref.sample5(3, t, 50)[:4] == ransac_ref.sample(3, t, 50) for t in range(32))


def test_solver_samples_and_routes(golden):
    """The stored candidates are the companion route's; the kernel route gives the same ones."""
    P, kind = golden["solver/pts"], golden["solver/kind"]
    assert P.shape == (64, 5, 4) and P.dtype == np.float32
    assert np.bincount(kind).tolist() == [21, 21, 21, 1]
    Ek, ck, _ = ref.essential_5pt(P.astype(np.float64), "kernel")
    np.testing.assert_array_equal(ck, golden["solver/count"])
    bar = float(golden["pose_abs_bar"])
    for s in range(64):
        for j in range(ck[s]):
            assert np.abs(Ek[s, j] - golden["solver/E"][s, j]).max() <= bar, (s, j)
    assert ck[63] == 0 and (ck[:63] >= 2).all()  # the repeated point: rank 4, rejected at the pivot floor
    assert (golden["solver/true_dist"][kind < 2] < 1e-3).all()


def test_library_exports_the_entries_and_the_abi_version_does_not_move():
    lib = _lib.load()
    for s in ("lg_ransac_relpose", "lg_essential_5pt"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION  # additive


def test_c_entry_checks_its_arguments_before_any_device_work():
    lib = _lib.load()
    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 255) & ~255
    p = ctypes.c_void_p(base)
    # 0 kpts0 1 kpts1 2 matches0 | 3 num0 4 num1 5 camera0 6 camera1 7 ransac_th | 8 T_gt 9 R 10 t 11 inliers 12 info
    # 13 m_kpts 14 errors
    def call(B=1, M=4, N=4, max_iters=100, confidence=0.99, seed=0, **at):
        a = [p] * 15
        for k, v in at.items():
            a[int(k[1:])] = v
        return lib.lg_ransac_relpose(a[0], a[1], a[2], B, M, N, a[3], a[4], a[5], a[6], a[7], max_iters, confidence, seed,
                                     *a[8:], None)

    def invalid(word, **kw):
        assert call(**kw) == _lib.LG_E_INVALID, kw
        assert word in lib.lg_last_error(), (kw, lib.lg_last_error())

    for k in (0, 1, 5, 6, 7, 9, 10, 11, 12, 13):
        invalid(b"null", **{f"i{k}": None})
    for dim in ("B", "M", "N"):
        invalid(b"negative", **{dim: -1})
    for bad in (0, -3, 2**30 + 1):
        invalid(b"max_iters", max_iters=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        invalid(b"confidence", confidence=bad)
    invalid(b"both", i3=None)
    invalid(b"both", i4=None)
    invalid(b"errors need", i8=None)
    invalid(b"M == N", i2=None, M=4, N=5)
    off8, off4, off2 = ctypes.c_void_p(base + 8), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    invalid(b"misaligned", i2=off4)  # int64 matches
    invalid(b"misaligned", i13=off8)  # 16-byte rows
    for k in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14):
        invalid(b"misaligned", **{f"i{k}": off2})
    # what may be null: matches0 (M == N), the counts together, T_gt with the errors
    nulls = {f"i{k}": None for k in (2, 3, 4, 8, 14)}
    for B, M in ((0, 4), (3, 0)):  # nothing to estimate: OK without a launch
        assert call(B=B, M=M, N=M, **nulls) == _lib.LG_OK
        assert call(B=B, M=M) == _lib.LG_OK
    invalid(b"null", B=0, i0=None)  # the checks come first even then

    def solver(S=1, pts=p, E=p, count=p):
        return lib.lg_essential_5pt(pts, S, E, count, None)

    for kw in ({"pts": None}, {"E": None}, {"count": None}, {"S": -1}, {"E": off4}, {"pts": off2}, {"count": off2}):
        assert solver(**kw) == _lib.LG_E_INVALID, kw
    assert solver(S=0) == _lib.LG_OK


def cpu_inputs(B=2, M=6, N=7):
    g = torch.Generator().manual_seed(0)
    pred = {"keypoints0": torch.rand(B, M, 2, generator=g) * 100, "keypoints1": torch.rand(B, N, 2, generator=g) * 100,
            "matches0": torch.randint(-1, N, (B, M), generator=g), "matching_scores0": torch.rand(B, M, generator=g)}
    cam = torch.tensor([[200.0, 100.0, 150.0, 150.0, 100.0, 50.0]]).repeat(B, 1)
    data = {"T_0to1": torch.eye(4)[:3].T.flatten().repeat(B, 1), "view0": {"camera": cam}, "view1": {"camera": cam}}
    return data, pred


def test_python_layer_checks_its_inputs():
    import lightglue_amd
    from lightglue_amd import relative_pose as rp

    assert lightglue_amd.eval_relative_pose_robust is rp.eval_relative_pose_robust
    assert lightglue_amd.RelativePoseEstimator is rp.RelativePoseEstimator
    assert lightglue_amd.ransac_relpose is rp.ransac_relpose
    data, pred = cpu_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        rp.eval_relative_pose_robust(data, pred, {"estimator": "hip", "ransac_th": 1.0})
    with pytest.raises(RuntimeError, match="no CPU path"):
        rp.as_export_callback()(pred, data)
    for k in pred:
        with pytest.raises(KeyError, match=k):
            rp.eval_relative_pose_robust(data, {q: v for q, v in pred.items() if q != k})
    for k in ("T_0to1", "view1"):
        with pytest.raises(KeyError, match=k):
            rp.eval_relative_pose_robust({q: v for q, v in data.items() if q != k}, pred)
    with pytest.raises(KeyError, match="camera"):
        rp.eval_relative_pose_robust({**data, "view0": {}}, pred)

    est = rp.RelativePoseEstimator({"ransac_th": 0.5, "options": {"seed": 5}})
    assert est.conf.ransac_th == 0.5 and est.conf.options.seed == 5 and est.conf.options.max_iters == 2000
    assert rp.RelativePoseEstimator.default_conf == {
        "ransac_th": 1.0, "options": {"max_iters": 2000, "confidence": 0.9999, "seed": 0}}
    assert est.required_data_keys == ["m_kpts0", "m_kpts1", "camera0", "camera1"]
    with pytest.raises(ValueError, match="unknown options"):
        rp.RelativePoseEstimator({"options": {"method": "ransac"}})
    p, cam = torch.rand(9, 2), data["view0"]["camera"][0]
    full = {"m_kpts0": p, "m_kpts1": p, "camera0": cam, "camera1": cam}
    for k in full:
        with pytest.raises(KeyError, match=k):
            est({q: v for q, v in full.items() if q != k})
    with pytest.raises(RuntimeError, match="no CPU path"):
        est(full)
    with pytest.raises(RuntimeError, match="no CPU path"):
        est({**full, "m_kpts0": p[None], "m_kpts1": p[None], "num_matches": torch.tensor([5])})
    with pytest.raises(ValueError, match=r"\[K, 2\]"):
        est({**full, "m_kpts1": p[:5]})
    with pytest.raises(ValueError, match="batched form"):
        est({**full, "num_matches": torch.tensor([5])})
    with pytest.raises(ValueError, match="required"):
        rp.ransac_relpose(p[None], p[None])


def test_load_estimator_resolves_both_types():
    import lightglue_amd
    from lightglue_amd import relative_pose as rp
    from lightglue_amd import robust

    assert rp.load_estimator("relative_pose", "hip") is rp.RelativePoseEstimator
    assert rp.load_estimator("homography", "hip") is robust.HomographyEstimator
    with pytest.raises(ValueError, match="poselib"):
        rp.load_estimator("relative_pose", "poselib")
    with pytest.raises(ValueError, match="lines"):
        rp.load_estimator("lines", "hip")
    assert lightglue_amd.load_estimator is robust.load_estimator  # the package's name stays the homography module's
