"""Robust homography estimation without a GPU: the float64 restatement (tests/ransac_ref.py) against
the fixture it produced (tests/golden/ransac/ransac.npz) and against the true homographies, the
library's export and argument checks, and the Python layer's checks (lightglue_amd.robust)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import ransac_ref as ref
from lightglue_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac", "ransac.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def options(g, name):
    return {"max_iters": int(g[f"{name}/max_iters"]), "confidence": float(g[f"{name}/confidence"]),
            "seed": int(g[f"{name}/seed"]), "min_area": float(g[f"{name}/min_area"])}


@pytest.fixture(scope="module")
def restated(golden):
    """Every case through the restatement, once."""
    return {name: ref.estimate_pair(golden[f"{name}/kpts0"], golden[f"{name}/kpts1"], golden[f"{name}/matches0"],
                                    float(golden[f"{name}/th"]), H_gt=golden[f"{name}/H_gt"], size=golden[f"{name}/size0"],
                                    **options(golden, name)) for name in golden["cases"]}


def test_restatement_reproduces_the_fixture(golden, restated):
    assert list(golden["cases"]) == list("123456789")
    for name, o in restated.items():
        np.testing.assert_array_equal(ref.info_row(o), golden[f"{name}/info"], err_msg=name)
        np.testing.assert_array_equal(o["inliers_slots"], golden[f"{name}/inliers"], err_msg=name)
        np.testing.assert_array_equal(o["m_kpts"], golden[f"{name}/m_kpts"], err_msg=name)
        if o["success"]:
            # another BLAS may move the SVD's last bits, and with them an fp32 rounding of the matrix
            np.testing.assert_allclose(o["H"], golden[f"{name}/H"], rtol=0, atol=2e-7 * np.abs(o["H"]).max(), err_msg=name)
            assert abs(o["H_error"] - float(golden[f"{name}/H_error"])) <= 1e-4 * o["H_error"] + 1e-7
        else:
            np.testing.assert_array_equal(o["H"], np.eye(3, dtype=np.float32))
            assert math.isinf(o["H_error"]) and not o["inliers_slots"].any() and o["num_inliers"] == 0
        assert o["margin"] >= float(golden["min_margin"]) == 1e-7, name
        assert o["margin"] == pytest.approx(float(golden[f"{name}/margin"]), rel=1e-3) or math.isinf(o["margin"])


def test_cases_reach_the_branches_they_are_there_for(golden, restated):
    info = {name: dict(zip(ref.INFO_FIELDS, golden[f"{name}/info"].tolist())) for name in golden["cases"]}
    assert info["1"]["rounds"] == 1 and info["1"]["num_matches"] == 64 and int(golden["1/max_iters"]) == 512
    assert info["2"]["rounds"] > 1 and info["2"]["num_matches"] == 200
    assert info["3"]["rounds"] == 2 and info["3"]["best_t"] < 300 == int(golden["3/max_iters"])
    assert info["3"]["num_matches"] == 150
    assert info["4"] == {**info["4"], "success": 1, "num_matches": 4, "num_inliers": 4}
    assert info["5"] == {**info["5"], "success": 0, "num_matches": 3, "rounds": 0}
    assert info["6"] == {**info["6"], "success": 0, "valid_hypotheses": 0, "best_t": -1} and info["6"]["num_matches"] > 4
    assert info["7"] == {**info["7"], "success": 0, "num_matches": 0, "rounds": 0}
    assert info["8"]["num_matches"] == 5 and info["8"]["success"] == 1
    # K = 5: most hypotheses have to draw again, and every one still ends with four distinct matches
    redraws = [len({((ref.mix64(ref.mix64(0) + (t << 16) + d) >> 32) * 5) >> 32 for d in range(4)}) < 4 for t in range(256)]
    assert sum(redraws) > 128 and all(len(set(ref.sample(0, t, 5))) == 4 for t in range(256))
    m9 = golden["9/matches0"]
    assert (m9 < -1).any() and (m9 >= len(golden["9/kpts1"])).any() and info["9"]["num_matches"] == 90
    assert len(golden["9/kpts0"]) != len(golden["9/kpts1"])
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_finds_the_true_model(golden, restated):
    for name in "12":  # at least 0.9 of what the true homography explains
        assert restated[name]["num_inliers"] >= 0.9 * int(golden[f"{name}/inliers_under_H_gt"]) > 0
    for name in "48":  # noise-free
        assert restated[name]["H_error"] < 1e-3
    for name, o in restated.items():  # the mask is the returned matrix's own
        pts, slots = ref.live_matches(golden[f"{name}/kpts0"], golden[f"{name}/kpts1"], golden[f"{name}/matches0"])
        if o["success"]:
            again = ref.residuals(o["H"].astype(np.float64), pts) < float(golden[f"{name}/th"])
            np.testing.assert_array_equal(again, o["inliers_slots"][slots])


def test_restatement_sampler_follows_the_specification():
    """The restatement's own sampler (the kernel's is pinned against it in tests/test_gpu_ransac.py)."""
    assert ref.mix64(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for state 0
    a = [ref.sample(7, t, 100) for t in range(8)]
    assert a == [ref.sample(7, t, 100) for t in range(8)] and a != [ref.sample(8, t, 100) for t in range(8)]
    assert all(0 <= i < 100 for s in a for i in s)
    assert ref.sample(0, 0, 3) is None  # four distinct indices do not exist: invalid after 64 draws


def test_library_exports_the_entry_and_the_abi_version_does_not_move():
    from lightglue_amd import robust

    lib = _lib.load()
    for s in ("lg_ransac_homography", "lg_ransac_lds_matches"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION  # additive
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cs566-project-lightglue_amd", "csrc",
                            "kernels.h")).read()
    declared = int(src.split("constexpr int RH_LDS_MATCHES = ")[1].split(";")[0])
    assert robust.LDS_MATCHES == lib.lg_ransac_lds_matches() == declared > 0  # asked of the library, no second copy


def test_c_entry_checks_its_arguments_before_any_device_work():
    lib = _lib.load()
    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 255) & ~255
    p = ctypes.c_void_p(base)
    # 0 kpts0 1 kpts1 2 matches0 | 3 num0 4 num1 5 ransac_th | 6 H_gt 7 size0 8 H 9 inliers 10 info 11 m_kpts 12 H_error
    def call(B=1, M=4, N=4, max_iters=100, confidence=0.99, seed=0, min_area=1.0, **at):
        a = [p] * 13
        for k, v in at.items():
            a[int(k[1:])] = v
        return lib.lg_ransac_homography(a[0], a[1], a[2], B, M, N, a[3], a[4], a[5], max_iters, confidence, seed, min_area,
                                        *a[6:], None)

    def invalid(word, **kw):
        assert call(**kw) == _lib.LG_E_INVALID, kw
        assert word in lib.lg_last_error(), (kw, lib.lg_last_error())

    for k in (0, 1, 5, 8, 9, 10, 11):
        invalid(b"null", **{f"i{k}": None})
    for dim in ("B", "M", "N"):
        invalid(b"negative", **{dim: -1})
    for bad in (0, -3, 2**30 + 1):
        invalid(b"max_iters", max_iters=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        invalid(b"confidence", confidence=bad)
    invalid(b"min_area", min_area=-1.0)
    invalid(b"both", i3=None)
    invalid(b"both", i4=None)
    invalid(b"H_error needs", i6=None)
    invalid(b"H_error needs", i7=None)
    invalid(b"M == N", i2=None, M=4, N=5)
    off8, off4, off2 = ctypes.c_void_p(base + 8), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    invalid(b"misaligned", i2=off4)  # int64 matches
    invalid(b"misaligned", i11=off8)  # 16-byte rows
    for k in (0, 1, 3, 4, 5, 6, 7, 8, 10, 12):
        invalid(b"misaligned", **{f"i{k}": off2})
    # what may be null: matches0 (M == N), the counts together, H_gt / size0 / H_error together
    nulls = {f"i{k}": None for k in (2, 3, 4, 6, 7, 12)}
    for B, M in ((0, 4), (3, 0)):  # nothing to estimate: OK without a launch
        assert call(B=B, M=M, N=M, **nulls) == _lib.LG_OK
        assert call(B=B, M=M) == _lib.LG_OK
    invalid(b"null", B=0, i0=None)  # the checks come first even then


def cpu_inputs(B=2, M=6, N=7):
    g = torch.Generator().manual_seed(0)
    pred = {"keypoints0": torch.rand(B, M, 2, generator=g) * 100, "keypoints1": torch.rand(B, N, 2, generator=g) * 100,
            "matches0": torch.randint(-1, N, (B, M), generator=g), "matching_scores0": torch.rand(B, M, generator=g)}
    data = {"H_0to1": torch.eye(3).repeat(B, 1, 1), "view0": {"image_size": torch.tensor([[100.0, 100.0]]).repeat(B, 1)}}
    return data, pred


def test_python_layer_checks_its_inputs():
    import lightglue_amd
    from lightglue_amd import robust

    assert lightglue_amd.eval_homography_robust is robust.eval_homography_robust
    assert lightglue_amd.HomographyEstimator is robust.HomographyEstimator
    assert lightglue_amd.load_estimator is robust.load_estimator
    data, pred = cpu_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        robust.eval_homography_robust(data, pred, {"estimator": "hip", "ransac_th": 1.0})
    with pytest.raises(RuntimeError, match="no CPU path"):
        robust.as_export_callback()(pred, data)
    for k in pred:
        with pytest.raises(KeyError, match=k):
            robust.eval_homography_robust(data, {q: v for q, v in pred.items() if q != k})
    with pytest.raises(KeyError, match="H_0to1"):
        robust.eval_homography_robust({"view0": data["view0"]}, pred)
    with pytest.raises(KeyError, match="image_size"):
        robust.eval_homography_robust({**data, "view0": {}}, pred)

    est = robust.HomographyEstimator({"ransac_th": 2.0, "options": {"seed": 5}})
    assert est.conf.ransac_th == 2.0 and est.conf.options.seed == 5 and est.conf.options.max_iters == 3000
    assert robust.HomographyEstimator.default_conf == {
        "ransac_th": 3.0, "options": {"max_iters": 3000, "confidence": 0.995, "seed": 0, "min_area": 1.0}}
    assert est.required_data_keys == ["m_kpts0", "m_kpts1"]
    with pytest.raises(ValueError, match="unknown options"):
        robust.HomographyEstimator({"options": {"method": "ransac"}})
    p = torch.rand(9, 2)
    with pytest.raises(KeyError, match="m_kpts1"):
        est({"m_kpts0": p})
    with pytest.raises(RuntimeError, match="no CPU path"):
        est({"m_kpts0": p, "m_kpts1": p})
    with pytest.raises(RuntimeError, match="no CPU path"):
        est({"m_kpts0": p[None], "m_kpts1": p[None], "num_matches": torch.tensor([5])})
    with pytest.raises(ValueError, match=r"\[K, 2\]"):
        est({"m_kpts0": p, "m_kpts1": p[:5]})
    with pytest.raises(ValueError, match=r"\[K, 2\]"):
        est({"m_kpts0": torch.rand(9, 3), "m_kpts1": torch.rand(9, 3)})
    with pytest.raises(ValueError, match="batched form"):
        est({"m_kpts0": p, "m_kpts1": p, "num_matches": torch.tensor([5])})


def test_load_estimator():
    from lightglue_amd import robust

    assert robust.load_estimator("homography", "hip") is robust.HomographyEstimator
    with pytest.raises(NotImplementedError, match="out of scope"):
        robust.load_estimator("relative_pose", "hip")
    with pytest.raises(ValueError, match="opencv"):
        robust.load_estimator("homography", "opencv")
    with pytest.raises(ValueError, match="lines"):
        robust.load_estimator("lines", "hip")
