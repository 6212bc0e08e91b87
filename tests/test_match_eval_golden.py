"""Host side of the batched match evaluation (lightglue_amd.match_eval, lg_eval_matches): the float64
restatement the GPU tests compare against reproduces the reference's fixture
(tests/golden/match_eval/match_eval.npz, written by tests/golden/make_match_eval_golden.py), the C entry is
exported and checks its arguments before any device work, and the Python layer checks its inputs --
no GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import match_eval_ref as ref
from lightglue_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_eval", "match_eval.npz")
CASES = "abcdefghij"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def case_pairs(g, name):
    """One dict of torch tensors per pair of a fixture case (num0 / num1 ints for the ragged case)."""
    B = g[f"{name}/kpts0"].shape[0]
    for b in range(B):
        p = {k.split("/")[1]: torch.from_numpy(np.asarray(v[b])) for k, v in g.items() if k.startswith(name + "/")}
        if "num0" in p:
            p["num0"], p["num1"] = int(p["num0"]), int(p["num1"])
        yield p


def evaluate(p):
    return ref.evaluate_pair(p["kpts0"], p["kpts1"], p["matches0"], p["scores0"], H=p["H"], image_size=p["size0"],
                             cam0=p["cam0"], cam1=p["cam1"], T=p["T"], num0=p.get("num0"), num1=p.get("num1"))


def test_fixture_has_every_case_and_the_margin_holds(golden):
    assert {k.split("/")[0] for k in golden if "/" in k} == set(CASES)
    assert 1e-6 < float(golden["dlt_rel_bar"]) < 1e-3  # fp32 against fp64 on a few hundred matches
    lives = {n: [int(c[0]) for c in golden[f"{n}/hom_counts"]] for n in CASES}
    assert lives == {"a": [4], "b": [33], "c": [65], "d": [200], "e": [256], "f": [257], "g": [0], "h": [3],
                     "i": [4, 33, 65], "j": [60, 75]}
    margin = float(golden["margin"])
    for n in CASES:
        for key, ths in (("hom", ref.HOM_THRESHOLDS), ("epi", ref.EPI_THRESHOLDS)):
            e = golden[f"{n}/{key}_err64"]
            e = e[~np.isnan(e)]
            for t in ths:
                assert e.size == 0 or np.abs(e - t).min() >= margin * t, (n, key, t)
    # every threshold has matches on both sides somewhere
    for key, cols in (("hom_counts", 2), ("epi_counts", 3)):
        c = np.concatenate([golden[f"{n}/{key}"] for n in CASES])
        for j in range(1, cols + 1):
            assert 0 < c[:, j].sum() < c[:, 0].sum()
    assert (golden["i/matches0"][0, 5:] >= 0).all()  # stale indices planted in the padding
    assert not np.array_equal(golden["j/size0"][0], golden["j/size0"][1])
    assert (golden["j/cam0"][:, 2] != golden["j/cam0"][:, 3]).all()  # fx != fy


@pytest.mark.parametrize("name", list(CASES))
def test_float64_restatement_reproduces_the_fixture(golden, name):
    for b, p in enumerate(case_pairs(golden, name)):
        out = evaluate(p)
        assert [out["n"]] + out["hom_counts"] == golden[f"{name}/hom_counts"][b].tolist()
        assert [out["n"]] + out["epi_counts"] == golden[f"{name}/epi_counts"][b].tolist()
        for key in ("hom_err", "epi_err"):
            want = golden[f"{name}/{key}64"][b]
            want = want[~np.isnan(want)]
            np.testing.assert_allclose(out[key].numpy(), want, rtol=1e-12, atol=0)
        want = golden[f"{name}/dlt_err64"][b]
        if out["n"] < 4:
            assert np.isnan(want) and np.isnan(out["H_error_dlt"]) and torch.isinf(out["H_dlt"]).all()
        else:
            # an eigenvector (eigh) against a singular vector (svd) of the same fp64 matrix: the corner
            # error agrees to the conditioning of the smallest eigenvector, far inside the bar.  The
            # homography itself is only defined to 2e-8 / |h22| relative: the two solvers may return
            # opposite signs, and h / (h22 + 1e-8) is not odd in h (h22 of the unit vector is ~0.1-1).
            assert abs(out["H_error_dlt"] - want) <= 1e-8 * want
            np.testing.assert_allclose(out["H_dlt"].numpy(), golden[f"{name}/H_dlt64"][b], rtol=0,
                                       atol=1e-6 * np.abs(golden[f"{name}/H_dlt64"][b]).max())


def test_library_exports_the_entry_and_the_abi_version_does_not_move():
    lib = _lib.load()
    assert "lg_eval_matches" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "lg_eval_matches")
    assert lib.lg_abi_version() == 12 == _lib.ABI_VERSION  # additive


def test_c_entry_checks_its_arguments_before_any_device_work():
    lib = _lib.load()
    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 255) & ~255
    p = ctypes.c_void_p(base)
    # 0 kpts0 1 kpts1 2 matches0 3 scores0 | 4 num0 5 num1 6 H 7 cam0 8 cam1 9 T 10 size0 | 11 hom_counts
    # 12 epi_counts 13 H_dlt 14 H_error_dlt
    def call(B=1, M=4, N=4, flags=7, **at):
        a = [p] * 15
        for k, v in at.items():
            a[int(k[1:])] = v
        return lib.lg_eval_matches(a[0], a[1], a[2], a[3], B, M, N, *a[4:11], flags, *a[11:], None)

    def invalid(word, **kw):
        assert call(**kw) == _lib.LG_E_INVALID, kw
        assert word in lib.lg_last_error(), (kw, lib.lg_last_error())

    for k in (0, 1, 2):
        invalid(b"null", **{f"i{k}": None})
    for dim in ("B", "M", "N"):
        invalid(b"negative", **{dim: -1})
    invalid(b"unknown flag", flags=8)
    invalid(b"unknown flag", flags=-1)
    invalid(b"no metric", flags=0)
    for k in (6, 11):  # a flag whose inputs or outputs are missing
        invalid(b"LG_EVAL_HOMOGRAPHY", flags=1, **{f"i{k}": None})
    for k in (7, 8, 9, 12):
        invalid(b"LG_EVAL_EPIPOLAR", flags=2, **{f"i{k}": None})
    for k in (3, 6, 10, 13, 14):
        invalid(b"LG_EVAL_DLT", flags=4, **{f"i{k}": None})
    invalid(b"both", i4=None)
    invalid(b"both", i5=None)
    off4, off2 = ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    invalid(b"misaligned", i2=off4)  # int64 matches
    for k in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14):
        invalid(b"misaligned", **{f"i{k}": off2})
    # what a flag does not name may be null: only the homography inputs and outputs
    nulls = {f"i{k}": None for k in (3, 4, 5, 7, 8, 9, 10, 12, 13, 14)}
    for B, M in ((0, 4), (3, 0)):  # nothing to evaluate: OK without a launch
        assert call(B=B, M=M, flags=1, **nulls) == _lib.LG_OK
        assert call(B=B, M=M) == _lib.LG_OK
    invalid(b"null", B=0, i0=None)  # the checks come first even then


def cpu_inputs(B=2, M=6, N=7):
    g = torch.Generator().manual_seed(0)
    pred = {"keypoints0": torch.rand(B, M, 2, generator=g) * 100, "keypoints1": torch.rand(B, N, 2, generator=g) * 100,
            "matches0": torch.randint(-1, N, (B, M), generator=g), "matching_scores0": torch.rand(B, M, generator=g)}
    cam = torch.tensor([[100.0, 100.0, 80.0, 90.0, 50.0, 50.0]]).repeat(B, 1)
    data = {"H_0to1": torch.eye(3).repeat(B, 1, 1), "T_0to1": torch.eye(4)[None].repeat(B, 1, 1),
            "view0": {"image_size": torch.tensor([[100.0, 100.0]]).repeat(B, 1), "camera": cam},
            "view1": {"camera": cam}}
    return data, pred


def test_python_layer_checks_its_inputs():
    import lightglue_amd
    from lightglue_amd import match_eval as me

    assert lightglue_amd.eval_matches is me.eval_matches
    assert lightglue_amd.eval_homography_dlt is me.eval_homography_dlt
    data, pred = cpu_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        me.eval_matches(data, pred)
    for fn in (me.eval_matches_homography, me.eval_matches_epipolar, me.eval_homography_dlt):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(data, pred)
    for k in pred:
        with pytest.raises(KeyError, match=k):
            me.eval_matches(data, {q: v for q, v in pred.items() if q != k})
    with pytest.raises(KeyError, match="H_0to1"):
        me.eval_matches_homography({}, pred)
    with pytest.raises(KeyError, match="T_0to1"):
        me.eval_matches_epipolar({k: v for k, v in data.items() if k != "T_0to1"}, pred)
    with pytest.raises(KeyError, match="camera"):
        me.eval_matches_epipolar({**data, "view1": {}}, pred)
    with pytest.raises(KeyError, match="image_size"):
        me.eval_homography_dlt({**data, "view0": {}}, pred)
    with pytest.raises(ValueError, match="metrics"):
        me.eval_matches(data, pred, metrics=("robust",))
    with pytest.raises(ValueError, match="metrics"):
        me.eval_matches(data, pred, metrics=())
    with pytest.raises(ValueError, match="matches0"):
        me.eval_matches(data, {**pred, "matches0": pred["matches0"][:, :-1]})
    with pytest.raises(ValueError, match="matches0"):
        me.eval_matches(data, {**pred, "matching_scores0": pred["matching_scores0"][:1]})
    with pytest.raises(ValueError, match="keypoints"):
        me.eval_matches(data, {**pred, "keypoints1": pred["keypoints1"][:1]})
    with pytest.raises(ValueError, match="together"):
        me.eval_matches(data, {**pred, "num_keypoints0": torch.tensor([3, 4])})
    with pytest.raises(ValueError, match="together"):
        me.eval_matches({**data, "num_keypoints1": torch.tensor([3, 4])}, pred)
    with pytest.raises(ValueError, match="shape"):
        me.eval_matches(data, {**pred, "num_keypoints0": torch.tensor([3]), "num_keypoints1": torch.tensor([3])})
    assert callable(me.as_export_callback(("homography",)))
