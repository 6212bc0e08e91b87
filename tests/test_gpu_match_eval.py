"""Batched match evaluation on the device (lightglue_amd.match_eval, csrc/match_eval.hip) -- needs an
MI355X.  Every case of the reference's fixture (tests/golden/match_eval/match_eval.npz): counts exactly, ratios
bit-equal to count / n in fp32, the DLT error within the fixture's ``dlt_rel_bar`` of its fp64 value
(the fp32 host path's own worst deviation: tests/golden/make_match_eval_golden.py); the ragged batch
against its pairs alone, poisoned padding, flag subsets, the unbatched form, run-to-run bits, untouched
outputs, and the matcher's own ``pred`` through TwoViewPipeline against tests/match_eval_ref.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import match_eval_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_eval", "match_eval.npz")
CASES = "abcdefghij"
HOM_KEYS = ("prec@1px", "prec@3px")
EPI_KEYS = ("epi_prec@1e-4", "epi_prec@5e-4", "epi_prec@1e-3")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def case_inputs(g, name, rows=None):
    """(data, pred) of a fixture case on the device; ``rows`` picks pairs."""
    def t(key):
        v = torch.from_numpy(g[f"{name}/{key}"])
        return (v if rows is None else v[rows]).cuda()

    pred = {"keypoints0": t("kpts0"), "keypoints1": t("kpts1"), "matches0": t("matches0"),
            "matching_scores0": t("scores0")}
    if f"{name}/num0" in g:
        pred["num_keypoints0"], pred["num_keypoints1"] = t("num0"), t("num1")
    data = {"H_0to1": t("H"), "T_0to1": t("T"), "view0": {"image_size": t("size0"), "camera": t("cam0")},
            "view1": {"camera": t("cam1")}}
    return data, pred


def same(a, b):
    """Bit equality of two result dicts (NaN equal to NaN)."""
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].nan_to_num(nan=-7.0), b[k].nan_to_num(nan=-7.0)), k


@pytest.mark.parametrize("name", list(CASES))
def test_every_fixture_case(golden, name):
    from lightglue_amd import hpatches_metrics, match_eval as me

    data, pred = case_inputs(golden, name)
    out = me.eval_matches(data, pred)
    B, M = pred["matches0"].shape
    N = pred["keypoints1"].shape[1]
    hc, ec = torch.from_numpy(golden[f"{name}/hom_counts"]), torch.from_numpy(golden[f"{name}/epi_counts"])
    n = hc[:, 0].float()
    assert out["num_matches"].dtype == torch.int32 and torch.equal(out["num_matches"].cpu(), hc[:, 0])
    assert torch.equal(ec[:, 0], hc[:, 0])
    for j, k in enumerate(HOM_KEYS):  # counts exactly: the ratio is count / n in fp32, bit for bit
        assert out[k].dtype == torch.float32 and torch.equal(out[k].cpu(), (hc[:, j + 1].float() / n).nan_to_num()), k
        assert torch.equal((out[k].cpu() * n).round().int(), hc[:, j + 1]), k
    for j, k in enumerate(EPI_KEYS):
        want = ec[:, j + 1].float() / n
        assert torch.equal(out[k].cpu().nan_to_num(nan=-7.0), want.nan_to_num(nan=-7.0)), k
    if "num_keypoints0" in pred:
        nkp = (pred["num_keypoints0"] + pred["num_keypoints1"]).float().cpu() / 2
    else:
        nkp = torch.full((B,), (M + N) / 2.0)
    assert torch.equal(out["num_keypoints"].cpu(), nkp)

    bar = float(golden["dlt_rel_bar"])
    err, Hd = out["H_error_dlt"].double().cpu(), out["H_dlt"].double().cpu()
    assert Hd.shape == (B, 3, 3) and err.shape == (B,)
    for b in range(B):
        want, Hw = float(golden[f"{name}/dlt_err64"][b]), torch.from_numpy(golden[f"{name}/H_dlt64"][b])
        rel = abs(float(err[b]) - want) / want if want == want else 0.0
        print(f"case {name}[{b}]: H_error_dlt {float(err[b]):.9g}, fp64 host {want:.9g}, rel {rel:.3e}, bar {bar:.3e}; "
              f"H_dlt max dev / max entry {float((Hd[b] - Hw).abs().max() / Hw.abs().max()):.3e}")
        if int(hc[b, 0]) < 4:  # what the host function returns: an all-inf homography, the error NaN
            host = hpatches_metrics.eval_homography_dlt(
                {"H_0to1": data["H_0to1"][b].cpu(), "view0": {"image_size": data["view0"]["image_size"][b].cpu()}},
                {"keypoints0": pred["keypoints0"][b].cpu(), "keypoints1": pred["keypoints1"][b].cpu(),
                 "matches0": pred["matches0"][b].cpu(), "matching_scores0": pred["matching_scores0"][b].cpu()})
            np.testing.assert_equal(float(out["H_error_dlt"][b]), host["H_error_dlt"])  # NaN == NaN here
            assert np.isnan(want) and torch.isinf(Hd[b]).all() and (Hd[b] > 0).all()
        else:
            assert abs(float(err[b]) - want) <= bar * want
            assert float((Hd[b] - Hw).abs().max()) <= bar * float(Hw.abs().max())


def test_ragged_batch_equals_its_pairs_alone_and_ignores_poisoned_padding(golden):
    from lightglue_amd import match_eval as me

    data, pred = case_inputs(golden, "i")
    out = me.eval_matches(data, pred)
    num0, num1 = golden["i/num0"], golden["i/num1"]
    for b, name in enumerate("abc"):
        d1, p1 = case_inputs(golden, name)
        assert p1["keypoints0"].shape[1] == num0[b] and p1["keypoints1"].shape[1] == num1[b]
        alone = me.eval_matches(d1, p1)
        for k in out:
            assert torch.equal(out[k][b].nan_to_num(nan=-7.0), alone[k][0].nan_to_num(nan=-7.0)), (name, k)
    poisoned = {k: v.clone() for k, v in pred.items()}
    for b in range(3):
        poisoned["keypoints0"][b, num0[b]:] = float("nan")
        poisoned["keypoints1"][b, num1[b]:] = float("nan")
        poisoned["matching_scores0"][b, num0[b]:] = float("nan")
        poisoned["matches0"][b, num0[b]:] = torch.tensor([10**12, -5, 2**31, 130] * 17)[: 65 - num0[b]].cuda()
    same(me.eval_matches(data, poisoned), out)
    # a match index at or beyond the partner count is no match (well-formed input never has one)
    bad = {k: v.clone() for k, v in pred.items()}
    live = torch.nonzero(bad["matches0"][1, :num0[1]] > -1)[0, 0]
    bad["matches0"][1, live] = int(num1[1])
    assert int(me.eval_matches(data, bad)["num_matches"][1]) == int(out["num_matches"][1]) - 1


def test_flag_subsets_unbatched_form_and_repeatability(golden):
    from lightglue_amd import match_eval as me

    data, pred = case_inputs(golden, "j")
    out = me.eval_matches(data, pred)
    same(me.eval_matches(data, pred), out)  # run to run
    parts = {}
    for fn in (me.eval_matches_homography, me.eval_matches_epipolar, me.eval_homography_dlt):
        r = fn(data, pred)
        same({k: out[k] for k in r}, r)
        parts.update(r)
    assert parts.keys() == out.keys()
    assert set(me.eval_matches_homography(data, pred)) == {"prec@1px", "prec@3px", "num_matches", "num_keypoints"}
    assert set(me.eval_matches_epipolar(data, pred)) == {*EPI_KEYS, "num_matches", "num_keypoints"}
    assert set(me.eval_homography_dlt(data, pred)) == {"H_error_dlt", "H_dlt"}
    same(me.eval_matches(data, pred, ("dlt", "epipolar")), {k: out[k] for k in out if k not in HOM_KEYS})
    # the reference's wrappers' form (an object with _data), a [B,4,4] pose, extra distortion columns
    from lightglue_amd.depth_matcher import Camera, Pose

    T44 = torch.eye(4, device="cuda").repeat(2, 1, 1)
    T44[:, :3, :3], T44[:, :3, 3] = data["T_0to1"][:, :9].reshape(2, 3, 3), data["T_0to1"][:, 9:]
    alt = {**data, "T_0to1": T44, "view0": {**data["view0"], "camera": Camera(data["view0"]["camera"])},
           "view1": {"camera": torch.cat([data["view1"]["camera"], torch.ones(2, 2, device="cuda")], 1)}}
    same(me.eval_matches(alt, pred), out)
    same(me.eval_matches({**data, "T_0to1": Pose(data["T_0to1"])}, pred), out)
    # one pair without the batch dimension: Python numbers, element 0 of the batched form
    d0 = {"H_0to1": data["H_0to1"][0], "T_0to1": data["T_0to1"][0],
          "view0": {"image_size": data["view0"]["image_size"][0], "camera": data["view0"]["camera"][0]},
          "view1": {"camera": data["view1"]["camera"][0]}}
    one = me.eval_matches(d0, {k: v[0] for k, v in pred.items()})
    assert one.keys() == out.keys()
    for k, v in one.items():
        if k == "H_dlt":
            assert v.shape == (3, 3) and torch.equal(v, out[k][0])
        else:
            assert isinstance(v, int if k == "num_matches" else float) and v == out[k][0].item(), k


def test_outputs_no_flag_names_stay_untouched(golden):
    from lightglue_amd import _lib

    data, pred = case_inputs(golden, "b")
    lib = _lib.load()
    B, M = pred["matches0"].shape
    N = pred["keypoints1"].shape[1]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    cam0, cam1 = data["view0"]["camera"].contiguous(), data["view1"]["camera"].contiguous()
    for flags in range(1, 8):
        hc = torch.full((B, 3), -77, dtype=torch.int32, device="cuda")
        ec = torch.full((B, 4), -77, dtype=torch.int32, device="cuda")
        Hd = torch.full((B, 9), -123.5, device="cuda")
        He = torch.full((B,), -123.5, device="cuda")
        rc = lib.lg_eval_matches(ptr(pred["keypoints0"]), ptr(pred["keypoints1"]), ptr(pred["matches0"]),
                                 ptr(pred["matching_scores0"]), B, M, N, None, None, ptr(data["H_0to1"]), ptr(cam0),
                                 ptr(cam1), ptr(data["T_0to1"]), ptr(data["view0"]["image_size"]), flags, ptr(hc),
                                 ptr(ec), ptr(Hd), ptr(He), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.LG_OK, lib.lg_last_error()
        torch.cuda.synchronize()
        assert bool((hc == -77).all()) == (not flags & 1), flags
        assert bool((ec == -77).all()) == (not flags & 2), flags
        assert bool((Hd == -123.5).all()) == (not flags & 4) and bool((He == -123.5).all()) == (not flags & 4), flags
        if flags & 1:
            assert torch.equal(hc.cpu(), torch.from_numpy(golden["b/hom_counts"]))
        if flags & 2:
            assert torch.equal(ec.cpu(), torch.from_numpy(golden["b/epi_counts"]))


def test_matcher_output_goes_straight_into_the_evaluation():
    """TwoViewPipeline with the LightGlue matcher on a synthetic homography batch (B = 3, N = 128): its
    ``pred`` is evaluated on the device as it is, and each pair equals the float64 restatement."""
    from golden_util import case_inputs as weight_inputs, load
    from lightglue_amd import match_eval as me, pipeline
    from lightglue_amd.weights import synthetic_pair

    conf, sd, _ = weight_inputs(load("tiny_ragged_b2")["meta"])
    pipe = pipeline.get_model("two_view_pipeline")({"matcher": {"name": "matchers.lightglue", **conf}}).eval().cuda()
    pipe.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    B, n = 3, 128
    pair = synthetic_pair(B=B, M=n, N=n, dim=conf.get("input_dim", 256), seed=5, width=640, height=480, kpt_noise=0.7)
    H = torch.tensor([[[1.02, 0.03, 8.0], [-0.02, 0.97, -5.0], [2e-5, -3e-5, 1.0]],
                      [[0.95, -0.05, 20.0], [0.04, 1.03, 3.0], [-4e-5, 1e-5, 1.0]],
                      [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])
    k1 = torch.from_numpy(pair["keypoints1"]).double()
    k1 = torch.cat([k1, torch.ones(B, n, 1, dtype=torch.float64)], -1) @ H.double().transpose(1, 2)
    pair["keypoints1"] = (k1[..., :2] / k1[..., 2:]).float().numpy()
    size = torch.tensor([[640.0, 480.0]]).repeat(B, 1).cuda()
    data = {"H_0to1": H.cuda(), "name": ["p/0", "p/1", "p/2"]}
    for i in (0, 1):
        data[f"view{i}"] = {"image_size": size, "scales": torch.ones(B, 2, device="cuda"),
                            "cache": {"keypoints": torch.from_numpy(pair[f"keypoints{i}"]).cuda(),
                                      "descriptors": torch.from_numpy(pair[f"descriptors{i}"]).cuda()}}
    with torch.no_grad():
        pred = pipe(data)
    assert pred["matches0"].is_cuda and pred["matches0"].shape == (B, n)
    out = me.eval_matches(data, pred, ("homography", "dlt"))
    assert all(v.is_cuda for v in out.values())
    cb = me.as_export_callback(("homography", "dlt"))(pred, data)
    same(cb, out)
    for b in range(B):
        r = ref.evaluate_pair(pred["keypoints0"][b].cpu(), pred["keypoints1"][b].cpu(), pred["matches0"][b].cpu(),
                              pred["matching_scores0"][b].cpu(), H=H[b], image_size=size[b].cpu())
        print(f"pair {b}: {r['n']} matches, counts {r['hom_counts']}, H_error_dlt {r.get('H_error_dlt')}")
        assert int(out["num_matches"][b]) == r["n"]
        nf = torch.tensor(float(r["n"]))
        for j, k in enumerate(HOM_KEYS):
            assert float(out[k][b]) == float((torch.tensor(float(r["hom_counts"][j])) / nf).nan_to_num()), (b, k)
        if r["n"] < 4:
            assert torch.isnan(out["H_error_dlt"][b]) and torch.isinf(out["H_dlt"][b]).all()
        else:
            # both sides are fp64 on the same fp32 inputs; the result is rounded to fp32 once
            assert abs(float(out["H_error_dlt"][b]) - r["H_error_dlt"]) <= 1e-6 * r["H_error_dlt"] + 1e-9
            # up to scale: h / (h22 + 1e-8) depends on the sign the solver returns h with
            got, want = out["H_dlt"][b].double().cpu(), r["H_dlt"]
            got, want = got / got[2, 2], want / want[2, 2]
            assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert int(out["num_matches"].sum()) > 0
