"""The wireframe step on the GPU (lightglue_amd.wireframe, csrc/wireframe.hip) -- needs an MI355X.

Every fixture of the real reference through ``lines_to_wireframe`` and through ``WireframeExtractor``
with stub extractors (integers and bools exact, floats within REF_ERR_FACTOR x the reference's own
fp32 error floored at 2 ulp); chains that a fixed sweep count would split; the capacity edge against
the numpy statement; the degenerate inputs; sampling positions; run-to-run equality; and the extractor
behind TwoViewPipeline in front of GlueStick.

Bounds that come from reasoning rather than a fixture:
* junction means and scores against the fp32 index-order sums of tests/wireframe_ref.py: the kernel
  performs the same IEEE operations in the same order, so 2 ulp of the magnitude is generous;
* descriptors against the fp64 statement: x / s - 0.5 and the four corner offsets are exact in fp32
  (s a power of two), so the error is the rounding of 4 weight products, 4 x 2 multiply-adds, the sum
  of squares, one sqrt and one division, each <= 2^-24 relative to values <= 1 in magnitude after the
  normalisation: DESC_TOL = 2e-6 covers the D <= 256 used here with room."""
import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import wireframe_ref
from wireframe_golden_util import (HEIGHT, S, ULP32, WIDTH, bar, case_names, check_against_fixture, extractor_conf, load_case,
                                   recipe_inputs, wf_conf)

pytestmark = pytest.mark.gpu

DESC_TOL = 2e-6
HOLD = {}


class StubPoints(torch.nn.Module):
    def __init__(self, conf):
        super().__init__()

    def forward(self, data):
        return {k: HOLD[k].clone() for k in ("keypoints", "keypoint_scores", "descriptors", "dense_descriptors")}


class StubLines(torch.nn.Module):
    def __init__(self, conf):
        super().__init__()

    def forward(self, data):
        return {k: HOLD[k].clone() for k in ("lines", "line_scores", "valid_lines")}


def _register():
    from lightglue_amd.pipeline import register_model

    register_model("test_stub_points", StubPoints)
    register_model("test_stub_lines", StubLines)


def _cuda(inp):
    return {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in inp.items() if k != "exact_pairs"}


def _np(pred):
    return {k: v.detach().cpu().numpy() for k, v in pred.items() if torch.is_tensor(v)}


def _run_extractor(recipe, inp, z, line_name="test_stub_lines"):
    from lightglue_amd import WireframeExtractor

    _register()
    HOLD.clear()
    HOLD.update(_cuda(inp))
    model = WireframeExtractor(extractor_conf(recipe, "test_stub_points", line_name)).eval().cuda()
    data = {"image": torch.zeros(recipe["B"], 1, HEIGHT, WIDTH, device="cuda"),
            "fill_junctions": torch.from_numpy(z["fill_junctions"]).float(), "fill_keypoints": torch.from_numpy(z["fill_keypoints"]).float()}
    if line_name is None:
        data.update({k: HOLD[k] for k in ("lines", "line_scores", "valid_lines")})
    scores_before = HOLD["line_scores"].clone()
    with torch.no_grad():
        pred = model(data)
    assert torch.equal(HOLD["line_scores"], scores_before)  # the caller's tensor is not modified
    return pred


@pytest.mark.parametrize("name", case_names())
def test_extractor_reproduces_fixture(name):
    z, meta = load_case(name)
    recipe = meta["recipe"]
    inp = recipe_inputs(recipe)
    pred = _run_extractor(recipe, inp, z)
    assert sorted(pred) == sorted(meta["output_keys"]) and "dense_descriptors" not in pred
    if recipe["forced"]:
        assert pred["num_junctions"].is_cuda and pred["num_junctions"].shape == (recipe["B"],)
    else:
        assert not pred["num_junctions"].is_cuda
    assert pred["lines_junc_idx"].dtype == torch.int64 and pred["pl_associativity"].dtype == torch.bool
    got = _np(pred)
    np.testing.assert_array_equal(got["valid_lines"], inp["valid_lines"])
    dev = check_against_fixture(z, recipe, inp, got)
    # the same through the data (line_extractor.name None)
    again = _np(_run_extractor(recipe, inp, z, line_name=None))
    for k, v in got.items():
        np.testing.assert_array_equal(again[k], v, err_msg=k)
    # coordinates against the reference's own fp32 arithmetic: index-order fp32 sums
    ref32 = wireframe_ref.wireframe(inp, wf_conf(recipe), z["fill_junctions"].astype(np.float32),
                                    z["fill_keypoints"].astype(np.float32), s=S, dtype=np.float32)
    bit_equal = all(np.array_equal(np.stack(ref32[k]), got[k]) for k in ("keypoints", "lines", "keypoint_scores"))
    print(name, "deviation / bar:", {k: (v, bar(z, k)) for k, v in dev.items()}, "coordinates and scores bit-equal to the "
          "fp32 index-order statement:", bit_equal)
    assert (pred["lines_junc_idx"] >= 0).all() and (pred["lines_junc_idx"] < pred["num_junctions"].to("cuda").view(-1, 1, 1)).all()


@pytest.mark.parametrize("name", [n for n in case_names() if n != "wf_independent_lines"])
def test_lines_to_wireframe_reproduces_fixture(name):
    from lightglue_amd import lines_to_wireframe

    z, meta = load_case(name)
    recipe = meta["recipe"]
    inp = recipe_inputs(recipe)
    B = recipe["B"]
    dense = torch.from_numpy(inp["dense_descriptors"]).cuda()
    scores = torch.from_numpy(z["out_line_scores"]).float().cuda()  # the extractor normalises them first
    fill = torch.from_numpy(z["fill_junctions"]).float().cuda() if recipe["forced"] else None
    junc, jsc, jdesc, conn, new_lines, idx, n_true = lines_to_wireframe(
        torch.from_numpy(inp["lines"]).cuda(), scores, dense, S, recipe["nms_radius"], recipe["forced"], recipe["max_num_lines"],
        fill_junctions=fill)
    n_list = n_true.tolist() if torch.is_tensor(n_true) else list(n_true)
    assert n_list == z["out_num_junctions"].ravel().tolist()
    assert torch.is_tensor(n_true) == bool(recipe["forced"])
    J = junc.shape[1]
    assert J == (2 * recipe["max_num_lines"] if recipe["forced"] else n_list[0])
    np.testing.assert_array_equal(idx.cpu().numpy(), z["out_lines_junc_idx"])
    np.testing.assert_array_equal(idx.cpu().numpy().reshape(B, -1), z["labels"])
    np.testing.assert_array_equal(conn.cpu().numpy(), z["out_pl_associativity"][:, :J, :J])
    for got, key, want in ((junc, "keypoints", z["out_keypoints"][:, :J]), (jsc, "keypoint_scores", z["out_keypoint_scores"][:, :J]),
                           (new_lines, "lines", z["out_lines"])):
        d = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        assert d <= bar(z, key), (key, d, bar(z, key))
    di = z["desc_index"]
    rows = di[:, 1] < J
    d = float(np.abs(jdesc.cpu().numpy()[di[rows, 0], di[rows, 1]].astype(np.float64) - z["desc_rows"][rows]).max())
    assert d <= bar(z, "descriptors"), (d, bar(z, "descriptors"))


def _ltw(lines, scores=None, D=16, hw=(15, 20), r=3, forced=False, max_lines=None, seed=0, fill=None):
    from lightglue_amd import lines_to_wireframe

    lines = torch.as_tensor(np.asarray(lines, np.float32)).cuda()
    B, L = lines.shape[:2]
    g = torch.Generator().manual_seed(seed)
    dense = torch.randn((B, D) + hw, generator=g).cuda()
    scores = torch.rand((B, L), generator=g).cuda() if scores is None else scores
    return lines_to_wireframe(lines, scores, dense, S, r, forced, max_lines, fill_junctions=fill), dense, scores


def _chain(order):
    pts = np.stack([4 + 2.9 * np.arange(64), np.full(64, 50.0)], 1)[order]
    return pts.reshape(1, 32, 2, 2)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_is_one_cluster(order):
    """64 endpoints 2.9 px apart on a line: one component, label 0, however the indices run; merging
    only what one or a fixed number of sweeps reaches would leave several."""
    idx = {"ascending": np.arange(64), "descending": np.arange(64)[::-1],
           "shuffled": np.random.Generator(np.random.PCG64(3)).permutation(64)}[order]
    (junc, jsc, jdesc, conn, new_lines, jidx, n_true), _, scores = _ltw(_chain(idx), hw=(15, 25))
    assert n_true == [1] and junc.shape == (1, 1, 2) and (jidx == 0).all()
    pts = _chain(idx).reshape(-1, 2).astype(np.float32)
    want = wireframe_ref.ordered_mean(pts, np.zeros(64, np.int64), 1, np.float32)
    assert np.abs(junc.cpu().numpy()[0] - want).max() <= 2 * ULP32 * 200
    assert conn.cpu().numpy().tolist() == [[[True]]]
    assert torch.equal(new_lines, junc.view(1, 1, 1, 2).expand(1, 32, 2, 2))


def test_two_chains_are_two_clusters():
    a = np.stack([4 + 2.9 * np.arange(64), np.full(64, 50.0)], 1)
    b = a + [0, 3.5]
    order = np.random.Generator(np.random.PCG64(4)).permutation(128)
    pts = np.concatenate([a, b])[order]
    (junc, _, _, conn, _, jidx, n_true), _, _ = _ltw(pts.reshape(1, 64, 2, 2), hw=(15, 25))
    assert n_true == [2]
    want, n = wireframe_ref.cluster_labels(pts.astype(np.float32), 3)
    assert n == 2
    np.testing.assert_array_equal(jidx.cpu().numpy().ravel(), want)


def _random_segments(L, width, height, r, seed):
    """L random segments whose endpoint-endpoint distances all lie outside +-1e-3 of r."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ep = (rng.random((2 * L, 2)) * [width - 1, height - 1]).astype(np.float32)
    for _ in range(100):
        p = ep.astype(np.float64)
        dx, dy = p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]
        near = np.abs(np.sqrt(dx * dx + dy * dy) - r) <= 1e-3
        bad = np.unique(np.nonzero(near)[0])
        if not len(bad):
            return ep.reshape(1, L, 2, 2)
        ep[bad] = (rng.random((len(bad), 2)) * [width - 1, height - 1]).astype(np.float32)  # move them
    raise AssertionError("could not clear the band")


@pytest.mark.parametrize("L,width,height", [(512, 160, 120), (2048, 480, 360)])
def test_capacity_edge_against_statement(L, width, height):
    """E = 1024 and the largest supported E = 4096 (several sweeps of 1024 threads per endpoint)."""
    from lightglue_amd.wireframe import MAX_LINES

    assert L <= MAX_LINES
    lines = _random_segments(L, width, height, 3, seed=L)
    (junc, jsc, jdesc, conn, new_lines, jidx, n_true), dense, scores = _ltw(lines, D=16, hw=(height // S, width // S), seed=L)
    ep = lines.reshape(-1, 2)
    labels, n = wireframe_ref.cluster_labels(ep, 3)
    assert n_true == [n] and 0.2 * len(ep) < n < len(ep) and np.bincount(labels).max() >= 4
    np.testing.assert_array_equal(jidx.cpu().numpy().ravel(), labels)
    want = wireframe_ref.ordered_mean(ep, labels, n, np.float32)
    want_s = wireframe_ref.ordered_mean(np.repeat(scores.cpu().numpy()[0], 2), labels, n, np.float32)
    got = junc.cpu().numpy()[0]
    print("L", L, "clusters", n, "junctions bit-equal:", np.array_equal(got, want))
    assert np.abs(got - want).max() <= 2 * ULP32 * width
    assert np.abs(jsc.cpu().numpy()[0] - want_s).max() <= 2 * ULP32
    np.testing.assert_array_equal(new_lines.cpu().numpy().reshape(-1, 2), got[labels])
    np.testing.assert_array_equal(conn.cpu().numpy()[0], wireframe_ref.associativity(labels.reshape(-1, 2), n))
    d = wireframe_ref.sample_descriptors(dense[0].permute(1, 2, 0).cpu().numpy(), got, S)
    assert np.abs(jdesc.cpu().numpy()[0] - d).max() <= DESC_TOL
    if L == MAX_LINES:
        with pytest.raises(ValueError, match="at most"):
            _ltw(np.zeros((1, L + 1, 2, 2), np.float32))


def _extract(inp, conf, image_hw=(HEIGHT, WIDTH), **data):
    from lightglue_amd import WireframeExtractor

    _register()
    HOLD.clear()
    HOLD.update({k: torch.as_tensor(v).cuda() for k, v in inp.items()})
    B = HOLD["keypoints"].shape[0]
    model = WireframeExtractor({"point_extractor": {"name": "test_stub_points", **conf.get("point", {})},
                                "line_extractor": {"name": None, **conf.get("line", {})},
                                "wireframe_params": conf.get("wf", {})}).eval().cuda()
    with torch.no_grad():
        return model({"image": torch.zeros((B, 1) + image_hw, device="cuda"), "lines": HOLD["lines"],
                      "line_scores": HOLD["line_scores"], **data})


def _points(B, K, D=16, seed=0, hw=(15, 20)):
    g = torch.Generator().manual_seed(seed)
    kp = torch.rand((B, K, 2), generator=g) * torch.tensor([WIDTH - 1.0, HEIGHT - 1.0])
    desc = torch.nn.functional.normalize(torch.randn((B, K, D), generator=g), dim=-1)
    return {"keypoints": kp, "keypoint_scores": torch.rand((B, K), generator=g), "descriptors": desc,
            "dense_descriptors": torch.randn((B, D) + hw, generator=g)}


def test_zero_lines():
    inp = {**_points(1, 9), "lines": torch.zeros(1, 0, 2, 2), "line_scores": torch.zeros(1, 0)}
    pred = _extract(inp, {})
    assert pred["lines"].shape == (1, 0, 2, 2) and pred["lines_junc_idx"].shape == (1, 0, 2)
    assert pred["num_junctions"].tolist() == [0]
    for k in ("keypoints", "keypoint_scores", "descriptors"):
        assert torch.equal(pred[k].cpu(), inp[k]), k
    assert torch.equal(pred["pl_associativity"].cpu(), torch.eye(9, dtype=torch.bool)[None])
    # forced: static shapes, the count on the device
    inp2 = {**_points(2, 5), "lines": torch.zeros(2, 0, 2, 2), "line_scores": torch.zeros(2, 0)}
    pred = _extract(inp2, {"point": {"force_num_keypoints": True}, "line": {"force_num_lines": True, "max_num_lines": 0}})
    assert pred["num_junctions"].is_cuda and pred["num_junctions"].tolist() == [0, 0]
    assert torch.equal(pred["keypoints"].cpu(), inp2["keypoints"])
    assert torch.equal(pred["pl_associativity"].cpu(), torch.eye(5, dtype=torch.bool)[None].repeat(2, 1, 1))


def test_one_line_and_identical_endpoints():
    (junc, jsc, jdesc, conn, new_lines, jidx, n_true), dense, scores = _ltw([[[[10.0, 20.0], [50.5, 60.25]]]])
    assert n_true == [2] and jidx.tolist() == [[[0, 1]]]
    assert torch.equal(junc.cpu(), torch.tensor([[[10.0, 20.0], [50.5, 60.25]]])) and torch.equal(new_lines.cpu()[0], junc.cpu())
    assert torch.equal(jsc, scores.repeat_interleave(2, dim=1))
    assert conn.cpu().tolist() == [[[True, True], [True, True]]]
    # every endpoint the same point: one junction there, every line a loop on it
    same = np.tile(np.array([33.25, 44.5], np.float32), (1, 7, 2, 1))
    (junc, jsc, jdesc, conn, new_lines, jidx, n_true), dense, scores = _ltw(same)
    assert n_true == [1] and (jidx == 0).all() and conn.cpu().tolist() == [[[True]]]
    assert torch.equal(junc.cpu(), torch.tensor([[[33.25, 44.5]]])) and torch.equal(new_lines.cpu(), torch.from_numpy(same))
    want = wireframe_ref.ordered_mean(np.repeat(scores.cpu().numpy()[0], 2), np.zeros(14, np.int64), 1, np.float32)
    assert abs(float(jsc[0, 0]) - float(want[0])) <= 2 * ULP32
    d = wireframe_ref.sample_descriptors(dense[0].permute(1, 2, 0).cpu().numpy(), junc.cpu().numpy()[0], S)
    assert np.abs(jdesc.cpu().numpy()[0] - d).max() <= DESC_TOL


def test_keypoint_on_an_endpoint_and_at_the_radius():
    """Distance 0 goes, exactly the radius stays (strict <), just inside goes; forced mode replaces in
    place with the caller's row, zero score and a sampled descriptor."""
    lines = torch.tensor([[[[40.0, 40.0], [100.0, 40.0]], [[100.0, 43.5], [100.0, 90.0]]]])
    inp = {**_points(1, 6, seed=2), "lines": lines, "line_scores": torch.tensor([[0.5, 1.0]])}
    inp["keypoints"][0, :4] = torch.tensor([[40.0, 40.0], [40.0, 43.0], [40.0, 42.9990], [100.0, 93.0]])
    inp["keypoints"][0, 4:] = torch.tensor([[70.0, 70.0], [10.0, 10.0]])
    want_removed = [True, False, True, False, False, False]
    free = _extract(inp, {})
    assert free["num_junctions"].tolist() == [4]  # (100, 40) and (100, 43.5) are 3.5 apart: no merge
    keep = ~torch.tensor(want_removed)
    assert torch.equal(free["keypoints"].cpu()[0, 4:], inp["keypoints"][0][keep])
    assert torch.equal(free["keypoint_scores"].cpu()[0, 4:], inp["keypoint_scores"][0][keep])
    assert torch.equal(free["descriptors"].cpu()[0, 4:], inp["descriptors"][0][keep])
    assert free["pl_associativity"].shape == (1, 8, 8)
    fill = torch.tensor([[[5.0, 6.0], [7.0, 8.0], [150.0, 110.0], [1.0, 2.0], [3.0, 4.0], [9.0, 9.0]]])
    forced = _extract(inp, {"point": {"force_num_keypoints": True}, "line": {"force_num_lines": True, "max_num_lines": 3}},
                      fill_keypoints=fill, fill_junctions=torch.full((1, 6, 2), 77.0))
    assert forced["num_junctions"].tolist() == [4] and forced["keypoints"].shape == (1, 12, 2)
    assert torch.equal(forced["keypoints"].cpu()[0, 4:6], torch.full((2, 2), 77.0)) and (forced["keypoint_scores"][0, 4:6] == 0).all()
    kp = forced["keypoints"].cpu()[0, 6:]
    rem = torch.tensor(want_removed)
    assert torch.equal(kp[rem], fill[0][rem]) and torch.equal(kp[~rem], inp["keypoints"][0][~rem])
    assert (forced["keypoint_scores"].cpu()[0, 6:][rem] == 0).all()
    assert torch.equal(forced["descriptors"].cpu()[0, 6:][~rem], inp["descriptors"][0][~rem])
    dense = inp["dense_descriptors"][0].permute(1, 2, 0).numpy()
    d = wireframe_ref.sample_descriptors(dense, forced["keypoints"].cpu().numpy()[0], S)
    sampled = np.r_[np.ones(6, bool), rem.numpy()]
    assert np.abs(forced["descriptors"].cpu().numpy()[0][sampled] - d[sampled]).max() <= DESC_TOL
    eye = np.eye(12, dtype=bool)
    eye[[0, 1, 2, 3], [1, 0, 3, 2]] = True
    np.testing.assert_array_equal(forced["pl_associativity"].cpu().numpy()[0], eye)


@pytest.mark.parametrize("D", [4, 64, 256, 1024])
def test_sampling_positions(D):
    """Cell centres (one cell, weight 1), cell corners (four cells at 1/4), the half-cell border where
    zero padding enters, and positions outside the map (zero descriptor), NaN and infinity included."""
    from lightglue_amd import sample_descriptors_corner_conv

    g = torch.Generator().manual_seed(D)
    dense = torch.randn((2, D, 15, 20), generator=g)
    pts = [[4.0, 4.0], [12.0, 20.0], [156.0, 116.0], [8.0, 8.0], [80.0, 64.0], [0.0, 0.0], [160.0, 120.0], [-3.0, 50.0],
           [50.0, -3.9], [163.0, 119.0], [-4.0, 10.0], [-20.0, 10.0], [10.0, 500.0], [1e9, 1e9], [float("nan"), 5.0],
           [float("inf"), 5.0], [3.7, 101.3], [77.77, 55.55]]
    pts = torch.tensor([pts, pts[::-1]])
    got = sample_descriptors_corner_conv(pts.cuda(), dense.cuda(), S)
    assert got.shape == (2, D, pts.shape[1])
    got = got.transpose(1, 2).cpu().numpy()
    with np.errstate(invalid="ignore"):
        for b in range(2):
            want = wireframe_ref.sample_descriptors(dense[b].permute(1, 2, 0).numpy(), pts[b].numpy(), S)
            assert np.abs(got[b] - want).max() <= DESC_TOL
    centre = torch.nn.functional.normalize(dense[0, :, 0, 0], dim=0).numpy()
    assert np.abs(got[0, 0] - centre).max() <= DESC_TOL
    outside = [10, 11, 12, 13, 14, 15]
    assert (got[0, outside] == 0).all()
    # the extractors' layout (an NHWC tensor seen as [B, D, Hc, Wc]) is read in place and gives the same
    view = dense.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    again = sample_descriptors_corner_conv(pts.cuda(), view, S)
    assert torch.equal(again.cpu().transpose(1, 2), torch.from_numpy(got))


def test_run_to_run_identical():
    z, meta = load_case("wf_forced_b2")
    recipe = meta["recipe"]
    inp = recipe_inputs(recipe)
    a, b = _run_extractor(recipe, inp, z), _run_extractor(recipe, inp, z)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    lines = _random_segments(512, 160, 120, 3, seed=9)
    (ra, _, _), (rb, _, _) = _ltw(lines, D=64), _ltw(lines, D=64)
    for x, y in zip(ra[:6], rb[:6]):
        assert torch.equal(x, y)
    assert ra[6] == rb[6]


def _views(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    views = {}
    for v in "01":
        image = torch.rand((B, 1, HEIGHT, WIDTH), generator=g)
        a = torch.rand((B, L, 1, 2), generator=g) * torch.tensor([WIDTH - 41.0, HEIGHT - 41.0]) + 20
        lines = torch.cat([a, a + (torch.rand((B, L, 1, 2), generator=g) - 0.5) * 40], dim=2)
        lines[:, 1::2, 0] = lines[:, 0:-1:2, 1] + 0.5  # every second line starts where the one before ends
        views["view" + v] = {"image": image.cuda(), "lines": lines.cuda(), "line_scores": (torch.rand((B, L), generator=g) + 0.1).cuda(),
                             "image_size": torch.tensor([[float(WIDTH), float(HEIGHT)]] * B).cuda()}
    return views


@pytest.mark.parametrize("forced", [False, True])
def test_two_view_pipeline_equals_components(forced):
    """superpoint + given segments -> lines.wireframe -> matchers.gluestick behind TwoViewPipeline
    returns exactly what the three components return when called by hand."""
    from lightglue_amd import GlueStick, SuperPoint, WireframeExtractor, pipeline
    from lightglue_amd.gs_weights import gluestick_state_dict

    B, L = (2, 12) if forced else (1, 14)
    sp_conf = {"name": "gluefactory_nonfree.superpoint", "dense_outputs": True, "detection_threshold": 0.0,
               "max_num_keypoints": 64, "force_num_keypoints": forced}
    ext_conf = {"name": "lines.wireframe", "point_extractor": sp_conf,
                "line_extractor": {"name": None, "force_num_lines": forced, "max_num_lines": L if forced else None}}
    layers = {"GNN_layers": ["self", "cross"] * 2}
    gs_conf = {"name": "matchers.gluestick", **layers}
    torch.manual_seed(5)
    pipe = pipeline.get_model("two_view_pipeline")({"extractor": ext_conf, "matcher": gs_conf}).eval().cuda()
    assert isinstance(pipe.extractor, WireframeExtractor) and isinstance(pipe.extractor.point_extractor, SuperPoint)
    assert isinstance(pipe.matcher, GlueStick)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in gluestick_state_dict(layers, seed=2).items()}
    pipe.matcher.load_state_dict(sd, strict=True)
    data = _views(B, L, seed=21)
    if forced:  # the random rows are the caller's, so that both routes see the same ones
        g = torch.Generator().manual_seed(8)
        for v in "01":
            data["view" + v]["fill_keypoints"] = torch.rand((B, 64, 2), generator=g) * 100
            data["view" + v]["fill_junctions"] = torch.rand((B, 2 * L, 2), generator=g) * 100
    with torch.no_grad():
        pred = pipe(data)
        by_hand = {}
        for v in "01":
            view = data["view" + v]
            pts = pipe.extractor.point_extractor(view)
            assert "dense_descriptors" in pts
            wf = pipe.extractor(view)
            K = pts["keypoints"].shape[1]
            if forced:
                assert wf["keypoints"].shape == (B, 2 * L + K, 2) and wf["num_junctions"].is_cuda
            n = int(wf["num_junctions"][0])
            assert 0 < n < 2 * L  # the touching lines share junctions
            assert (wf["lines_junc_idx"] >= 0).all()
            assert (wf["lines_junc_idx"] < wf["num_junctions"].to("cuda").view(-1, 1, 1)).all()
            by_hand.update({k + v: t for k, t in wf.items()})
        by_hand.update(pipe.matcher({**data, **by_hand}))
    assert sorted(pred) == sorted(by_hand)
    for k, t in by_hand.items():
        assert torch.equal(pred[k], t), k
    assert "line_matches0" in pred and pred["line_matches0"].shape == (B, L)
