"""The pose-and-depth line ground truth on the device (lightglue_amd.line_gt, csrc/gt_lines.hip) against
the fixtures the reference produced (tests/golden/make_line_gt_depth_golden.py) -- needs an MI355X.

Bars: stage A equal to the fixture on decided entries and lines and inside the recorded bounds elsewhere,
the exact fixtures bit for bit; stage B on the fixture's own stage-A arrays equal to the reference's labels
with no gating; end to end bit for bit on the exact fixtures, on the random ones equal to the reference for
every pair without anything undecidable and to the restated stage B on the device's own stage-A outputs
for every pair; small shapes (the exact recipe, whose every step is exact in fp32) equal to the
restatement's CPU path; the pipeline's loss from ground truth to value bit-identical to ``GlueStick.loss``
on the same tensors."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import gt_depth_ref as GD
import lgamd  # noqa: F401
import line_gt_depth_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_line_gt_depth_golden import exact_case  # noqa: E402  (a NumPy recipe; the reference is not touched)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAMES = R.fixture_names()
RANDOM = [n for n in NAMES if not R.load_fixture(n)[1]["exact"]]
LABELS = ("positive", "m0", "m1")


def _lg():
    from lightglue_amd import line_gt

    return line_gt


def _dev(g, *keys):
    return [torch.from_numpy(np.asarray(g[k])).to(DEV) for k in keys]


def _np(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _keyed(a):
    """The device's stage-A dict under the fixtures' names, as NumPy."""
    torch.cuda.synchronize()
    names = ("num_close_pts0", "num_close_pts1_t") + R.STAGE_A_KEYS[2:]
    return {k: a[n].cpu().numpy() for k, n in zip(R.STAGE_A_KEYS, names)}


@functools.lru_cache(maxsize=None)
def _stage_a(name):
    """One device run of stage A per fixture, shared by the tests below (read-only)."""
    g, meta = R.load_fixture(name)
    out = _lg().close_point_counts_from_pose_depth(*_dev(g, "lines0", "lines1"), R.feed_of(g, meta, device=DEV), meta["npts"],
                                                   meta["dist_th"], meta["min_visibility_th"])
    return out, _keyed(out)


@functools.lru_cache(maxsize=None)
def _end_to_end(name):
    g, meta = R.load_fixture(name)
    out = _lg().gt_line_matches_from_pose_depth(*_dev(g, "lines0", "lines1", "valid_lines0", "valid_lines1"),
                                                R.feed_of(g, meta, device=DEV), **R.call_kw(meta))
    return out, _np(out)


# ------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", NAMES)
def test_stage_a(name):
    g, meta = R.load_fixture(name)
    dev, got = _stage_a(name)
    B, n0, n1 = meta["B"], meta["n0"], meta["n1"]
    shapes = {"num_close_pts0": (B, n0, n1), "num_close_pts1_t": (B, n0, n1), "out_of0": (B, n1), "out_of1": (B, n0),
              "ignore_depth0": (B, n0), "ignore_depth1": (B, n1), "num_visible0": (B, n0), "num_visible1": (B, n1)}
    assert {k: tuple(v.shape) for k, v in dev.items()} == shapes
    for k, v in dev.items():
        assert v.dtype == (torch.uint8 if k.startswith("num_") else torch.bool), k
    if not meta["exact"]:
        for k, und in (("cnt0", "und0"), ("cnt1t", "und1t")):
            print(f"{name} {k}: {int((got[k] != g[k]).sum())} entries differ from the fp32 reference, "
                  f"{int((g[und] > 0).sum())} undecidable, {int((g[k] > 0).sum())} nonzero")
    R.check_stage_a(got, g, meta)


@pytest.mark.parametrize("name", NAMES)
def test_stage_b_labels_from_the_fixture_arrays(name):
    g, meta = R.load_fixture(name)
    out = _lg().line_labels_from_visibility_counts(*_dev(g, *R.STAGE_A_KEYS, "valid_lines0", "valid_lines1"), meta["npts"],
                                                   meta["overlap_th"])
    assert out[0].dtype == torch.bool and out[1].dtype == out[2].dtype == torch.int64
    R.check_labels(_np(out), g)


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end(name):
    g, meta = R.load_fixture(name)
    dev, got = _end_to_end(name)
    assert dev[0].dtype == torch.bool and dev[1].dtype == dev[2].dtype == torch.int64
    if meta["exact"]:
        R.check_labels(got, g)
        return
    decided = R.pair_decided(g, meta)
    print(f"{name}: {int(decided.sum())} of {meta['B']} pairs without anything undecidable")
    assert decided.sum() >= 1
    R.check_labels(got, g, pairs=decided)
    # every pair: the restated stage B on the device's own stage-A outputs
    want = R.stage_b_of(_stage_a(name)[1], g["valid_lines0"], g["valid_lines1"], meta["npts"], meta["overlap_th"])
    for x, w, k in zip(got, want[:3], LABELS):
        np.testing.assert_array_equal(x, w.numpy(), err_msg=k)


@pytest.mark.parametrize("name", NAMES)
def test_structure_of_the_labels(name):
    g, _ = R.load_fixture(name)
    _, (pos, m0, m1) = _end_to_end(name)
    _, a = _stage_a(name)
    assert pos.sum(2).max() <= 1 and pos.sum(1).max() <= 1
    np.testing.assert_array_equal(m0 == -2, ~g["valid_lines0"] | a["ignore_depth0"])
    np.testing.assert_array_equal(m1 == -2, ~g["valid_lines1"] | a["ignore_depth1"])
    for b in range(pos.shape[0]):
        i = np.nonzero(m0[b] >= 0)[0]
        np.testing.assert_array_equal(m1[b][m0[b][i]], i)
        j = np.nonzero(m1[b] >= 0)[0]
        np.testing.assert_array_equal(m0[b][m1[b][j]], j)
        np.testing.assert_array_equal(np.argwhere(pos[b]), np.stack([i, m0[b][i]], 1))
    assert pos.any()


def test_the_homography_entries_still_give_their_fixture_results():
    import line_gt_ref as LR

    name = "line_gt_exact_b3_n64_n48"
    g, meta = LR.load_fixture(name)
    out = _lg().line_labels_from_counts(*_dev(g, "cnt0", "cnt1t", "out_of0", "out_of1", "valid_lines0", "valid_lines1"),
                                        meta["npts"], meta["overlap_th"])
    LR.check_labels(_np(out), g)
    out = _lg().gt_line_matches_from_homography(*_dev(g, "lines0", "lines1", "valid_lines0", "valid_lines1"), meta["shape"],
                                                meta["shape"], *_dev(g, "H_0to1"), meta["npts"], meta["dist_th"],
                                                meta["overlap_th"], meta["min_visibility_th"])
    LR.check_labels(_np(out), g)


# ------------------------------------------------------------------ small shapes: the exact recipe
@functools.lru_cache(maxsize=None)
def _scene(seed, B, n0, n1, S=128, lengths=(8, 16, 24, 32)):
    g, shape, _ = exact_case(seed, B, n0, n1, S=S, lengths=lengths)
    return g, {"image_shape0": list(shape), "image_shape1": list(shape)}


def _both(g, meta, npts=33, image=True, **kw):
    """(device labels, device stage A, restated labels, restated stage A) of one scene."""
    kw = {"npts": npts, "dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.5, **kw}
    lines = _dev(g, "lines0", "lines1", "valid_lines0", "valid_lines1")
    data = R.feed_of(g, meta, device=DEV, image=image)
    a = _keyed(_lg().close_point_counts_from_pose_depth(lines[0], lines[1], data, kw["npts"], kw["dist_th"], kw["min_visibility_th"]))
    got = _np(_lg().gt_line_matches_from_pose_depth(*lines, data, **kw))
    cpu = [t.cpu() for t in lines]
    cdata = R.feed_of(g, meta, image=image)
    ca = R.stage_a(cpu[0], cpu[1], cdata, kw["npts"], kw["dist_th"], kw["min_visibility_th"])
    want = R.gt_line_matches_from_pose_depth(*cpu, cdata, **kw)
    return got, a, [w.numpy() for w in want], {k: v.numpy() for k, v in ca.items()}


def _assert_equal(got, a, want, ca, label=""):
    for k in R.STAGE_A_KEYS:
        np.testing.assert_array_equal(a[k].astype(np.int64), ca[k].astype(np.int64), err_msg=f"{label} {k}")
    for x, w, k in zip(got, want, LABELS):
        assert x.dtype == w.dtype, (label, k)
        np.testing.assert_array_equal(x, w, err_msg=f"{label} {k}")


@pytest.mark.parametrize("n0, n1", [(1, 1), (17, 15), (15, 17), (16, 33)])
def test_tile_edges_and_both_transposes_of_the_solver(n0, n1):
    g, meta = _scene(5, 2, n0, n1)
    got, a, want, ca = _both(g, meta)
    _assert_equal(got, a, want, ca)
    if n0 > 1:
        assert want[0].any() and ca["ignore_depth0"].any() | ca["ignore_depth1"].any()


@pytest.mark.parametrize("npts, S, lengths", [(2, 128, (8, 16, 24, 32)), (255, 512, (254,))])
def test_fewest_and_most_samples(npts, S, lengths):
    g, meta = _scene(6, 1, 20, 22, S, lengths)
    got, a, want, ca = _both(g, meta, npts=npts)
    _assert_equal(got, a, want, ca)
    assert ca["num_visible0"].max() == npts and want[0].any()


def test_a_pair_alone_equals_itself_inside_a_batch():
    g, meta = _scene(7, 1, 23, 19)
    one = _both(g, meta)
    _assert_equal(*one)
    g3 = {k: np.concatenate([v, v, v]) for k, v in g.items()}
    got3, a3, _, _ = _both(g3, meta)
    for b in range(3):
        for x, y in zip(got3, one[0]):
            np.testing.assert_array_equal(x[b], y[0])
        for k in R.STAGE_A_KEYS:
            np.testing.assert_array_equal(a3[k][b], one[1][k][0])


def test_empty_sides_give_the_reference_tuple():
    g, meta = _scene(7, 1, 23, 19)
    l0, l1, v0, v1 = _dev(g, "lines0", "lines1", "valid_lines0", "valid_lines1")
    l0, l1, v0, v1 = (torch.cat([t, t]) for t in (l0, l1, v0, v1))  # B = 2; the data is not read
    data = R.feed_of(g, meta, device=DEV)
    for a, b, va, vb in ((l0[:, :0], l1, v0[:, :0], v1), (l0, l1[:, :0], v0, v1[:, :0]), (l0[:, :0], l1[:, :0], v0[:, :0], v1[:, :0])):
        out = _lg().gt_line_matches_from_pose_depth(a, b, va, vb, data)
        want = R.gt_line_matches_from_pose_depth(a.cpu(), b.cpu(), va.cpu(), vb.cpu(), None)
        for x, w, k in zip(out, want, LABELS):
            assert tuple(x.shape) == tuple(w.shape) and x.dtype == w.dtype and x.device.type == "cuda", k
            assert torch.equal(x.cpu(), w), k
        assert out[1].dtype == torch.int64 and tuple(out[1].shape) == (2, a.shape[1]) and tuple(out[2].shape) == (2, b.shape[1])


def test_degenerate_inputs():
    g, meta = _scene(8, 2, 21, 18)
    base = _both(g, meta)
    _assert_equal(*base)
    assert base[0][0].any()
    # all lines invalid
    inv = {**g, "valid_lines0": np.zeros_like(g["valid_lines0"]), "valid_lines1": np.zeros_like(g["valid_lines1"])}
    got, a, want, ca = _both(inv, meta)
    _assert_equal(got, a, want, ca, "invalid")
    assert not got[0].any() and (got[1] == -2).all() and (got[2] == -2).all()
    # an all-zero depth map: every line of that image ignored, nothing NaN-poisoned into `positive`
    for k in ("depth0", "depth1"):
        dark = {**g, k: np.zeros_like(g[k])}
        got, a, want, ca = _both(dark, meta)
        _assert_equal(got, a, want, ca, "dark " + k)
        s = k[-1]
        assert a["ignore_depth" + s].all() and (a["num_visible" + s] == 0).all() and not got[0].any()
        assert (got[1 + int(s)] == -2).all() and not (got[2 - int(s)] >= 0).any()
    # a pose that takes every sample behind the camera, and one that takes it out of the image
    for label, t in (("behind", [0.0, 0.0, -8.0]), ("aside", [64.0, 0.0, 0.0])):
        T = np.tile(np.concatenate([np.eye(3).reshape(9), t]).astype(np.float32), (2, 1))
        away = {**g, "T_0to1": T, "T_1to0": T}
        got, a, want, ca = _both(away, meta)
        _assert_equal(got, a, want, ca, label)
        assert (a["num_visible0"] == 0).all() and (a["num_visible1"] == 0).all() and not got[0].any() and (got[1] != -2).any()
        assert (got[1] < 0).all() and (got[2] < 0).all()
        if label == "aside":
            assert a["out_of1"][~a["ignore_depth0"]].all()
    # a zero-length line: NaNs in its direction, so nothing is close to it
    z = {**g, "lines0": g["lines0"].copy()}
    z["lines0"][:, 0, 2:] = z["lines0"][:, 0, :2] = [40.0, 50.0]
    got, a, want, ca = _both(z, meta)
    _assert_equal(got, a, want, ca, "zero length")
    assert (a["cnt0"][:, 0] == 0).all() and not got[0][:, 0].any()


def test_image_size_differs_from_the_depth_map_and_the_fallback_without_images():
    g, meta = _scene(9, 2, 24, 20)
    full = _both(g, meta)
    small = {"image_shape0": [100, 90], "image_shape1": [80, 128]}
    got, a, want, ca = _both(g, small)
    _assert_equal(got, a, want, ca, "smaller images")
    assert a["out_of0"].sum() > full[1]["out_of0"].sum() and a["out_of1"].sum() > full[1]["out_of1"].sum()
    for k in ("cnt0", "cnt1t", "ignore_depth0", "num_visible0"):  # only the outside test reads the image size
        np.testing.assert_array_equal(a[k], full[1][k])
    bare = _both(g, meta, image=False)  # no view["image"]: the depth map's size, here the same 128 x 128
    _assert_equal(*bare, "no image")
    for x, y in zip(bare[0], full[0]):
        np.testing.assert_array_equal(x, y)


def test_layouts_dtypes_holders_and_repeatability():
    from lightglue_amd.depth_matcher import Camera, Pose

    g, meta = _scene(10, 2, 21, 18)
    l0, l1, v0, v1 = _dev(g, "lines0", "lines1", "valid_lines0", "valid_lines1")
    data = R.feed_of(g, meta, device=DEV)
    call = lambda a, b, d: _np(_lg().gt_line_matches_from_pose_depth(a, b, v0, v1, d, npts=33))  # noqa: E731
    base = call(l0, l1, data)
    for x, y in zip(base, call(l0, l1, data)):
        np.testing.assert_array_equal(x, y)  # two runs bit-identical
    assert base[0].any()

    def with_(**kw):
        d = {**data, "view0": dict(data["view0"]), "view1": dict(data["view1"])}
        for k, v in kw.items():
            if k.startswith("camera"):
                d["view" + k[-1]]["camera"] = v
            elif k.startswith("depth"):
                d["view" + k[-1]]["depth"] = v
            else:
                d[k] = v
        return d

    T4 = torch.eye(4, device=DEV).repeat(2, 1, 1)
    T4[:, :3, :3] = data["T_0to1"][:, :9].reshape(2, 3, 3)
    T4[:, :3, 3] = data["T_0to1"][:, 9:]
    variants = {
        "[B,n,2,2]": (l0.reshape(2, -1, 2, 2), l1.reshape(2, -1, 2, 2), data),
        "[B,n,k,2] first and last": (torch.stack([l0[..., :2], l0[..., :2] * 0 - 7, l0[..., 2:]], 2),
                                     torch.stack([l1[..., :2], l1[..., 2:] + 9, l1[..., :2] - 3, l1[..., 2:]], 2), data),
        "non-contiguous fp64": (torch.cat([l0, l0], -1).double()[..., :4], l1.double().transpose(0, 1).contiguous().transpose(0, 1),
                                with_(depth0=data["view0"]["depth"].double(), camera1=data["view1"]["camera"].double())),
        "holders": (l0, l1, with_(camera0=Camera(data["view0"]["camera"]), camera1=Camera(data["view1"]["camera"]),
                                  T_0to1=Pose(data["T_0to1"]), T_1to0=Pose(data["T_1to0"]))),
        "a pose as [B,4,4], a camera as one row, depth as [B,1,H,W]": (
            l0, l1, with_(T_0to1=T4, camera0=data["view0"]["camera"][0], depth1=data["view1"]["depth"][:, None])),
    }
    assert not variants["non-contiguous fp64"][1].is_contiguous()
    for label, (a, b, d) in variants.items():
        for x, y in zip(base, call(a, b, d)):
            np.testing.assert_array_equal(x, y, err_msg=label)


# ------------------------------------------------------------------ the matcher and the pipeline
def test_the_matcher_returns_points_and_lines():
    from lightglue_amd.pipeline import get_model

    name = RANDOM[0]
    g, meta = R.load_fixture(name)
    data = R.feed_of(g, meta, device=DEV)
    l0, l1, v0, v1 = _dev(g, "lines0", "lines1", "valid_lines0", "valid_lines1")
    data.update({"lines0": l0, "lines1": l1, "valid_lines0": v0, "valid_lines1": v1,
                 "keypoints0": l0[..., :2].contiguous(), "keypoints1": l1[..., :2].contiguous()})
    conf = {"n_line_sampled_pts": meta["npts"], "line_perp_dist_th": meta["dist_th"], "overlap_th": meta["overlap_th"],
            "min_visibility_th": meta["min_visibility_th"]}
    out = get_model("matchers.line_depth_matcher")(conf)(data)
    _, want = _end_to_end(name)
    for k, w in zip(("line_assignment", "line_matches0", "line_matches1"), want):
        np.testing.assert_array_equal(out[k].cpu().numpy(), w, err_msg=k)
    points = get_model("matchers.depth_matcher")({})(data)
    assert set(out) == set(points) | {"line_assignment", "line_matches0", "line_matches1"}
    for k, v in points.items():
        assert torch.equal(out[k], v) or (v.dtype.is_floating_point and torch.equal(out[k].isnan(), v.isnan())
                                          and torch.equal(out[k].nan_to_num(), v.nan_to_num())), k
    lines_only = get_model("line_depth_matcher")({**conf, "use_points": False})(data)
    assert set(lines_only) == {"line_assignment", "line_matches0", "line_matches1"}


def test_pipeline_loss_from_line_ground_truth():
    from gluestick_golden_util import model_data
    from lightglue_amd.gs_weights import gluestick_state_dict, wireframe_pair
    from lightglue_amd.pipeline import TwoViewPipeline

    B, W, H = 2, 640, 480
    conf = {"GNN_layers": ["self", "cross"] * 2}
    recipe = {"B": B, "image_wh": [W, H], "image_size": True}
    pair = wireframe_pair(B, (40, 44), (88, 84), (40, 44), seed=61, noise=0.05, width=W, height=H)
    pipe = TwoViewPipeline({"matcher": {"name": "matchers.gluestick", **conf},
                            "ground_truth": {"name": "matchers.line_depth_matcher"}}).eval().cuda()
    sd = gluestick_state_dict(conf, seed=12, proj_gain=15.0, line_gain=0.5)
    pipe.matcher.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    data = {k: v for k, v in model_data(recipe, pair, "cuda").items() if not k.startswith("gt_")}
    assert data["keypoints0"].shape[1] == 128 and data["lines0"].shape[1:] == (40, 2, 2)
    # view 1 of the pair is view 0 plus noise: carry it into the second camera of a plane_scene with the
    # scene's own fp64 projection (points over a hole of the depth map stay where they are)
    scene = GD.plane_scene(71, B, 8, 8, n_dist=2, width=W, height=H, holes=4)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).double()  # noqa: E731

    def carry(xy):
        flat = xy.detach().cpu().double().reshape(B, -1, 2)
        clamped = torch.minimum(flat.clamp(min=0), flat.new_tensor([W - 1.0, H - 1.0]))
        d, v = GD.sample_depth(clamped, t64(scene["depth0"]))
        p, vis = GD.project(clamped, d, None, t64(scene["camera0"]), t64(scene["camera1"]), t64(scene["T_0to1"]), v)
        return torch.where(vis[..., None], p, flat).reshape(xy.shape).to(xy)

    data["keypoints1"], data["lines1"] = carry(data["keypoints1"]), carry(data["lines1"])
    for v in "01":
        data["view" + v]["camera"] = torch.from_numpy(scene["camera" + v]).to(DEV)
        data["view" + v]["depth"] = torch.from_numpy(scene["depth" + v]).to(DEV)
    data["T_0to1"], data["T_1to0"] = torch.from_numpy(scene["T_0to1"]).to(DEV), torch.from_numpy(scene["T_1to0"]).to(DEV)
    data["valid_lines0"] = torch.ones(B, 40, dtype=torch.bool, device=DEV)
    data["valid_lines1"] = torch.ones(B, 44, dtype=torch.bool, device=DEV)
    data["valid_lines1"][:, 5] = False
    with torch.no_grad():
        pred = pipe(data)
        assert not any(k.startswith("gt_") for k in pred)
        losses, metrics = pipe.loss(pred, data)
    torch.cuda.synchronize()
    for k in ("gt_line_assignment", "gt_line_matches0", "gt_line_matches1", "gt_assignment", "gt_matches0", "gt_matches1"):
        assert k in pred and pred[k].device.type == "cuda", k
    assert pred["gt_line_assignment"].any() and pred["gt_line_assignment"].dtype == torch.bool
    assert (pred["gt_line_matches1"][:, 5] == -2).all()
    # at least half of the lines the scene shares are found
    shared = torch.from_numpy(pair["gt_line_assignment"]).to(DEV)
    found = int((pred["gt_line_assignment"] & shared).sum())
    print(f"{found} of {int(shared.sum())} shared lines found")
    assert found >= 0.5 * int(shared.sum())
    assert "line_assignment_nll" in losses and torch.isfinite(losses["line_assignment_nll"]).all()
    assert torch.isfinite(losses["total"]).all()
    direct, _ = pipe.matcher.loss(pred, {**pred, **data})
    assert set(direct) <= set(losses)
    for k, v in direct.items():
        assert torch.equal(torch.as_tensor(losses[k]), torch.as_tensor(v)), k
