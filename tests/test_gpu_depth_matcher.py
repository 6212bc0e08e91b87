"""The pose-and-depth ground truth on the device (lightglue_amd.depth_matcher, csrc/gt_depth.hip)
against the fixtures the reference produced (tests/golden/make_gt_depth_golden.py), hand-built edge
cases against the CPU restatement (tests/gt_depth_ref.py), and the pipeline's training step end to
end from the HIP ground truth to the last gradient -- needs an MI355X.

Bars: the exact fixture bit for bit in all twelve outputs and all three variants; the random fixtures
equal on every item the fixture's fp64 margins decide, depths and projections within the recorded
tolerances; the hand-built cases (exact arithmetic by construction) bit for bit; the pipeline's
losses and parameter gradients bit-identical to the matcher's own ``loss`` on the same ``gt_*``
tensors."""
import functools

import numpy as np
import pytest
import torch

import gt_depth_ref as R
import lgamd  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = R.KEYS
CASES = [(n, i) for n in R.fixture_names() for i in range(len(R.load_fixture(n)[1]["variants"]))]


def _matcher(**conf):
    from lightglue_amd.pipeline import get_model

    return get_model("matchers.depth_matcher")(conf)


def _feed(g, meta=None):
    d = R.feed_of(g, device=DEV)
    if meta is not None:
        d.update(R.precomputed_kw(g, meta, device=DEV))
    return d


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return R.load_fixture(name)


@functools.lru_cache(maxsize=None)
def _run(name, i, reward=True):
    """One device run per fixture variant and flavour, shared by the tests below (read-only)."""
    g, meta = _fixture(name)
    out = _matcher(**R.variant_conf(meta["variants"][i]), reward=reward)(_feed(g, meta))
    return _np(out), out


@pytest.mark.parametrize("name,i", CASES)
def test_matcher_matches_reference_fixture(name, i):
    g, meta = _fixture(name)
    got, dev = _run(name, i)
    assert list(got) == KEYS
    assert dev["assignment"].dtype == torch.bool and dev["visible0"].dtype == torch.bool and dev["visible1"].dtype == torch.bool
    assert dev["matches0"].dtype == torch.int64 and dev["matches1"].dtype == torch.int64
    for k in ("reward", "matching_scores0", "depth_keypoints0", "depth_keypoints1", "proj_0to1", "proj_1to0"):
        assert dev[k].dtype == torch.float32, k
    R.check_against_fixture(got, g, meta, meta["variants"][i])


@pytest.mark.parametrize("name,i", CASES)
def test_structure_of_the_outputs(name, i):
    """At most one positive per row and per column; matches0 / matches1 agree wherever both point at
    each other; the scores are (matches > -1); a positive's row and column carry it unless the
    negative threshold overrode them with -1, and both are visible."""
    got, _ = _run(name, i)
    a, m0, m1 = got["assignment"], got["matches0"], got["matches1"]
    assert a.sum(2).max() <= 1 and a.sum(1).max() <= 1
    for b in range(a.shape[0]):
        r = np.nonzero(m0[b] >= 0)[0]
        back = m1[b][m0[b][r]]
        assert np.all((back == r) | (back < 0)), "matches0 -> matches1 is inconsistent"
        assert np.all(a[b][r, m0[b][r]])
        c = np.nonzero(m1[b] >= 0)[0]
        back = m0[b][m1[b][c]]
        assert np.all((back == c) | (back < 0)), "matches1 -> matches0 is inconsistent"
        assert np.all(a[b][m1[b][c], c])
        bi, bj = np.nonzero(a[b])
        assert np.all((m0[b][bi] == bj) | (m0[b][bi] == -1)) and np.all((m1[b][bj] == bi) | (m1[b][bj] == -1))
        assert np.all(got["visible0"][b][bi]) and np.all(got["visible1"][b][bj])
    np.testing.assert_array_equal(got["matching_scores0"], (m0 > -1).astype(np.float32))
    np.testing.assert_array_equal(got["matching_scores1"], (m1 > -1).astype(np.float32))
    assert set(np.unique(got["reward"])) <= {-1.0, 0.0, 1.0}
    assert m0.min() >= -2 and m1.min() >= -2 and m0.max() < a.shape[2] and m1.max() < a.shape[1]


@pytest.mark.parametrize("name,i", [("gtd_exact_b3_m64_n48", 2), ("gtd_rand_nd4_b2_m300_n257", 0), ("gtd_rand_nd2_b2_m300_n257", 2)])
def test_reward_false_omits_the_key_and_changes_nothing_else(name, i):
    full, _ = _run(name, i)
    lean, _ = _run(name, i, reward=False)
    assert list(lean) == [k for k in KEYS if k != "reward"]
    for k in lean:
        np.testing.assert_array_equal(lean[k].view(np.uint8), full[k].view(np.uint8), err_msg=k)


@pytest.mark.parametrize("name,i", [("gtd_exact_b3_m64_n48", 2), ("gtd_rand_b1_m37_n1100", 1), ("gtd_rand_b1_m1100_n37", 1)])
def test_two_runs_are_bit_identical(name, i):
    g, meta = _fixture(name)
    first, _ = _run(name, i)
    again = _np(_matcher(**R.variant_conf(meta["variants"][i]))(_feed(g, meta)))
    for k in KEYS:
        np.testing.assert_array_equal(again[k].view(np.uint8), first[k].view(np.uint8), err_msg=k)


# ---------------------------------------------------------------------------------------------
# hand-built cases: 512 x 512 pinhole cameras with f = c = 256, depth 4, R = I and a baseline that
# shifts by (8, -4) px -- every fp32 operation is exact, so the restatement's fp32 run is the bar, bit for bit
def _flat(kp0, kp1, holes0=(), holes1=(), fill0=4.0, fill1=4.0, S=512):
    kp0, kp1 = np.asarray(kp0, np.float32), np.asarray(kp1, np.float32)
    B = kp0.shape[0]
    cam = np.tile(np.array([S, S, 256.0, 256.0, 256.0, 256.0], np.float32), (B, 1))
    eye = np.eye(3).reshape(9)
    g = {"keypoints0": kp0, "keypoints1": kp1, "camera0": cam, "camera1": cam,
         "T_0to1": np.tile(np.concatenate([eye, [0.125, -0.0625, 0.0]]).astype(np.float32), (B, 1)),
         "T_1to0": np.tile(np.concatenate([eye, [-0.125, 0.0625, 0.0]]).astype(np.float32), (B, 1)),
         "depth0": np.full((B, S, S), fill0, np.float32), "depth1": np.full((B, S, S), fill1, np.float32)}
    for d, holes in ((g["depth0"], holes0), (g["depth1"], holes1)):
        for x0, y0, x1, y1 in holes:
            d[:, y0:y1, x0:x1] = 0.0
    return g


def _equals_restatement(g, **conf):
    cpu = R.feed_of(g)
    want = R.gt_matches_from_pose_depth(cpu["keypoints0"], cpu["keypoints1"], cpu, conf.get("th_positive", 3.0),
                                        conf.get("th_negative", 5.0), conf.get("th_epi"), conf.get("th_consistency"))
    got = _np(_matcher(**conf)(_feed(g)))
    R.compare(got, {k: v.numpy() for k, v in want.items()}, None, None, True)
    return got


@pytest.mark.parametrize("conf", [{}, {"th_consistency": 1.0}, {"th_consistency": 1.0, "th_epi": 1.0}])
def test_one_point_per_image(conf):
    near = _equals_restatement(_flat([[[100.5, 200.5]]], [[[109.5, 196.5]]]), **conf)  # 1 px off the projection
    assert near["assignment"].tolist() == [[[True]]] and near["matches0"].tolist() == [[0]] and near["matches1"].tolist() == [[0]]
    # with th_epi the epipolar term is masked to ignored x ignored (:87), so a matched pair gets its -1
    assert near["reward"].tolist() == [[[0.0 if "th_epi" in conf else 1.0]]] and near["visible0"].all() and near["visible1"].all()
    far = _equals_restatement(_flat([[[100.5, 200.5]]], [[[300.5, 296.5]]]), **conf)
    assert not far["assignment"].any() and far["matches0"].tolist() == [[-1]] and far["matches1"].tolist() == [[-1]]
    assert far["reward"].tolist() == [[[-1.0]]]


@pytest.mark.parametrize("M,N", [(0, 5), (5, 0)])
def test_empty_side_returns_the_documented_dict(M, N):
    g = _flat(np.zeros((2, M, 2)), np.zeros((2, N, 2)))
    out = _matcher()(_feed(g))
    assert list(out) == KEYS
    ref_a, ref_m0, ref_m1 = R.gt_matches_from_pose_depth(torch.zeros(2, M, 2), torch.zeros(2, N, 2), R.feed_of(g))
    assert out["assignment"].dtype == torch.bool and out["assignment"].shape == ref_a.shape and not out["assignment"].any()
    assert torch.equal(out["matches0"].cpu(), ref_m0) and torch.equal(out["matches1"].cpu(), ref_m1)
    assert out["reward"].shape == (2, M, N) and out["proj_0to1"].shape == (2, M, 2) and out["proj_1to0"].shape == (2, N, 2)
    assert out["visible0"].dtype == torch.bool and out["visible0"].shape == (2, M) and out["visible1"].shape == (2, N)
    assert out["depth_keypoints0"].shape == (2, M) and out["depth_keypoints1"].shape == (2, N)
    assert not out["matching_scores0"].any() and not out["matching_scores1"].any() and not out["visible1"].any()


def _grid_points(rng, B, M):
    return rng.integers(60, 420, (B, M, 2)) + 0.5


@pytest.mark.parametrize("conf", [{}, {"th_epi": 1.0}, {"th_consistency": 1.0, "th_epi": 1.0}])
def test_all_depth_invalid_in_one_image(conf):
    """Every column is masked: argmin 0, no positive; labels -2, or -1 by the negative / epipolar rules."""
    rng = np.random.Generator(np.random.PCG64(5))
    kp0 = _grid_points(rng, 2, 70)
    kp1 = kp0[:, :41] + np.array([8.0, -4.0]) + rng.integers(-6, 7, (2, 41, 2))
    got = _equals_restatement(_flat(kp0, kp1, fill1=0.0), **conf)
    assert not got["assignment"].any() and not got["visible1"].any() and (got["matches0"] < 0).all()
    assert np.isnan(got["depth_keypoints1"]).all() and (got["reward"] <= 0).all()
    assert (got["matches0"] == -1).any() and (got["matches0"] == -2).any()
    if "th_epi" in conf and "th_consistency" not in conf:
        assert (got["matches1"] == -1).any()  # only the epipolar step can label a point without depth
    else:
        assert "th_epi" in conf or (got["matches1"] == -2).all()


def test_hole_borders_and_samples_outside_the_map():
    """Keypoints on a hole border (a NaN neighbour with weight 0 -> the nearest sample, valid), inside
    the hole (NaN depth), at the map's edge with the nearest sample outside (0) and inside."""
    kp0 = [[[100.5, 100.5],   # (100, 100) has depth, (101, *) is the hole: NaN sum, nearest (100, 100) -> 4
            [101.5, 100.5],   # inside the hole: NaN
            [99.5, 100.5],    # clear of the hole: plain bilinear
            [100.5, 99.5],    # the hole's corner neighbour below-right
            [-0.25, 200.5],   # ix = -0.75: (0, 200) is a hole -> NaN sum, nearest (-1, 200) outside -> 0
            [0.25, 300.5],    # ix = -0.25: (0, 300) has depth, the outside corner is skipped (zero padding): 0.75 * 4
            [0.25, 200.5],    # ix = -0.25 over the hole at the edge: nearest (0, 200) -> NaN
            [511.75, 40.5],   # ix = 511.25: right edge, the outside corner is skipped
            [200.5, 200.5]]]
    kp1 = [[[108.5, 96.5], [109.5, 96.5], [107.5, 96.5], [208.5, 196.5], [8.25, 296.5], [300.5, 300.5], [7.75, 196.5]]]
    g = _flat(kp0, kp1, holes0=[(101, 90, 140, 130), (0, 195, 3, 206)], holes1=[(109, 90, 150, 97)])
    for conf in ({}, {"th_consistency": 1.0}, {"th_consistency": 1.0, "th_epi": 1.0}):
        got = _equals_restatement(g, **conf)
        d = got["depth_keypoints0"][0]
        assert d[0] == 4.0 and np.isnan(d[1]) and d[2] == 4.0 and d[4] == 0.0 and d[5] == 3.0 and np.isnan(d[6]) and d[7] == 3.0
    # point 0 projects onto the border of image 1's hole: the nearest sample there has depth, it stays visible
    assert got["visible0"][0].tolist()[:5] == [True, False, True, True, False]


def test_strong_distortion_limit_rule():
    """k1 > 0, k2 <= 0: points beyond r^2 = 1 / (3 k1) are invalid (utils.py:104-118).  Powers of two keep
    the fp32 arithmetic exact up to the final comparison, so the restatement's fp32 run is the bar for
    the flags; projections are compared to 1e-3 px."""
    rng = np.random.Generator(np.random.PCG64(9))
    kp0 = rng.integers(20, 490, (1, 200, 2)) + 0.5
    kp1 = rng.integers(20, 490, (1, 90, 2)) + 0.5
    g = _flat(kp0, kp1)
    for k in ("camera0", "camera1"):
        g[k] = np.concatenate([g[k], np.tile(np.array([2.0, -0.5, 0.0078125, -0.00390625], np.float32), (1, 1))], 1)
    cpu = R.feed_of(g)
    want = R.gt_matches_from_pose_depth(cpu["keypoints0"], cpu["keypoints1"], cpu, 3.0, 5.0, None, None)
    got = _np(_matcher()(_feed(g)))
    r2 = (((kp0 + np.array([8.0, -4.0]) - 256.0) / 256.0) ** 2).sum(-1)
    assert (r2 > 1 / 6.0).any() and (r2 < 1 / 6.0).any() and (np.abs(r2 - 1 / 6.0) > 1e-4).all()
    np.testing.assert_array_equal(got["visible0"], want["visible0"].numpy())
    np.testing.assert_array_equal(got["visible1"], want["visible1"].numpy())
    assert got["visible0"].any() and not got["visible0"].all()
    np.testing.assert_allclose(got["proj_0to1"], want["proj_0to1"].numpy(), rtol=0, atol=1e-3)
    np.testing.assert_array_equal(got["matches0"], want["matches0"].numpy())


def test_views_and_other_dtypes_equal_the_contiguous_fp32_run():
    """Non-contiguous keypoints, fp64 holding fp32 values, and odd M * N (a reward / assignment whose
    second pair starts off a 16-byte boundary)."""
    g, meta = _fixture("gtd_rand_nd2_b2_m300_n257")
    conf = R.variant_conf(meta["variants"][2])
    feed = _feed(g)
    sub = {**feed, "keypoints0": feed["keypoints0"][:, :299], "keypoints1": feed["keypoints1"][:, :255]}
    assert not sub["keypoints0"].is_contiguous() and (299 * 255) % 4 != 0
    a = _matcher(**conf)(sub)
    contiguous = {**sub, "keypoints0": sub["keypoints0"].contiguous(), "keypoints1": sub["keypoints1"].contiguous()}
    b = _matcher(**conf)(contiguous)
    wide = {k: (v.double() if torch.is_tensor(v) else {kk: vv.double() for kk, vv in v.items()}) for k, v in sub.items()}
    c = _matcher(**conf)(wide)
    strided = torch.zeros(2, 299, 4, device=DEV)
    strided[..., ::2] = sub["keypoints0"]
    d = _matcher(**conf)({**sub, "keypoints0": strided[..., ::2]})
    for k in KEYS:
        for other in (b, c, d):
            assert a[k].dtype == other[k].dtype and torch.equal(a[k].view(torch.uint8), other[k].view(torch.uint8)), k
    # dropping points keeps a row's other candidates: compare with the restatement on what its own margins decide
    gs = {**g, "keypoints0": g["keypoints0"][:, :299], "keypoints1": g["keypoints1"][:, :255]}
    v = meta["variants"][2]
    tol = R.tolerances(gs, v["th_positive"], v["th_negative"], v["th_epi"], v["th_consistency"])
    mg = R.margins(gs, v["th_positive"], v["th_negative"], v["th_epi"], v["th_consistency"], tol)
    R.compare(_np(a), {k: t.numpy() for k, t in mg["out"].items()}, mg, tol, False)


def test_camera_and_pose_forms_agree():
    from lightglue_amd.depth_matcher import Camera, Pose

    g, meta = _fixture("gtd_rand_nd4_b2_m300_n257")
    conf = R.variant_conf(meta["variants"][2])
    feed = _feed(g)
    base = _matcher(**conf)(feed)

    class Wrapped:  # the reference's TensorWrapper from outside: a _data tensor
        def __init__(self, data):
            self._data = data

    def with_forms(cam, pose):
        return {**feed, "view0": {**feed["view0"], "camera": cam(feed["view0"]["camera"])},
                "view1": {**feed["view1"], "camera": cam(feed["view1"]["camera"])},
                "T_0to1": pose(feed["T_0to1"]), "T_1to0": pose(feed["T_1to0"])}

    def mat4(rows):
        T = torch.eye(4, device=DEV).repeat(rows.shape[0], 1, 1)
        T[:, :3, :3], T[:, :3, 3] = rows[:, :9].reshape(-1, 3, 3), rows[:, 9:]
        return T

    for cam, pose in ((Camera, Pose), (Wrapped, Wrapped), (lambda c: c, mat4), (lambda c: Camera(c.double()), lambda p: Pose(p.double()))):
        out = _matcher(**conf)(with_forms(cam, pose))
        for k in KEYS:
            assert torch.equal(out[k].view(torch.uint8), base[k].view(torch.uint8)), k
    # an unbatched row broadcasts over B
    one = {**feed, "view0": {**feed["view0"], "camera": feed["view0"]["camera"][0]},
           "view1": {**feed["view1"], "camera": feed["view1"]["camera"][0]}, "T_0to1": feed["T_0to1"][0], "T_1to0": feed["T_1to0"][0]}
    tiled = with_forms(lambda c: c[:1].repeat(2, 1), lambda p: p[:1].repeat(2, 1))
    a, b = _matcher(**conf)(one), _matcher(**conf)(tiled)
    for k in KEYS:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    np.testing.assert_array_equal(a["matches0"][0].cpu().numpy(), base["matches0"][0].cpu().numpy())


def test_flat_indices_past_2_to_the_31():
    """3 x 32768 x 32768: the last pair's block of the assignment starts at byte 2^31.  Without the
    reward (it would be 12 GiB); every positive is found where matches0 says, in every pair."""
    B, M = 3, 32768
    rng = np.random.Generator(np.random.PCG64(17))
    kp0 = _grid_points(rng, B, M)
    kp1 = np.stack([kp0[b, rng.permutation(M)] for b in range(B)]) + np.array([8.0, -4.0])
    out = _matcher(reward=False)(_feed(_flat(kp0, kp1)))
    a, m0, m1 = out["assignment"], out["matches0"], out["matches1"]
    assert a.shape == (B, M, M) and a.numel() > 2**31
    pos = m0 > -1
    n_pos = int(pos.sum())
    assert n_pos > M and int(a.sum()) == n_pos == int((m1 > -1).sum())  # duplicates tie; the unique points match
    b, i = torch.nonzero(pos, as_tuple=True)
    assert bool(a[b, i, m0[b, i]].all()) and bool((m1[b, m0[b, i]] == i).all())
    assert bool(pos[B - 1].any()) and bool(out["visible0"].all()) and bool(out["visible1"].all())
    # the same labels as each pair alone
    alone = _matcher(reward=False)(_feed(_flat(kp0[B - 1:], kp1[B - 1:])))
    assert torch.equal(alone["matches0"][0], m0[B - 1]) and torch.equal(alone["matches1"][0], m1[B - 1])
    assert torch.equal(alone["assignment"][0], a[B - 1])


# ---------------------------------------------------------------------------------------------
# end to end: the pipeline's training step
def _e2e_data(B=2, M=128, seed=23):
    from lightglue_amd.sg_weights import synthetic_scores
    from lightglue_amd.weights import synthetic_pair

    W, H = 320, 240
    g = R.plane_scene(seed, B, M, M, width=W, height=H)
    p = synthetic_pair(B=B, M=M, N=M, seed=seed, width=W, height=H)
    data = {"keypoints0": g["keypoints0"], "keypoints1": g["keypoints1"], "descriptors0": p["descriptors0"],
            "descriptors1": p["descriptors1"], "keypoint_scores0": synthetic_scores(B, M, seed=seed + 1),
            "keypoint_scores1": synthetic_scores(B, M, seed=seed + 2)}
    feed = {k: torch.from_numpy(v).to(DEV) for k, v in data.items()}
    size = torch.tensor([[float(W), float(H)]] * B, device=DEV)
    scene = _feed(g)
    for i in "01":
        feed["view" + i] = {"image_size": size, "image": torch.zeros(B, 1, H, W, device=DEV), **scene["view" + i]}
    feed["T_0to1"], feed["T_1to0"] = scene["T_0to1"], scene["T_1to0"]
    return g, feed


def _matcher_conf(kind):
    if kind == "lightglue":
        return {"name": "matchers.lightglue", "n_layers": 3}
    return {"name": "gluefactory_nonfree.superglue", "GNN_layers": ["self", "cross"]}


@pytest.mark.parametrize("kind", ["lightglue", "superglue"])
def test_pipeline_loss_and_backward_equal_the_direct_call(kind):
    from lightglue_amd.pipeline import TwoViewPipeline
    from lightglue_amd.weights import synthetic_state_dict

    torch.manual_seed(0)
    th = {"th_positive": 3.0, "th_negative": 5.0, "th_consistency": 4.0, "th_epi": 1.0}
    pipe = TwoViewPipeline({"matcher": _matcher_conf(kind), "ground_truth": {"name": "matchers.depth_matcher", **th}}).to(DEV)
    if kind == "lightglue":
        sd = synthetic_state_dict({"n_layers": 3}, seed=4)
        pipe.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    pipe.train()
    g, feed = _e2e_data()

    def grads():
        out = {n: p.grad.clone() for n, p in pipe.named_parameters() if p.grad is not None}
        pipe.zero_grad(set_to_none=True)
        return out

    pred = pipe(feed)
    assert not any(k.startswith("gt_") for k in pred)
    losses, _ = pipe.loss(pred, feed)
    torch.mean(losses["total"]).backward()  # train.py:436,450
    g_pipe = grads()
    assert g_pipe and all(torch.isfinite(x).all() for x in g_pipe.values())
    assert any(bool(x.abs().max() > 0) for x in g_pipe.values())
    gt = {k: v for k, v in pred.items() if k.startswith("gt_")}
    assert sorted(gt) == sorted("gt_" + k for k in KEYS)
    assert gt["gt_assignment"].dtype == torch.bool and bool(gt["gt_assignment"].any())

    # the matcher alone, handed the same gt_* tensors
    pred2 = pipe.matcher(feed)
    out2 = pipe.matcher.loss(pred2, {**pred2, **feed, **gt})
    losses2 = out2 if isinstance(out2, dict) else out2[0]
    torch.mean(losses2["total"]).backward()
    g_direct = grads()
    assert set(losses2) <= set(losses)
    for k, v in losses2.items():
        if torch.is_tensor(v):
            assert torch.equal(losses[k], v), k
        else:
            assert losses[k] == v, k
    assert g_pipe.keys() == g_direct.keys()
    for n in g_pipe:
        assert torch.equal(g_pipe[n], g_direct[n]), n

    # the ground truth itself, against the CPU restatement on the decidable items
    args = (th["th_positive"], th["th_negative"], th["th_epi"], th["th_consistency"])
    tol = R.tolerances(g, *args)
    mg = R.margins(g, *args, tol)
    for k in ("und_rows", "und_cols", "und_p0", "und_p1", "und_reward"):
        assert (~mg[k]).mean() >= 0.9, k
    R.compare({k[3:]: v.cpu().numpy() for k, v in gt.items()}, {k: t.numpy() for k, t in mg["out"].items()}, mg, tol, False)
