"""Batched LO-RANSAC on the device (lightglue_amd.robust, csrc/ransac_homography.hip) -- needs an MI355X.
Every case of tests/golden/ransac/ransac.npz through the C ABI and through HomographyEstimator: the
info row and the inlier mask equal the float64 restatement's (tests/ransac_ref.py; the fixture's
margins are what makes that a fair demand), H_error_ransac within the project's DLT bar
(``dlt_rel_bar`` of tests/golden/match_eval/match_eval.npz).  Then what no fixture can hold: the
mask against the returned matrix, ragged and permuted batches against their pairs alone, per-pair
thresholds, run-to-run bits, the global-memory route, untouched outputs, and a matcher's ``pred``
straight from TwoViewPipeline."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import ransac_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ransac", "ransac.npz")
MIN_MARGIN = 1e-7


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def bar():
    v = float(np.load(os.path.join(HERE, "golden", "match_eval", "match_eval.npz"))["dlt_rel_bar"])
    assert abs(v - 2.059e-5) < 1e-8
    return v


def options(g, name):
    return {"max_iters": int(g[f"{name}/max_iters"]), "confidence": float(g[f"{name}/confidence"]),
            "seed": int(g[f"{name}/seed"]), "min_area": float(g[f"{name}/min_area"])}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def abi_call(kp0, kp1, m0, th, num0=None, num1=None, H_gt=None, size0=None, fill=-123.5, **opt):
    """lg_ransac_homography through ctypes on prefilled outputs; everything back on the host."""
    from lightglue_amd import _lib

    lib = _lib.load()
    B, M = kp0.shape[:2]
    N = kp1.shape[1]
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    H = torch.full((B, 9), fill, device="cuda")
    inl = torch.full((B, M), 77, dtype=torch.uint8, device="cuda")
    info = torch.full((B, 8), -77, dtype=torch.int32, device="cuda")
    mk = torch.full((B, M, 4), fill, device="cuda")
    err = torch.full((B,), fill, device="cuda") if H_gt is not None else None
    rc = lib.lg_ransac_homography(ptr(kp0), ptr(kp1), ptr(m0), B, M, N, ptr(num0), ptr(num1), ptr(th), opt["max_iters"],
                                  opt["confidence"], opt["seed"], opt["min_area"], ptr(H_gt), ptr(size0), ptr(H), ptr(inl),
                                  ptr(info), ptr(mk), ptr(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.LG_OK, lib.lg_last_error()
    torch.cuda.synchronize()
    out = {"H": H.cpu().numpy().reshape(B, 3, 3), "inliers": inl.cpu().numpy(), "info": info.cpu().numpy(),
           "m_kpts": mk.cpu().numpy()}
    if err is not None:
        out["H_error"] = err.cpu().numpy()
    return out


def case_call(g, name, **over):
    kp0, kp1, m0 = dev(g[f"{name}/kpts0"][None]), dev(g[f"{name}/kpts1"][None]), dev(g[f"{name}/matches0"][None])
    th = dev(np.array([g[f"{name}/th"]], dtype=np.float32))
    return abi_call(kp0, kp1, m0, th, H_gt=dev(g[f"{name}/H_gt"][None]), size0=dev(g[f"{name}/size0"][None]),
                    **{**options(g, name), **over})


def self_consistent(H, mask, kp0, kp1, m0, th, num0=None, num1=None):
    """The mask is the fp64 classification under the returned fp32 matrix, nothing else."""
    pts, slots = ref.live_matches(kp0, kp1, m0, num0, num1)
    want = np.zeros(len(kp0), dtype=bool)
    if len(pts):
        with np.errstate(invalid="ignore"):
            want[slots] = ref.residuals(H.astype(np.float64), pts) < float(np.float32(th))
    np.testing.assert_array_equal(mask.astype(bool), want)


def against_restatement(got, want, b, bar, what):
    """One pair of a device result against the restatement's dict."""
    info = got["info"][b]
    print(f"{what}: info {info[:7].tolist()}, restatement {ref.info_row(want)[:7].tolist()}, margin {want['margin']:.3e}")
    np.testing.assert_array_equal(info, ref.info_row(want), err_msg=what)
    M = len(want["inliers_slots"])
    np.testing.assert_array_equal(got["inliers"][b][:M].astype(bool), want["inliers_slots"], err_msg=what)
    assert set(np.unique(got["inliers"][b])) <= {0, 1}
    if "H_error" in got and "H_error" in want:
        e, w = float(got["H_error"][b]), want["H_error"]
        print(f"{what}: H_error {e:.9g}, restatement {w:.9g}, bar {bar:.3e}")
        if want["success"]:
            assert abs(e - w) <= bar * w, what
        else:
            assert math.isinf(e) and e > 0, what
    if not want["success"]:
        np.testing.assert_array_equal(got["H"][b], np.eye(3, dtype=np.float32))
        assert not got["inliers"][b].any()


@pytest.mark.parametrize("name", list("123456789"))
def test_every_fixture_case_through_the_c_abi(golden, bar, name):
    g = golden
    got = case_call(g, name)
    want = {**dict(zip(ref.INFO_FIELDS, g[f"{name}/info"].tolist())), "inliers_slots": g[f"{name}/inliers"],
            "H_error": float(g[f"{name}/H_error"]), "margin": float(g[f"{name}/margin"])}
    assert want["margin"] >= MIN_MARGIN
    against_restatement(got, want, 0, bar, f"case {name}")
    self_consistent(got["H"][0], got["inliers"][0], g[f"{name}/kpts0"], g[f"{name}/kpts1"], g[f"{name}/matches0"],
                    g[f"{name}/th"])
    if want["success"]:
        assert got["H"][0][2, 2] == 1.0
        # the same DLT on the same inlier set, rounded to fp32 once on either side
        assert np.abs(got["H"][0] - g[f"{name}/H"]).max() <= bar * np.abs(g[f"{name}/H"]).max()
    # the compaction buffer: the matched points in slot order, nothing past them
    K = int(g[f"{name}/info"][1])
    np.testing.assert_array_equal(got["m_kpts"][0, :K], g[f"{name}/m_kpts"])
    assert (got["m_kpts"][0, K:] == -123.5).all()


@pytest.mark.parametrize("name", list("123456789"))
def test_every_fixture_case_through_the_estimator(golden, name):
    from lightglue_amd import robust

    g = golden
    pts = g[f"{name}/m_kpts"]
    K = len(pts)
    slots = ref.live_matches(g[f"{name}/kpts0"], g[f"{name}/kpts1"], g[f"{name}/matches0"])[1]
    est = robust.load_estimator("homography", "hip")({"ransac_th": float(g[f"{name}/th"]), "options": options(g, name)})
    out = est({"m_kpts0": dev(pts[:, :2]), "m_kpts1": dev(pts[:, 2:])})
    assert set(out) == {"success", "M_0to1", "inliers"} and isinstance(out["success"], bool)
    assert out["M_0to1"].shape == (3, 3) and out["M_0to1"].is_cuda and out["M_0to1"].dtype == torch.float32
    assert out["inliers"].shape == (K,) and out["inliers"].dtype == torch.bool
    assert out["success"] == bool(g[f"{name}/info"][0])
    np.testing.assert_array_equal(out["inliers"].cpu().numpy(), g[f"{name}/inliers"][slots])
    if K:  # the matched-points form is the keypoint form of the same matches: the same bits
        np.testing.assert_array_equal(out["M_0to1"].cpu().numpy(), case_call(g, name)["H"][0])
    # the batched form: device tensors, the same pair twice, the second cut short by num_matches
    if K >= 2:
        p0, p1 = dev(np.stack([pts[:, :2]] * 2)), dev(np.stack([pts[:, 2:]] * 2))
        two = est({"m_kpts0": p0, "m_kpts1": p1, "num_matches": torch.tensor([K, K - 1])})
        assert two["success"].shape == (2,) and two["success"].dtype == torch.bool and two["success"].is_cuda
        assert two["M_0to1"].shape == (2, 3, 3) and two["inliers"].shape == (2, K)
        assert torch.equal(two["M_0to1"][0], out["M_0to1"]) and torch.equal(two["inliers"][0], out["inliers"])
        assert int(two["info"][1, 1]) == K - 1 and not bool(two["inliers"][1, K - 1])


def ragged_batch(g, names, max_iters):
    """The pairs padded to one shape; the padding holds NaN keypoints and wild match indices."""
    M = max(len(g[f"{n}/kpts0"]) for n in names) + 3
    N = max(len(g[f"{n}/kpts1"]) for n in names) + 5
    B = len(names)
    kp0, kp1 = np.full((B, M, 2), np.nan, dtype=np.float32), np.full((B, N, 2), np.nan, dtype=np.float32)
    wild = np.resize(np.array([10**12, -5, 2**31, 1, 0, N - 1], dtype=np.int64), M)
    m0 = np.tile(wild, (B, 1))
    num0, num1 = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, n in enumerate(names):
        a, c = g[f"{n}/kpts0"], g[f"{n}/kpts1"]
        num0[b], num1[b] = len(a), len(c)
        kp0[b, :len(a)], kp1[b, :len(c)], m0[b, :len(a)] = a, c, g[f"{n}/matches0"]
    th = np.array([g[f"{n}/th"] for n in names], dtype=np.float32)
    Hg, sz = np.stack([g[f"{n}/H_gt"] for n in names]), np.stack([g[f"{n}/size0"] for n in names])
    opt = {**options(g, names[0]), "max_iters": max_iters}
    return abi_call(dev(kp0), dev(kp1), dev(m0), dev(th), dev(num0), dev(num1), dev(Hg), dev(sz), **opt), num0


def test_ragged_and_permuted_batches_equal_their_pairs_alone(golden):
    g = golden
    names = list("123456789")
    alone = {n: case_call(g, n, max_iters=300) for n in names}
    for order in (names, ["9", "2", "7", "1", "6", "3", "8", "5", "4"]):
        got, num0 = ragged_batch(g, order, 300)
        for b, n in enumerate(order):
            a = alone[n]
            K = int(a["info"][0, 1])
            np.testing.assert_array_equal(got["info"][b], a["info"][0], err_msg=n)
            assert got["H"][b].tobytes() == a["H"][0].tobytes(), n
            assert got["H_error"][b].tobytes() == a["H_error"][0].tobytes(), n
            np.testing.assert_array_equal(got["inliers"][b, :num0[b]], a["inliers"][0], err_msg=n)
            assert not got["inliers"][b, num0[b]:].any()
            assert got["m_kpts"][b, :K].tobytes() == a["m_kpts"][0, :K].tobytes(), n
            assert (got["m_kpts"][b, K:] == -123.5).all()


def test_per_pair_thresholds_equal_single_calls(golden):
    g = golden
    ths = [0.5, 1.0, 3.0]
    rep = lambda k: dev(np.stack([g[f"2/{k}"]] * 3))  # noqa: E731
    got = abi_call(rep("kpts0"), rep("kpts1"), rep("matches0"), dev(np.array(ths, dtype=np.float32)), H_gt=rep("H_gt"),
                   size0=rep("size0"), **options(g, "2"))
    for b, th in enumerate(ths):
        one = abi_call(dev(g["2/kpts0"][None]), dev(g["2/kpts1"][None]), dev(g["2/matches0"][None]),
                       dev(np.array([th], dtype=np.float32)), H_gt=dev(g["2/H_gt"][None]), size0=dev(g["2/size0"][None]),
                       **options(g, "2"))
        for k in one:
            assert got[k][b].tobytes() == one[k][0].tobytes(), (th, k)
        self_consistent(got["H"][b], got["inliers"][b], g["2/kpts0"], g["2/kpts1"], g["2/matches0"], th)
    assert got["info"][0, 2] < got["info"][1, 2] < got["info"][2, 2]  # a wider threshold, more inliers
    # a [B] tensor as the estimator's ransac_th: the same three results on the matched points
    from lightglue_amd import robust

    pts = np.stack([g["2/m_kpts"]] * 3)
    est = robust.HomographyEstimator({"ransac_th": torch.tensor(ths), "options": options(g, "2")})
    out = est({"m_kpts0": dev(pts[..., :2]), "m_kpts1": dev(pts[..., 2:])})
    np.testing.assert_array_equal(out["M_0to1"].cpu().numpy(), got["H"])
    np.testing.assert_array_equal(out["info"].cpu().numpy(), got["info"])


def test_run_to_run_bits_and_another_seed(golden):
    g = golden
    a, b = case_call(g, "2"), case_call(g, "2")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = case_call(g, "2", seed=12345)
    assert c["info"][0, 3] != a["info"][0, 3] and c["info"][0, 0] == 1
    self_consistent(c["H"][0], c["inliers"][0], g["2/kpts0"], g["2/kpts1"], g["2/matches0"], g["2/th"])
    assert c["info"][0, 2] == c["inliers"][0].sum()


def test_kernel_sampler_is_keyed_by_seed_hypothesis_and_draw():
    """The kernel's own sampler, hypothesis by hypothesis.  Twelve exact matches of a translation on
    integer pixels: four in general position (slots 0-3) and eight on one line (slots 4-11).  A sample is
    valid if and only if it holds at most two of the line's points (every other triple has an integer
    determinant of at least 1, a collinear one exactly 0), and every valid hypothesis explains all twelve.
    So ``valid_hypotheses`` under a cap of n counts the valid samples among t < n and ``best_t`` is the first
    of them: both follow from the specification's index sequence alone."""
    G = np.array([[50, 60], [600, 40], [580, 430], [70, 400]], dtype=np.int64)
    x = np.array([10, 23, 37, 52, 68, 85, 103, 122], dtype=np.int64)
    P = np.concatenate([G, np.stack([x, 2 * x + 5], 1)])
    det = lambda a, b, c: int((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))  # noqa: E731
    for i in range(12):
        for j in range(i + 1, 12):
            for k in range(j + 1, 12):
                assert (det(P[i], P[j], P[k]) == 0) == (i >= 4)  # collinear exactly when all three are on the line
    k0 = P.astype(np.float32)
    k1 = k0 + np.array([7, -3], dtype=np.float32)
    th = dev(np.array([1.0], dtype=np.float32))
    seen = set()
    for seed in (0, 1, 2, 12345, 2**63 + 5):
        valid = [sum(i >= 4 for i in ref.sample(seed, t, 12)) <= 2 for t in range(256)]
        seen.add(tuple(valid))
        for cap in (1, 37, 256):
            got = abi_call(dev(k0[None]), dev(k1[None]), None, th, max_iters=cap, confidence=0.995, seed=seed, min_area=1.0)
            n = sum(valid[:cap])
            first = valid.index(True) if n else -1
            want = [int(n > 0), 12, 12 if n else 0, first, 12 if n else 0, 1, n, 0]
            assert got["info"][0].tolist() == want, (seed, cap)
    assert len(seen) == 5  # another seed, another sequence
    # the batch position is not part of the key: the pair at three places of a batch
    rep = dev(np.stack([k0] * 3)), dev(np.stack([k1] * 3))
    got = abi_call(rep[0], rep[1], None, dev(np.ones(3, dtype=np.float32)), max_iters=256, confidence=0.995, seed=2, min_area=1.0)
    assert (got["info"] == got["info"][0]).all() and got["H"][1].tobytes() == got["H"][0].tobytes() == got["H"][2].tobytes()


def test_more_matches_than_lds_holds_run_from_global_memory(bar):
    """K just above the LDS capacity and K equal to it, max_iters 256, against the restatement;
    generator seeds in a fixed order, the first whose two margins pass the fixture's rule."""
    from lightglue_amd import robust

    K = robust.LDS_MATCHES + 1
    H_gt = np.array([[0.98, -0.04, 12.0], [0.03, 1.01, -7.0], [-3e-5, 2e-5, 1.0]])
    size = np.array([640.0, 480.0], dtype=np.float32)
    opt = {"max_iters": 256, "confidence": 0.995, "seed": 3, "min_area": 1.0}
    for gen_seed in range(20):
        rng = np.random.default_rng(1000 + gen_seed)
        k0 = rng.uniform([20, 20], [620, 460], (K, 2))
        q = np.concatenate([k0, np.ones((K, 1))], 1) @ H_gt.T
        k1 = q[:, :2] / q[:, 2:] + rng.normal(0, 0.7, (K, 2))
        out = rng.permutation(K)[: K // 2]
        k1[out] = rng.uniform([0, 0], [640, 480], (len(out), 2))
        k0, k1 = k0.astype(np.float32), k1.astype(np.float32)
        want = ref.estimate_pair(k0, k1, None, 3.0, H_gt=H_gt.astype(np.float32), size=size, **opt)
        # one match fewer fits LDS exactly: the same leading K - 1 matches, under the same rule
        want2 = ref.estimate_pair(k0[:-1], k1[:-1], None, 3.0, H_gt=H_gt.astype(np.float32), size=size, **opt)
        if min(want["margin"], want2["margin"]) >= MIN_MARGIN:
            break
    else:
        pytest.fail("no generator seed passes the margin rule")
    assert want["num_matches"] == K > robust.LDS_MATCHES and want["success"] and want["rounds"] == 1
    th = dev(np.array([3.0], dtype=np.float32))
    got = abi_call(dev(k0[None]), dev(k1[None]), None, th, H_gt=dev(H_gt.astype(np.float32)[None]), size0=dev(size[None]),
                   **opt)
    against_restatement(got, want, 0, bar, f"K = {K} (generator seed {1000 + gen_seed})")
    self_consistent(got["H"][0], got["inliers"][0], k0, k1, None, 3.0)
    np.testing.assert_array_equal(got["m_kpts"][0], np.concatenate([k0, k1], 1))
    assert want2["num_matches"] == robust.LDS_MATCHES and want2["success"]
    n = torch.tensor([K - 1], dtype=torch.int32).cuda()
    got2 = abi_call(dev(k0[None]), dev(k1[None]), None, th, n, n, dev(H_gt.astype(np.float32)[None]), dev(size[None]), **opt)
    against_restatement(got2, want2, 0, bar, f"K = {K - 1}")
    self_consistent(got2["H"][0], got2["inliers"][0], k0, k1, None, 3.0, K - 1, K - 1)


def test_matcher_output_goes_straight_into_the_robust_evaluation(bar):
    """TwoViewPipeline with the nearest-neighbour matcher on synthetic descriptors (B = 2, 96 and 80
    keypoints): its ``pred`` is evaluated as it is, and each pair equals the restatement."""
    from lightglue_amd import robust
    from lightglue_amd.pipeline import TwoViewPipeline

    rng = np.random.default_rng(11)
    B, M, N, D = 2, 96, 80, 64
    H = np.array([[[1.02, 0.03, 8.0], [-0.02, 0.97, -5.0], [2e-5, -3e-5, 1.0]],
                  [[0.95, -0.05, 20.0], [0.04, 1.03, 3.0], [-4e-5, 1e-5, 1.0]]])
    k0 = rng.uniform([20, 20], [620, 460], (B, M, 2))
    d0 = rng.normal(size=(B, M, D))
    k1, d1 = rng.uniform([0, 0], [640, 480], (B, N, 2)), rng.normal(size=(B, N, D))
    for b in range(B):  # 60 true correspondences at shuffled slots; a quarter of them land in the wrong place
        src, dst = rng.permutation(M)[:60], rng.permutation(N)[:60]
        q = np.concatenate([k0[b, src], np.ones((60, 1))], 1) @ H[b].T
        k1[b, dst] = q[:, :2] / q[:, 2:] + rng.normal(0, 0.7, (60, 2))
        k1[b, dst[:15]] = rng.uniform([0, 0], [640, 480], (15, 2))
        d1[b, dst] = d0[b, src] + 0.1 * rng.normal(size=(60, D))
    unit = lambda d: (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)  # noqa: E731
    size = torch.tensor([[640.0, 480.0]]).repeat(B, 1).cuda()
    data = {"view0": {"image_size": size, "cache": {"keypoints": dev(k0.astype(np.float32)), "descriptors": dev(unit(d0))}},
            "view1": {"image_size": size, "cache": {"keypoints": dev(k1.astype(np.float32)), "descriptors": dev(unit(d1))}},
            "H_0to1": dev(H.astype(np.float32))}
    pipe = TwoViewPipeline({"extractor": {"name": None}, "allow_no_extract": True,
                            "matcher": {"name": "matchers.nearest_neighbor_matcher", "ratio_thresh": 0.9}})
    with torch.no_grad():
        pred = pipe(data)
    conf = {"estimator": "hip", "ransac_th": 2.0, "options": {"max_iters": 512, "seed": 1}}
    out = robust.eval_homography_robust(data, pred, conf)
    assert set(out) == {"H_error_ransac", "ransac_inl", "ransac_inl%", "M_0to1", "inliers"}
    assert all(v.is_cuda for v in out.values())
    assert out["H_error_ransac"].shape == (B,) and out["M_0to1"].shape == (B, 3, 3) and out["inliers"].shape == (B, M)
    cb = robust.as_export_callback(conf)(pred, data)
    assert all(torch.equal(cb[k], out[k]) for k in out)
    for b in range(B):
        want = ref.estimate_pair(pred["keypoints0"][b].cpu().numpy(), pred["keypoints1"][b].cpu().numpy(),
                                 pred["matches0"][b].cpu().numpy(), 2.0, H_gt=H[b].astype(np.float32), size=[640.0, 480.0],
                                 max_iters=512, confidence=0.995, seed=1, min_area=1.0)
        print(f"pair {b}: restatement info {ref.info_row(want)[:7].tolist()}, H_error {want['H_error']:.6g}, "
              f"margin {want['margin']:.3e}; device H_error {float(out['H_error_ransac'][b]):.6g}")
        assert want["margin"] >= MIN_MARGIN and want["success"] and want["num_matches"] >= 30
        np.testing.assert_array_equal(out["inliers"][b].cpu().numpy(), want["inliers_slots"])
        assert float(out["ransac_inl"][b]) == want["num_inliers"]
        assert float(out["ransac_inl%"][b]) == float(np.float32(want["num_inliers"]) / np.float32(want["num_matches"]))
        assert abs(float(out["H_error_ransac"][b]) - want["H_error"]) <= bar * want["H_error"]
    # one pair without the batch dimension: Python numbers, element 0 of the batched form
    d0_, p0_ = ({"H_0to1": data["H_0to1"][0], "view0": {"image_size": size[0]}},
                {k: pred[k][0] for k in ("keypoints0", "keypoints1", "matches0", "matching_scores0")})
    one = robust.eval_homography_robust(d0_, p0_, conf)
    for k in ("H_error_ransac", "ransac_inl", "ransac_inl%"):
        assert isinstance(one[k], float) and one[k] == float(out[k][0]), k
    assert torch.equal(one["M_0to1"], out["M_0to1"][0]) and torch.equal(one["inliers"], out["inliers"][0])
