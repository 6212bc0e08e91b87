"""Batched five-point LO-RANSAC on the device (lightglue_amd.relative_pose, csrc/ransac_relpose.hip) --
needs an MI355X.  The solver alone through lg_essential_5pt against the restatement's companion route;
every case of tests/golden/relpose/relpose.npz through the C ABI: info fields 0-6 and the inlier mask
equal the float64 restatement's (tests/relpose_ref.py; the fixture's margins and its two agreeing root
routes are what makes that a fair demand), R and t within ``pose_abs_bar``, the errors within fp32
rounding of their float64 recomputation.  Then what no fixture can hold: the mask against the returned
pose, ragged and permuted batches against their pairs alone, per-pair thresholds, run-to-run bits, the
two sides of the LDS threshold, the estimator class and a matcher's ``pred`` straight from
TwoViewPipeline."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import relpose_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "relpose", "relpose.npz")
CASES = ["one_round", "several_rounds", "partial_round", "five_exact", "four", "none", "plane", "forward", "intrinsics",
         "keypoints"]
OUT_ROUNDING = 2.0**-22  # fp32 rounding of an output, relative


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    assert float(g["pose_abs_bar"]) == max(10 * float(g["pose_route_diff"]), 2.0**-22)
    return g


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cam6(c):
    """fx, fy, cx, cy -> the reference's Camera row (w, h, fx, fy, cx, cy)."""
    c = np.asarray(c, dtype=np.float32)
    return np.concatenate([2 * c[..., 2:], c], -1)


def abi_call(kp0, kp1, m0, cam0, cam1, th, num0=None, num1=None, T_gt=None, fill=-123.5, **opt):
    """lg_ransac_relpose through ctypes on prefilled outputs; everything back on the host."""
    from lightglue_amd import _lib

    lib = _lib.load()
    B, M = kp0.shape[:2]
    N = kp1.shape[1]
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    R = torch.full((B, 9), fill, device="cuda")
    t = torch.full((B, 3), fill, device="cuda")
    inl = torch.full((B, M), 77, dtype=torch.uint8, device="cuda")
    info = torch.full((B, 8), -77, dtype=torch.int32, device="cuda")
    mk = torch.full((B, M, 4), fill, device="cuda")
    err = torch.full((B, 3), fill, device="cuda") if T_gt is not None else None
    rc = lib.lg_ransac_relpose(ptr(kp0), ptr(kp1), ptr(m0), B, M, N, ptr(num0), ptr(num1), ptr(cam0), ptr(cam1), ptr(th),
                               opt["max_iters"], opt["confidence"], opt["seed"], ptr(T_gt), ptr(R), ptr(t), ptr(inl),
                               ptr(info), ptr(mk), ptr(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.LG_OK, lib.lg_last_error()
    torch.cuda.synchronize()
    out = {"R": R.cpu().numpy().reshape(B, 3, 3), "t": t.cpu().numpy(), "inliers": inl.cpu().numpy(),
           "info": info.cpu().numpy(), "m_kpts": mk.cpu().numpy()}
    if err is not None:
        out["errors"] = err.cpu().numpy()
    return out


def options(g, name):
    return {"max_iters": int(g[f"{name}/max_iters"]), "confidence": float(g[f"{name}/confidence"]),
            "seed": int(g[f"{name}/seed"])}


def case_call(g, name, **over):
    one = lambda k: dev(g[f"{name}/{k}"][None])  # noqa: E731
    return abi_call(one("kpts0"), one("kpts1"), one("matches0"), one("camera0"), one("camera1"),
                    dev(np.array([g[f"{name}/th"]], dtype=np.float32)), T_gt=one("T_gt"), **{**options(g, name), **over})


def restate(g, name, **over):
    return ref.estimate_pair(g[f"{name}/kpts0"], g[f"{name}/kpts1"], g[f"{name}/matches0"], g[f"{name}/camera0"],
                             g[f"{name}/camera1"], float(g[f"{name}/th"]), T_gt=g[f"{name}/T_gt"],
                             **{**options(g, name), **over})


def self_consistent(R, t, mask, kp0, kp1, m0, cam0, cam1, th, num0=None, num1=None):
    """The mask is the fp64 classification under the returned fp32 pose, nothing else; the pose is a pose."""
    pts, slots = ref.live_matches(kp0, kp1, m0, num0, num1)
    want = np.zeros(len(kp0), dtype=bool)
    R, t = R.astype(np.float64), t.astype(np.float64)
    if len(pts):
        n, thn = ref.normalise(pts, cam0, cam1), ref.threshold_n(th, cam0, cam1)
        with np.errstate(invalid="ignore"):
            want[slots] = (ref.sampson2(ref.essential_from(R, t), n) < thn * thn) & ref._front(R, t, n)
    np.testing.assert_array_equal(mask.astype(bool), want)
    if mask.any():
        assert np.linalg.norm(R.T @ R - np.eye(3)) <= 1e-6 and np.linalg.det(R) > 0
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-6


def against_restatement(got, want, b, g, what, T_gt=None):
    """One pair of a device result against the restatement's dict."""
    info, bar = got["info"][b], float(g["pose_abs_bar"])
    print(f"{what}: info {info.tolist()}, restatement {ref.info_row(want).tolist()}, margin {want['margin']:.3e}")
    np.testing.assert_array_equal(info[:7], ref.info_row(want)[:7], err_msg=what)
    M = len(want["inliers_slots"])
    np.testing.assert_array_equal(got["inliers"][b][:M].astype(bool), want["inliers_slots"], err_msg=what)
    assert set(np.unique(got["inliers"][b])) <= {0, 1}
    if want["success"]:
        dR, dt = np.abs(got["R"][b] - want["R"]).max(), np.abs(got["t"][b] - want["t"]).max()
        print(f"{what}: |R - R'| {dR:.3e}, |t - t'| {dt:.3e}, bar {bar:.3e}")
        assert dR <= bar and dt <= bar, what
        if "errors" in got:
            again = ref.pose_errors(got["R"][b], got["t"][b], T_gt)
            print(f"{what}: errors {got['errors'][b].tolist()}, recomputed {again}")
            for e, w in zip(got["errors"][b], again):
                assert w >= 0.01 and abs(float(e) - w) <= OUT_ROUNDING * w, what
    else:
        np.testing.assert_array_equal(got["R"][b], np.eye(3, dtype=np.float32))
        assert not got["t"][b].any() and not got["inliers"][b].any() and info[2] == 0
        if "errors" in got:
            assert np.isposinf(got["errors"][b]).all()


# ---- the solver alone ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved(golden):
    from lightglue_amd import _lib

    lib = _lib.load()
    P = dev(golden["solver/pts"])
    E = torch.full((64, 10, 9), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    rc = lib.lg_essential_5pt(ctypes.c_void_p(P.data_ptr()), 64, ctypes.c_void_p(E.data_ptr()),
                              ctypes.c_void_p(cnt.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.LG_OK, lib.lg_last_error()
    torch.cuda.synchronize()
    return E.cpu().numpy(), cnt.cpu().numpy()


def nearest(E, others):
    return min(min(np.abs(E - o).max(), np.abs(E + o).max()) for o in others)


def test_solver_matches_the_companion_route(golden, solved):
    E, cnt = solved
    bar, kind = float(golden["pose_abs_bar"]), golden["solver/kind"]
    np.testing.assert_array_equal(cnt[kind < 3], golden["solver/count"][kind < 3])
    worst = 0.0
    for s in np.nonzero(kind < 3)[0]:
        want = golden["solver/E"][s, :cnt[s]]
        used = set()
        for j in range(cnt[s]):  # one to one: each candidate's nearest is its own
            d = [min(np.abs(E[s, j] - w).max(), np.abs(E[s, j] + w).max()) for w in want]
            k = int(np.argmin(d))
            assert k not in used, (s, j)
            used.add(k)
            worst = max(worst, d[k])
    print(f"solver: largest candidate difference to the companion route {worst:.3e}, bar {bar:.3e}")
    assert worst <= bar


def test_solver_candidates_meet_the_constraints(golden, solved):
    E, cnt = solved
    P = golden["solver/pts"].astype(np.float64)
    bar, worst = float(golden["solver_res_bar"]), 0.0
    for s in range(64):
        for j in range(cnt[s]):
            e = E[s, j].reshape(3, 3)
            assert abs(np.linalg.norm(e) - 1.0) < 1e-12
            x0 = np.concatenate([P[s, :, :2], np.ones((5, 1))], 1)
            x1 = np.concatenate([P[s, :, 2:], np.ones((5, 1))], 1)
            r = max(np.abs(np.einsum("ki,ij,kj->k", x1, e, x0)).max(), abs(np.linalg.det(e)),
                    np.linalg.norm(2 * e @ e.T @ e - np.trace(e @ e.T) * e))
            worst = max(worst, r)
    print(f"solver: largest constraint residual {worst:.3e}, companion route {float(golden['solver_res_companion']):.3e}, "
          f"bar {bar:.3e}")
    assert worst <= bar


def test_solver_finds_the_true_matrix_and_leaves_the_rest_alone(golden, solved):
    E, cnt = solved
    kind, bar = golden["solver/kind"], float(golden["pose_abs_bar"])
    for s in np.nonzero(kind < 2)[0]:  # noise free: the true E is a candidate, as near as the companion route has it
        d = nearest(golden["solver/E_true"][s], E[s, :cnt[s]])
        assert d <= golden["solver/true_dist"][s] + bar, (s, d)
    rep = int(np.nonzero(kind == 3)[0][0])  # the repeated point: finite candidates, or none
    assert 0 <= cnt[rep] <= 10 and np.isfinite(E[rep, :cnt[rep]]).all()
    for s in range(64):  # nothing past count is written
        assert 0 <= cnt[s] <= 10 and (E[s, cnt[s]:] == -7.0).all() and np.isfinite(E[s, :cnt[s]]).all()


# ---- every fixture case through the C ABI ---------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_case(golden, name):
    g = golden
    got = case_call(g, name)
    want = restate(g, name)
    np.testing.assert_array_equal(ref.info_row(want), g[f"{name}/info"])  # the restatement is the fixture's
    against_restatement(got, want, 0, g, name, T_gt=g[f"{name}/T_gt"])
    K = want["num_matches"]
    np.testing.assert_array_equal(got["m_kpts"][0][:K], want["m_kpts"])
    assert (got["m_kpts"][0][K:] == -123.5).all()  # rows past the matches are not written
    self_consistent(got["R"][0], got["t"][0], got["inliers"][0], g[f"{name}/kpts0"], g[f"{name}/kpts1"],
                    g[f"{name}/matches0"], g[f"{name}/camera0"], g[f"{name}/camera1"], float(g[f"{name}/th"]))
    assert got["info"][0][7] >= 0


@pytest.mark.parametrize("name", ["lds", "lds_plus_1"])
def test_both_sides_of_the_lds_threshold(golden, name):
    """K = LDS_MATCHES runs from LDS, one more from m_kpts in global memory: both equal the restatement."""
    from lightglue_amd import robust

    g = golden
    assert len(g[f"{name}/kpts0"]) == robust.LDS_MATCHES + (name == "lds_plus_1") and int(g[f"{name}/max_iters"]) == 256
    got = case_call(g, name)
    want = dict(zip(ref.INFO_FIELDS, g[f"{name}/info"].tolist()))
    want.update(inliers_slots=g[f"{name}/inliers"], R=g[f"{name}/R"], t=g[f"{name}/t"], margin=float(g[f"{name}/margin"]))
    against_restatement(got, want, 0, g, name, T_gt=g[f"{name}/T_gt"])  # tests/test_relpose_golden.py restates it
    self_consistent(got["R"][0], got["t"][0], got["inliers"][0], g[f"{name}/kpts0"], g[f"{name}/kpts1"],
                    g[f"{name}/matches0"], g[f"{name}/camera0"], g[f"{name}/camera1"], float(g[f"{name}/th"]))


# ---- what no fixture can hold -------------------------------------------------------------------------
def ragged_batch(g):
    """Five pairs of different sizes, padded to one capacity with rubbish, in a shuffled order."""
    names = ["keypoints", "one_round", "none", "intrinsics", "five_exact"]
    M = max(len(g[f"{n}/kpts0"]) for n in names) + 9
    N = max(len(g[f"{n}/kpts1"]) for n in names) + 5
    rng = np.random.default_rng(3)
    kp0 = rng.uniform(0, 1600, (5, M, 2)).astype(np.float32)
    kp1 = rng.uniform(0, 1600, (5, N, 2)).astype(np.float32)
    m0 = rng.integers(-1, N, (5, M)).astype(np.int64)  # padding slots hold plausible matches: the counts rule
    n0, n1 = np.zeros(5, dtype=np.int32), np.zeros(5, dtype=np.int32)
    for b, n in enumerate(names):
        n0[b], n1[b] = len(g[f"{n}/kpts0"]), len(g[f"{n}/kpts1"])
        kp0[b, :n0[b]], kp1[b, :n1[b]], m0[b, :n0[b]] = g[f"{n}/kpts0"], g[f"{n}/kpts1"], g[f"{n}/matches0"]
    cam0 = np.stack([g[f"{n}/camera0"] for n in names])
    cam1 = np.stack([g[f"{n}/camera1"] for n in names])
    T = np.stack([g[f"{n}/T_gt"] for n in names])
    return names, kp0, kp1, m0, n0, n1, cam0, cam1, T


def test_ragged_permuted_batch_equals_its_pairs_alone(golden):
    g = golden
    names, kp0, kp1, m0, n0, n1, cam0, cam1, T = ragged_batch(g)
    th = np.array([float(g[f"{n}/th"]) for n in names], dtype=np.float32)
    opt = {"max_iters": 512, "confidence": 0.9999, "seed": 0}
    both = abi_call(dev(kp0), dev(kp1), dev(m0), dev(cam0), dev(cam1), dev(th), dev(n0), dev(n1), T_gt=dev(T), **opt)
    for b, n in enumerate(names):
        one = lambda a: dev(a[b:b + 1])  # noqa: E731
        alone = abi_call(one(kp0), one(kp1), one(m0), one(cam0), one(cam1), one(th), one(n0), one(n1), T_gt=one(T), **opt)
        for k in ("R", "t", "inliers", "info", "errors"):
            np.testing.assert_array_equal(both[k][b], alone[k][0], err_msg=f"{n} {k}")
        K = both["info"][b][1]
        np.testing.assert_array_equal(both["m_kpts"][b][:K], alone["m_kpts"][0][:K])
        # and it is the fixture's case: the padding changed nothing
        np.testing.assert_array_equal(both["info"][b][:7], g[f"{n}/info"][:7], err_msg=n)
        np.testing.assert_array_equal(both["inliers"][b][:n0[b]].astype(bool), g[f"{n}/inliers"], err_msg=n)
        assert not both["inliers"][b][n0[b]:].any()
        self_consistent(both["R"][b], both["t"][b], both["inliers"][b], kp0[b], kp1[b], m0[b], cam0[b], cam1[b], th[b],
                        n0[b], n1[b])
    perm = np.array([3, 0, 4, 2, 1])
    p = lambda a: dev(a[perm])  # noqa: E731
    shuffled = abi_call(p(kp0), p(kp1), p(m0), p(cam0), p(cam1), p(th), p(n0), p(n1), T_gt=p(T), **opt)
    for k in ("R", "t", "inliers", "info", "errors"):
        np.testing.assert_array_equal(shuffled[k], both[k][perm], err_msg=k)


def test_per_pair_thresholds_and_run_to_run_bits(golden):
    g, n = golden, "forward"
    rep = lambda a, k=3: dev(np.repeat(np.asarray(a)[None], k, 0))  # noqa: E731
    th = np.array([0.5, 1.0, 2.0], dtype=np.float32)
    args = (rep(g[f"{n}/kpts0"]), rep(g[f"{n}/kpts1"]), rep(g[f"{n}/matches0"]), rep(g[f"{n}/camera0"]),
            rep(g[f"{n}/camera1"]), dev(th))
    a = abi_call(*args, T_gt=rep(g[f"{n}/T_gt"]), **options(g, n))
    b = abi_call(*args, T_gt=rep(g[f"{n}/T_gt"]), **options(g, n))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)  # the same bits
    np.testing.assert_array_equal(a["info"][1][:7], g[f"{n}/info"][:7])  # th = 1.0 is the fixture's
    for i in range(3):
        self_consistent(a["R"][i], a["t"][i], a["inliers"][i], g[f"{n}/kpts0"], g[f"{n}/kpts1"], g[f"{n}/matches0"],
                        g[f"{n}/camera0"], g[f"{n}/camera1"], th[i])
    assert a["info"][0][2] < a["info"][1][2] < a["info"][2][2] and (a["info"][:, 0] == 1).all()


def test_relative_pose_estimator_single_and_batched(golden):
    from lightglue_amd import relative_pose as rp
    from lightglue_amd.depth_matcher import Camera, Pose

    g, n = golden, "one_round"
    est = rp.RelativePoseEstimator({"ransac_th": float(g[f"{n}/th"]), "options": options(g, n)})
    p0, p1 = dev(g[f"{n}/kpts0"]), dev(g[f"{n}/kpts1"])
    cam = Camera(dev(cam6(g[f"{n}/camera0"])))
    one = est({"m_kpts0": p0, "m_kpts1": p1, "camera0": cam, "camera1": cam})
    assert one["success"] is True and isinstance(one["M_0to1"], Pose) and one["M_0to1"].R.shape == (3, 3)
    np.testing.assert_array_equal(one["inliers"].cpu().numpy(), g[f"{n}/inliers"])
    bar = float(g["pose_abs_bar"])
    assert np.abs(one["M_0to1"].R.cpu().numpy() - g[f"{n}/R"]).max() <= bar
    assert np.abs(one["M_0to1"].t.cpu().numpy() - g[f"{n}/t"]).max() <= bar
    # batched: the pair, the pair cut to 40 matches through num_matches, and an empty pair
    nm = torch.tensor([80, 40, 0], dtype=torch.int32, device="cuda")
    rows = dev(np.repeat(cam6(g[f"{n}/camera0"])[None], 3, 0))
    out = est({"m_kpts0": p0[None].repeat(3, 1, 1), "m_kpts1": p1[None].repeat(3, 1, 1), "camera0": rows, "camera1": rows,
               "num_matches": nm})
    assert out["success"].tolist() == [True, True, False] and out["success"].is_cuda and out["inliers"].shape == (3, 80)
    assert torch.equal(out["M_0to1"].R[0], one["M_0to1"].R) and torch.equal(out["inliers"][0], one["inliers"])
    assert out["info"][:, 1].tolist() == [80, 40, 0] and not out["inliers"][1, 40:].any()
    want = ref.estimate_pair(g[f"{n}/kpts0"][:40], g[f"{n}/kpts1"][:40], None, g[f"{n}/camera0"], g[f"{n}/camera1"],
                             float(g[f"{n}/th"]), **options(g, n))
    print(f"cut to 40: restatement info {ref.info_row(want).tolist()}, margin {want['margin']:.3e}")
    assert want["margin"] >= 1e-7
    np.testing.assert_array_equal(out["info"][1, :7].cpu().numpy(), ref.info_row(want)[:7])
    np.testing.assert_array_equal(out["inliers"][1, :40].cpu().numpy(), want["inliers_slots"])
    assert torch.equal(out["M_0to1"].R[2].cpu(), torch.eye(3)) and not out["M_0to1"].t[2].any()


def test_matcher_output_goes_straight_into_the_robust_evaluation():
    """TwoViewPipeline with the nearest-neighbour matcher on synthetic descriptors (B = 2, 96 and 80
    keypoints, 60 true matches each on a noise-free scene): its ``pred`` is evaluated as it is."""
    from lightglue_amd import relative_pose as rp
    from lightglue_amd.pipeline import TwoViewPipeline

    rng = np.random.default_rng(11)
    B, M, N, D = 2, 96, 80, 64
    cam = np.array([1000.0, 1010.0, 800.0, 600.0])
    k0 = rng.uniform([100, 100], [1500, 1100], (B, M, 2))
    d0 = rng.normal(size=(B, M, D))
    k1, d1 = rng.uniform([0, 0], [1600, 1200], (B, N, 2)), rng.normal(size=(B, N, D))
    T = np.zeros((B, 12))
    for b in range(B):  # 60 true correspondences at shuffled slots
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + np.sin(0.15) * kx + (1 - np.cos(0.15)) * kx @ kx
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        T[b] = np.concatenate([R.reshape(9), t])
        src, dst = rng.permutation(M)[:60], rng.permutation(N)[:60]
        z = rng.uniform(4, 9, 60)
        X = np.stack([(k0[b, src, 0] - cam[2]) / cam[0] * z, (k0[b, src, 1] - cam[3]) / cam[1] * z, z], 1)
        Y = X @ R.T + t
        k1[b, dst] = np.stack([Y[:, 0] / Y[:, 2] * cam[0] + cam[2], Y[:, 1] / Y[:, 2] * cam[1] + cam[3]], 1)
        d1[b, dst] = d0[b, src] + 0.1 * rng.normal(size=(60, D))
    unit = lambda d: (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)  # noqa: E731
    size = torch.tensor([[1600.0, 1200.0]]).repeat(B, 1).cuda()
    rows = dev(np.repeat(cam6(cam)[None], B, 0))
    data = {"view0": {"image_size": size, "camera": rows,
                      "cache": {"keypoints": dev(k0.astype(np.float32)), "descriptors": dev(unit(d0))}},
            "view1": {"image_size": size, "camera": rows,
                      "cache": {"keypoints": dev(k1.astype(np.float32)), "descriptors": dev(unit(d1))}},
            "T_0to1": dev(T.astype(np.float32))}
    pipe = TwoViewPipeline({"extractor": {"name": None}, "allow_no_extract": True,
                            "matcher": {"name": "matchers.nearest_neighbor_matcher", "ratio_thresh": 0.9}})
    with torch.no_grad():
        pred = pipe(data)
    conf = {"estimator": "hip", "ransac_th": 1.0, "options": {"max_iters": 512, "seed": 1}}
    out = rp.eval_relative_pose_robust(data, pred, conf)
    assert set(out) == {"rel_pose_error", "ransac_inl", "ransac_inl%", "M_0to1", "inliers"}
    assert all(out[k].is_cuda for k in ("rel_pose_error", "ransac_inl", "ransac_inl%", "inliers"))
    assert out["rel_pose_error"].shape == (B,) and out["M_0to1"].R.shape == (B, 3, 3) and out["inliers"].shape == (B, M)
    cb = rp.as_export_callback(conf)(pred, data)
    assert all(torch.equal(cb[k], out[k]) for k in ("rel_pose_error", "ransac_inl", "ransac_inl%", "inliers"))
    m0 = pred["matches0"].cpu().numpy()
    for b in range(B):
        nm = int((m0[b] > -1).sum())
        print(f"pair {b}: {nm} matches, {int(out['ransac_inl'][b])} inliers, rel_pose_error "
              f"{float(out['rel_pose_error'][b]):.4g} deg")
        assert nm >= 30 and float(out["ransac_inl"][b]) >= 0.5 * nm  # at least half are true matches
        assert float(out["rel_pose_error"][b]) < 1.0  # a sanity bound on a noise-free scene, not a tolerance
        assert float(out["ransac_inl%"][b]) == float(np.float32(out["ransac_inl"][b].item()) / np.float32(nm))
        assert int(out["inliers"][b].sum()) == int(out["ransac_inl"][b])
    # one pair without the batch dimension: Python numbers, element 0 of the batched form
    d0_ = {"T_0to1": data["T_0to1"][0], "view0": {"camera": rows[0]}, "view1": {"camera": rows[0]}}
    p0_ = {k: pred[k][0] for k in ("keypoints0", "keypoints1", "matches0", "matching_scores0")}
    one = rp.eval_relative_pose_robust(d0_, p0_, conf)
    for k in ("rel_pose_error", "ransac_inl", "ransac_inl%"):
        assert isinstance(one[k], float) and one[k] == float(out[k][0]), k
    assert torch.equal(one["M_0to1"].R, out["M_0to1"].R[0]) and torch.equal(one["inliers"], out["inliers"][0])
