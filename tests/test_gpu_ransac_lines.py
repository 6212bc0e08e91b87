"""Hybrid point-and-line LO-RANSAC on the device (lightglue_amd.robust, csrc/ransac_homography_lines.hip)
-- needs an MI355X.  Every case of tests/golden/ransac_lines/ransac_lines.npz through the C ABI on
prefilled outputs: the info row and both masks equal the float64 restatement's (tests/
ransac_lines_ref.py; the fixture's margins are what makes that a fair demand), H_error within the
project's DLT bar (``dlt_rel_bar`` of tests/golden/match_eval/match_eval.npz), as
tests/test_gpu_ransac.py uses it.  Then what no fixture can hold: the LDS capacities' edges, the sampler
pinned without the restatement, batch positions, run-to-run bits, swapped endpoints, the estimator
contract, ``eval_homography_robust`` and one pass from the wireframe through GlueStick."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import ransac_lines_ref as ref
from ransac_ref import sample

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ransac_lines_golden as gen  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "ransac_lines", "ransac_lines.npz")
MIN_MARGIN = 1e-7
FILL = -123.5
SIZE = np.array([640.0, 480.0], dtype=np.float32)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def bar():
    v = float(np.load(os.path.join(HERE, "golden", "match_eval", "match_eval.npz"))["dlt_rel_bar"])
    assert abs(v - 2.059e-5) < 1e-8
    return v


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def abi_call(inp, th, H_gt=None, size0=None, **opt):
    """lg_ransac_homography_lines through ctypes on prefilled outputs; everything back on the host.
    ``inp``: batched numpy arrays under the fixture's names (``num0/1`` and ``num_lines0/1`` optional)."""
    from lightglue_amd import _lib

    lib = _lib.load()
    t = {k: dev(v) for k, v in inp.items()}
    B, M, N = t["kpts0"].shape[0], t["kpts0"].shape[1], t["kpts1"].shape[1]
    L0, L1 = t["lines0"].shape[1], t["lines1"].shape[1]
    th, H_gt, size0 = dev(np.asarray(th, dtype=np.float32).reshape(-1)), dev(H_gt), dev(size0)
    ptr = lambda x: None if x is None or x.numel() == 0 else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    H = torch.full((B, 9), FILL, device="cuda")
    inl = torch.full((B, M), 77, dtype=torch.uint8, device="cuda")
    linl = torch.full((B, L0), 77, dtype=torch.uint8, device="cuda")
    info = torch.full((B, 12), -77, dtype=torch.int32, device="cuda")
    mk, ml = torch.full((B, M, 4), FILL, device="cuda"), torch.full((B, L0, 8), FILL, device="cuda")
    err = torch.full((B,), FILL, device="cuda") if H_gt is not None else None
    rc = lib.lg_ransac_homography_lines(
        ptr(t["kpts0"]), ptr(t["kpts1"]), ptr(t.get("matches0")), B, M, N, ptr(t.get("num0")), ptr(t.get("num1")),
        ptr(t["lines0"]), ptr(t["lines1"]), ptr(t.get("line_matches0")), L0, L1, ptr(t.get("num_lines0")),
        ptr(t.get("num_lines1")), ptr(th), opt["max_iters"], opt["confidence"], opt["seed"], opt["min_line_length"], ptr(H_gt),
        ptr(size0), ptr(H), ptr(inl), ptr(linl), ptr(info), ptr(mk), ptr(ml), ptr(err),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.LG_OK, lib.lg_last_error()
    torch.cuda.synchronize()
    out = {"H": H.cpu().numpy().reshape(B, 3, 3), "inliers": inl.cpu().numpy(), "line_inliers": linl.cpu().numpy(),
           "info": info.cpu().numpy(), "m_kpts": mk.cpu().numpy(), "m_lines": ml.cpu().numpy()}
    if err is not None:
        out["H_error"] = err.cpu().numpy()
    return out


def case_inputs(g, name):
    """One fixture case as a batch of one."""
    inp = {k: g[f"{name}/{k}"][None] for k in gen.INPUTS}
    for k in ("num_lines0", "num_lines1"):
        if f"{name}/{k}" in g:
            inp[k] = np.array([g[f"{name}/{k}"]], dtype=np.int32)
    return inp


def options(g, name):
    return {"max_iters": int(g[f"{name}/max_iters"]), "confidence": float(g[f"{name}/confidence"]),
            "seed": int(g[f"{name}/seed"]), "min_line_length": float(g[f"{name}/min_line_length"])}


def case_call(g, name, inp=None, th=None, **over):
    return abi_call(inp or case_inputs(g, name), g[f"{name}/th"] if th is None else th, H_gt=g[f"{name}/H_gt"][None],
                    size0=g[f"{name}/size0"][None], **{**options(g, name), **over})


def self_consistent(got, b, inp, th, min_line_length=1.0):
    """Both masks are the fp64 classification in pixels under the returned fp32 matrix, nothing else."""
    one = {k: v[b] for k, v in inp.items()}
    pts, slots = ref.live_matches(one["kpts0"], one["kpts1"], one.get("matches0"), one.get("num0"), one.get("num1"))
    lns, lslots = ref.live_lines(one["lines0"], one["lines1"], one.get("line_matches0"), one.get("num_lines0"),
                                 one.get("num_lines1"), min_line_length)
    want, lwant = np.zeros(one["kpts0"].shape[0], dtype=bool), np.zeros(one["lines0"].shape[0], dtype=bool)
    if got["info"][b, 0]:
        want[slots], lwant[lslots] = ref.classify(got["H"][b].astype(np.float64), pts, lns[:, :4], ref.segment_line(lns[:, 4:]),
                                                  float(np.float32(th)), ref._Margin())
    np.testing.assert_array_equal(got["inliers"][b].astype(bool), want)
    np.testing.assert_array_equal(got["line_inliers"][b].astype(bool), lwant)


def against_restatement(got, want, b, bar, what):
    """One pair of a device result against the restatement's dict."""
    info = got["info"][b]
    print(f"{what}: info {info[:9].tolist()}, restatement {ref.info_row(want)[:9].tolist()}, margin {want['margin']:.3e}")
    assert want["margin"] >= MIN_MARGIN, what
    np.testing.assert_array_equal(info, ref.info_row(want), err_msg=what)
    np.testing.assert_array_equal(got["inliers"][b].astype(bool), want["inliers_slots"], err_msg=what)
    np.testing.assert_array_equal(got["line_inliers"][b].astype(bool), want["line_inliers_slots"], err_msg=what)
    assert set(np.unique(got["inliers"][b])) | set(np.unique(got["line_inliers"][b])) <= {0, 1}
    Kp, Kl = len(want["m_kpts"]), len(want["m_lines"])
    np.testing.assert_array_equal(got["m_kpts"][b, :Kp], want["m_kpts"])  # the compaction buffers: nothing past the rows
    np.testing.assert_array_equal(got["m_lines"][b, :Kl], want["m_lines"])
    assert (got["m_kpts"][b, Kp:] == FILL).all() and (got["m_lines"][b, Kl:] == FILL).all()
    e, w = float(got["H_error"][b]), want["H_error"]
    print(f"{what}: H_error {e:.9g}, restatement {w:.9g}, bar {bar:.3e}")
    if want["success"]:
        assert abs(e - w) <= bar * w, what
        assert got["H"][b][2, 2] == 1.0
        assert np.abs(got["H"][b] - want["H"]).max() <= bar * np.abs(want["H"]).max()
    else:
        assert math.isinf(e) and e > 0, what
        np.testing.assert_array_equal(got["H"][b], np.eye(3, dtype=np.float32))
        assert not got["inliers"][b].any() and not got["line_inliers"][b].any()


def stored(g, name):
    want = dict(zip(ref.INFO_FIELDS, g[f"{name}/info"].tolist()))
    want.update(inliers_slots=g[f"{name}/inliers"], line_inliers_slots=g[f"{name}/line_inliers"], H=g[f"{name}/H"],
                H_error=float(g[f"{name}/H_error"]), margin=float(g[f"{name}/margin"]), m_kpts=g[f"{name}/m_kpts"],
                m_lines=g[f"{name}/m_lines"])
    return want


@pytest.mark.parametrize("name", gen.CASES)
def test_every_fixture_case_through_the_c_abi(golden, bar, name):
    g = golden
    inp = case_inputs(g, name)
    got = case_call(g, name, inp)
    against_restatement(got, stored(g, name), 0, bar, f"case {name}")
    self_consistent(got, 0, inp, g[f"{name}/th"])


def test_three_points_and_two_lines_succeed_where_the_points_alone_cannot(golden):
    from lightglue_amd import robust

    g = golden
    assert case_call(g, "three_two")["info"][0, :5].tolist() == [1, 3, 2, 3, 2]
    r = robust.ransac_homography(dev(g["three_two/kpts0"][None]), dev(g["three_two/kpts1"][None]), None, 2.0)
    assert r["info"][0, :2].tolist() == [0, 3]  # K < 4


@pytest.mark.parametrize("which", ["points", "lines", "both"])
def test_more_features_than_lds_holds_run_from_global_memory(bar, which):
    """Each set at its LDS capacity (through the counts) and one past it, max_iters 256, against the
    restatement; generator seeds in a fixed order, the first whose margins pass the fixture's rule."""
    from lightglue_amd import robust

    cp, cl = robust.LDS_POINTS, robust.LDS_LINES
    n_p, n_l = {"points": (cp + 1, 8), "lines": (8, cl + 1), "both": (cp + 1, cl + 1)}[which]
    opt = {"max_iters": 256, "confidence": 0.995, "seed": 3, "min_line_length": 1.0}
    H_gt = gen.H_GT.astype(np.float32)

    def restate(s, np_, nl_):
        return ref.estimate_pair(s["kpts0"], s["kpts1"], None, s["lines0"], s["lines1"], None, 2.0, np_, np_, nl_, nl_,
                                 H_gt=H_gt, size=SIZE, max_iters=256, confidence=0.995, seed=3)

    for gen_seed in range(20):
        s = gen.scene(np.random.default_rng(2000 + gen_seed), n_p, n_l, 0.5, 0.5)
        del s["matches0"], s["line_matches0"]
        # one feature fewer of each oversized set fits LDS exactly: the leading ones, under the same rule
        fit_p, fit_l = min(n_p, cp), min(n_l, cl)
        want, want2 = restate(s, n_p, n_l), restate(s, fit_p, fit_l)
        if min(want["margin"], want2["margin"]) >= MIN_MARGIN:
            break
    else:
        pytest.fail("no generator seed passes the margin rule")
    assert (want["num_point_matches"], want["num_line_matches"]) == (n_p, n_l) and want["success"] and want["rounds"] == 1
    assert (want2["num_point_matches"], want2["num_line_matches"]) == (fit_p, fit_l) and want2["success"]
    inp = {k: v[None] for k, v in s.items()}
    got = abi_call(inp, 2.0, H_gt[None], SIZE[None], **opt)
    against_restatement(got, want, 0, bar, f"{which}: Kp = {n_p}, Kl = {n_l} (generator seed {2000 + gen_seed})")
    self_consistent(got, 0, inp, 2.0)
    i32 = lambda v: np.array([v], dtype=np.int32)  # noqa: E731
    inp2 = {**inp, "num0": i32(fit_p), "num1": i32(fit_p), "num_lines0": i32(fit_l), "num_lines1": i32(fit_l)}
    got2 = abi_call(inp2, 2.0, H_gt[None], SIZE[None], **opt)
    against_restatement(got2, want2, 0, bar, f"{which}: Kp = {fit_p}, Kl = {fit_l}")
    self_consistent(got2, 0, inp2, 2.0)


def test_kernel_sampler_and_the_two_plus_two_rule():
    """The kernel's own sampler, hypothesis by hypothesis.  Six exact points and six exact segments of a
    translation on integer pixels, all in general position: a sample of four distinct features is valid
    if and only if it is not two points with two lines, and every valid hypothesis explains all twelve.
    So ``valid_hypotheses`` under a cap of n counts such samples among t < n and ``best_t`` is the first
    of them: both follow from the specification's index sequence alone (features 0-5 are the points)."""
    P = np.array([[50, 60], [600, 40], [580, 430], [70, 400], [320, 250], [200, 130]], dtype=np.float32)
    L = np.array([[[100, 80], [300, 120]], [[450, 60], [520, 300]], [[90, 350], [260, 300]], [[400, 400], [610, 330]],
                  [[150, 200], [380, 180]], [[330, 90], [470, 410]]], dtype=np.float32)
    shift = np.array([7, -3], dtype=np.float32)
    inp = {"kpts0": P[None], "kpts1": (P + shift)[None], "lines0": L[None], "lines1": (L + shift)[None]}
    seen = set()
    for seed in (0, 1, 2, 12345, 2**63 + 5):
        valid = [sum(i < 6 for i in sample(seed, t, 12)) != 2 for t in range(256)]
        seen.add(tuple(valid))
        for cap in (1, 37, 256):
            got = abi_call(inp, 1.0, max_iters=cap, confidence=0.995, seed=seed, min_line_length=1.0)
            n = sum(valid[:cap])
            first = valid.index(True) if n else -1
            want = [int(n > 0), 6, 6, 6 if n else 0, 6 if n else 0, first, 12 if n else 0, 1, n, 0, 0, 0]
            assert got["info"][0].tolist() == want, (seed, cap)
    assert len(seen) == 5 and all(0 < sum(v) < 256 for v in seen)  # another seed, another sequence; both kinds occur


def test_a_pair_is_the_same_alone_and_anywhere_in_a_batch(golden):
    g = golden
    one = case_inputs(g, "mixed")
    alone = case_call(g, "mixed", one)
    five = {k: np.concatenate([v] * 5) for k, v in one.items()}
    others = [0.5, 1.0, 3.0, 4.0]
    rep = lambda k: np.concatenate([g[f"mixed/{k}"][None]] * 5)  # noqa: E731
    for pos in range(5):
        th = np.array(others[:pos] + [float(g["mixed/th"])] + others[pos:], dtype=np.float32)
        got = abi_call(five, th, rep("H_gt"), rep("size0"), **options(g, "mixed"))
        for k in alone:
            assert got[k][pos].tobytes() == alone[k][0].tobytes(), (pos, k)
        for b in range(5):
            self_consistent(got, b, five, th[b])
        n = got["info"][:, 3] + got["info"][:, 4]
        assert n[np.argmin(th)] < n[np.argmax(th)]  # a wider threshold, more inliers


def test_run_to_run_bits_and_another_seed(golden):
    g = golden
    a, b = case_call(g, "rounds"), case_call(g, "rounds")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = case_call(g, "rounds", seed=12345)
    assert c["info"][0, 5] != a["info"][0, 5] and c["info"][0, 0] == 1
    self_consistent(c, 0, case_inputs(g, "rounds"), g["rounds/th"])
    assert c["info"][0, 3] == c["inliers"][0].sum() and c["info"][0, 4] == c["line_inliers"][0].sum()


@pytest.mark.parametrize("name", ["mixed", "pieces", "ragged"])
def test_swapping_image1_endpoints_moves_no_bit_but_m_lines(golden, name):
    g = golden
    inp = case_inputs(g, name)
    a = case_call(g, name, inp)
    b = case_call(g, name, {**inp, "lines1": inp["lines1"][:, :, ::-1]})
    for k in a:
        if k != "m_lines":
            assert a[k].tobytes() == b[k].tobytes(), k
    Kl = int(a["info"][0, 2])
    swapped = a["m_lines"][0, :Kl].reshape(Kl, 4, 2)[:, [0, 1, 3, 2]].reshape(Kl, 8)
    np.testing.assert_array_equal(b["m_lines"][0, :Kl], swapped)


def test_estimator_contract_single_batched_and_either_key_pair_missing(golden):
    from lightglue_amd import relative_pose, robust

    g = golden
    cls = robust.load_estimator("homography", "homography_est")
    assert cls is robust.PointLineHomographyEstimator is relative_pose.load_estimator("homography", "homography_est")
    for name in ("mixed", "lines_only", "points_only", "k3"):
        pts, lns = g[f"{name}/m_kpts"], g[f"{name}/m_lines"]
        Kp, Kl = len(pts), len(lns)
        opt = options(g, name)
        est = cls({"ransac_th": float(g[f"{name}/th"]), "options": opt})
        data = {"m_kpts0": dev(pts[:, :2]), "m_kpts1": dev(pts[:, 2:]),
                "m_lines0": dev(lns[:, :4].reshape(Kl, 2, 2)), "m_lines1": dev(lns[:, 4:].reshape(Kl, 2, 2))}
        out = est(data)
        assert set(out) == {"success", "M_0to1", "inliers", "line_inliers"} and isinstance(out["success"], bool)
        assert out["M_0to1"].shape == (3, 3) and out["M_0to1"].is_cuda and out["M_0to1"].dtype == torch.float32
        assert out["inliers"].shape == (Kp,) and out["inliers"].dtype == torch.bool
        assert out["line_inliers"].shape == (Kl,) and out["line_inliers"].dtype == torch.bool
        assert out["success"] == bool(g[f"{name}/info"][0])
        # the matched form is the slot form of the same live features: the same bits (the fixture's slot
        # forms of these cases hold exactly their live features, in order)
        low = case_call(g, name)
        np.testing.assert_array_equal(out["M_0to1"].cpu().numpy(), low["H"][0])
        np.testing.assert_array_equal(out["inliers"].cpu().numpy(), low["inliers"][0].astype(bool))
        np.testing.assert_array_equal(out["line_inliers"].cpu().numpy(), low["line_inliers"][0].astype(bool))
        # an empty set may be left out
        if Kl == 0:
            alone = est({k: v for k, v in data.items() if "kpts" in k})
            assert torch.equal(alone["M_0to1"], out["M_0to1"]) and alone["line_inliers"].shape == (0,)
        if Kp == 0:
            alone = est({k: v for k, v in data.items() if "lines" in k})
            assert torch.equal(alone["M_0to1"], out["M_0to1"]) and alone["inliers"].shape == (0,)
        # the batched form: device tensors, the same pair twice, the second cut short by the counts
        if Kp >= 2 and Kl >= 2:
            two = est({**{k: torch.stack([v, v]) for k, v in data.items()}, "num_matches": torch.tensor([Kp, Kp - 1]),
                       "num_line_matches": torch.tensor([Kl, Kl - 1])})
            assert two["success"].shape == (2,) and two["success"].dtype == torch.bool and two["success"].is_cuda
            assert two["M_0to1"].shape == (2, 3, 3) and two["inliers"].shape == (2, Kp) and two["line_inliers"].shape == (2, Kl)
            assert torch.equal(two["M_0to1"][0], out["M_0to1"]) and torch.equal(two["inliers"][0], out["inliers"])
            assert torch.equal(two["line_inliers"][0], out["line_inliers"])
            assert two["info"][1, 1:3].tolist() == [Kp - 1, Kl - 1]
            assert not bool(two["inliers"][1, Kp - 1]) and not bool(two["line_inliers"][1, Kl - 1])
    # lines-only data on the batched form, without any point key
    lns = g["lines_only/m_lines"]
    l0, l1 = dev(lns[:, :4].reshape(1, -1, 2, 2)), dev(lns[:, 4:].reshape(1, -1, 2, 2))
    out = cls({"ransac_th": 2.0, "options": options(g, "lines_only")})({"m_lines0": l0, "m_lines1": l1})
    assert out["success"].tolist() == [True] and out["inliers"].shape == (1, 0)
    np.testing.assert_array_equal(out["M_0to1"][0].cpu().numpy(), case_call(g, "lines_only")["H"][0])


def batch_pred(g, names):
    """Fixture cases of equal shapes as one batch in the matcher's ``pred`` form."""
    st = lambda k: dev(np.stack([g[f"{n}/{k}"] for n in names]))  # noqa: E731
    pred = {"keypoints0": st("kpts0"), "keypoints1": st("kpts1"), "matches0": st("matches0"),
            "matching_scores0": torch.ones(st("matches0").shape, device="cuda"), "lines0": st("lines0"), "lines1": st("lines1"),
            "line_matches0": st("line_matches0"), "line_matching_scores0": torch.ones(st("line_matches0").shape, device="cuda")}
    data = {"H_0to1": st("H_gt"), "view0": {"image_size": st("size0")}}
    return data, pred


def test_eval_homography_robust_with_lines(golden, bar):
    from lightglue_amd import robust

    g = golden
    names = ["mixed", "mixed"]
    data, pred = batch_pred(g, names)
    conf = {"estimator": "homography_est", "ransac_th": float(g["mixed/th"]), "options": options(g, "mixed")}
    out = robust.eval_homography_robust(data, pred, conf)
    assert set(out) == {"H_error_ransac", "ransac_inl", "ransac_inl%", "ransac_line_inl", "M_0to1", "inliers", "line_inliers"}
    assert all(v.is_cuda for v in out.values()) and out["H_error_ransac"].shape == (2,)
    info = g["mixed/info"]
    low = case_call(g, "mixed")
    for b in range(2):
        assert float(out["ransac_inl"][b]) == info[3] + info[4] and float(out["ransac_line_inl"][b]) == info[4]
        assert float(out["ransac_inl%"][b]) == float(np.float32(info[3] + info[4]) / np.float32(info[1] + info[2]))
        np.testing.assert_array_equal(out["M_0to1"][b].cpu().numpy(), low["H"][0])
        np.testing.assert_array_equal(out["inliers"][b].cpu().numpy(), g["mixed/inliers"])
        np.testing.assert_array_equal(out["line_inliers"][b].cpu().numpy(), g["mixed/line_inliers"])
        assert out["H_error_ransac"][b].cpu().numpy().tobytes() == low["H_error"][0].tobytes()
    cb = robust.as_export_callback(conf)(pred, data)
    assert all(torch.equal(cb[k], out[k]) for k in out)
    # one pair without the batch dimension: Python numbers, element 0 of the batched form
    one = robust.eval_homography_robust({"H_0to1": data["H_0to1"][0], "view0": {"image_size": data["view0"]["image_size"][0]}},
                                        {k: v[0] for k, v in pred.items()}, conf)
    for k in ("H_error_ransac", "ransac_inl", "ransac_inl%", "ransac_line_inl"):
        assert isinstance(one[k], float) and one[k] == float(out[k][0]), k
    for k in ("M_0to1", "inliers", "line_inliers"):
        assert torch.equal(one[k], out[k][0]), k
    # orig_lines0/1 take precedence: with nonsense under lines0/1 the result does not move
    junk = {**pred, "orig_lines0": pred["lines0"], "orig_lines1": pred["lines1"], "lines0": pred["lines0"] * 0 + 5,
            "lines1": pred["lines1"] * 0 + 5}
    again = robust.eval_homography_robust(data, junk, conf)
    assert all(torch.equal(again[k], out[k]) for k in out)
    # ragged lines: num_lines0/1 are read
    rdata, rpred = batch_pred(g, ["ragged"])
    rpred["num_lines0"], rpred["num_lines1"] = dev(g["ragged/num_lines0"].reshape(1)), dev(g["ragged/num_lines1"].reshape(1))
    rout = robust.eval_homography_robust(rdata, rpred, {**conf, "options": options(g, "ragged")})
    np.testing.assert_array_equal(rout["line_inliers"][0].cpu().numpy(), g["ragged/line_inliers"])
    np.testing.assert_array_equal(rout["inliers"][0].cpu().numpy(), g["ragged/inliers"])
    # lines only: a pred without point keys
    ldata, lpred = batch_pred(g, ["lines_only"])
    lpred = {k: v for k, v in lpred.items() if "line" in k}
    lout = robust.eval_homography_robust(ldata, lpred, {**conf, "options": options(g, "lines_only")})
    np.testing.assert_array_equal(lout["line_inliers"][0].cpu().numpy(), g["lines_only/line_inliers"])
    assert lout["inliers"].shape == (1, 0) and float(lout["ransac_inl"][0]) == g["lines_only/info"][4]
    # "hip" does not look at lines
    hip = {"estimator": "hip", "ransac_th": 2.0, "options": {"max_iters": 512, "seed": 1}}
    a = robust.eval_homography_robust(data, pred, hip)
    b = robust.eval_homography_robust(data, {k: v for k, v in pred.items() if "line" not in k}, hip)
    assert set(a) == set(b) == {"H_error_ransac", "ransac_inl", "ransac_inl%", "M_0to1", "inliers"}
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_wireframe_to_gluestick_to_the_robust_evaluation():
    """lines.wireframe (segments from the data) -> matchers.gluestick with random weights ->
    eval_homography_robust with "homography_est": whatever the random matcher matched, the evaluation
    equals the low-level call on the same tensors."""
    from lightglue_amd import pipeline, robust
    from lightglue_amd.gs_weights import gluestick_state_dict

    B, L, Hh, Ww = 1, 14, 120, 160
    sp_conf = {"name": "gluefactory_nonfree.superpoint", "dense_outputs": True, "detection_threshold": 0.0,
               "max_num_keypoints": 64, "force_num_keypoints": False}
    ext_conf = {"name": "lines.wireframe", "point_extractor": sp_conf,
                "line_extractor": {"name": None, "force_num_lines": False, "max_num_lines": None}}
    layers = {"GNN_layers": ["self", "cross"] * 2}
    torch.manual_seed(5)
    # filter_threshold 0: a matcher with random weights still matches (every mutual best pair)
    pipe = pipeline.get_model("two_view_pipeline")({"extractor": ext_conf,
                                                    "matcher": {"name": "matchers.gluestick", "filter_threshold": 0.0, **layers}})
    pipe = pipe.eval().cuda()
    pipe.matcher.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in gluestick_state_dict(layers, seed=2).items()},
                                 strict=True)
    gt = torch.Generator().manual_seed(21)
    data = {"H_0to1": torch.eye(3)[None].cuda()}
    for v in "01":
        a = torch.rand((B, L, 1, 2), generator=gt) * torch.tensor([Ww - 41.0, Hh - 41.0]) + 20
        lines = torch.cat([a, a + (torch.rand((B, L, 1, 2), generator=gt) - 0.5) * 40], dim=2)
        data["view" + v] = {"image": torch.rand((B, 1, Hh, Ww), generator=gt).cuda(), "lines": lines.cuda(),
                            "line_scores": (torch.rand((B, L), generator=gt) + 0.1).cuda(),
                            "image_size": torch.tensor([[float(Ww), float(Hh)]] * B).cuda()}
    with torch.no_grad():
        pred = pipe(data)
    assert pred["line_matches0"].shape == (B, L) and "lines0" in pred
    conf = {"estimator": "homography_est", "ransac_th": 2.0, "options": {"max_iters": 256, "seed": 4}}
    out = robust.eval_homography_robust(data, pred, conf)
    l0, l1 = (pred["orig_lines0"], pred["orig_lines1"]) if "orig_lines0" in pred else (pred["lines0"], pred["lines1"])
    low = robust.ransac_homography_lines(pred["keypoints0"], pred["keypoints1"], pred["matches0"], l0, l1, pred["line_matches0"],
                                         2.0, pred.get("num_keypoints0"), pred.get("num_keypoints1"), pred.get("num_lines0"),
                                         pred.get("num_lines1"), max_iters=256, seed=4, H_gt=data["H_0to1"],
                                         image_size0=data["view0"]["image_size"])
    info = low["info"]
    print("end to end: info", info[0, :9].tolist())
    assert torch.equal(out["M_0to1"], low["H"]) and torch.equal(out["inliers"], low["inliers"])
    assert torch.equal(out["line_inliers"], low["line_inliers"]) and torch.equal(out["H_error_ransac"], low["H_error"])
    assert torch.equal(out["ransac_inl"], (info[:, 3] + info[:, 4]).float())
    assert torch.equal(out["ransac_line_inl"], info[:, 4].float())
