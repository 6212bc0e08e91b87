"""The homography ground truth on the device (lightglue_amd.gt_matcher, csrc/gt_match.hip) against
the fixtures the reference produced (tests/golden/make_gt_golden.py), and the pipeline's training
step end to end: ``pipe.loss(pipe(data), data)["total"]`` from the HIP ground truth to the last
gradient -- needs an MI355X.

Bars: the exact fixture bit for bit in all eight outputs; the random fixtures equal on every item the
fixture's fp64 margins decide (tests/gt_ref.py), projections within the recorded tolerance; the
pipeline's losses and parameter gradients bit-identical to the matcher's own ``loss`` on the same
``gt_*`` tensors (same kernels, same inputs)."""
import functools

import numpy as np
import pytest
import torch

import gt_ref
import lgamd  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ["assignment", "reward", "matches0", "matches1", "matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0"]


def _matcher(**conf):
    from lightglue_amd.pipeline import get_model

    return get_model("matchers.homography_matcher")(conf)


def _feed(g):
    return {"keypoints0": torch.from_numpy(g["keypoints0"]).to(DEV), "keypoints1": torch.from_numpy(g["keypoints1"]).to(DEV),
            "H_0to1": torch.from_numpy(g["H_0to1"]).to(DEV)}


@functools.lru_cache(maxsize=None)
def _run(name, reward=True):
    """One device run per fixture and flavour, shared by the tests below (read-only)."""
    g, meta = gt_ref.load_fixture(name)
    out = _matcher(th_positive=meta["th_positive"], th_negative=meta["th_negative"], reward=reward)(_feed(g))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, out


@pytest.mark.parametrize("name", gt_ref.fixture_names())
def test_matcher_matches_reference_fixture(name):
    g, meta = gt_ref.load_fixture(name)
    got, dev = _run(name)
    assert list(got) == KEYS
    assert dev["assignment"].dtype == torch.bool and dev["matches0"].dtype == torch.int64
    assert dev["reward"].dtype == torch.float32 and dev["matches1"].dtype == torch.int64
    gt_ref.check_against_fixture(got, g, meta)


@pytest.mark.parametrize("name", gt_ref.fixture_names())
def test_structure_of_the_outputs(name):
    """At most one positive per row and per column; matches0 / matches1 agree wherever both point at
    each other; the scores are (matches > -1); a positive's row and column carry it unless the
    negative threshold overrode them with -1."""
    got, _ = _run(name)
    a, m0, m1 = got["assignment"], got["matches0"], got["matches1"]
    assert a.sum(2).max() <= 1 and a.sum(1).max() <= 1
    for b in range(a.shape[0]):
        i = np.nonzero(m0[b] >= 0)[0]
        back = m1[b][m0[b][i]]
        assert np.all((back == i) | (back < 0)), "matches0 -> matches1 is inconsistent"
        assert np.all(a[b][i, m0[b][i]])
        j = np.nonzero(m1[b] >= 0)[0]
        back = m0[b][m1[b][j]]
        assert np.all((back == j) | (back < 0)), "matches1 -> matches0 is inconsistent"
        assert np.all(a[b][m1[b][j], j])
        bi, bj = np.nonzero(a[b])
        assert np.all((m0[b][bi] == bj) | (m0[b][bi] == -1)) and np.all((m1[b][bj] == bi) | (m1[b][bj] == -1))
    np.testing.assert_array_equal(got["matching_scores0"], (m0 > -1).astype(np.float32))
    np.testing.assert_array_equal(got["matching_scores1"], (m1 > -1).astype(np.float32))
    assert set(np.unique(got["reward"])) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("name", ["gt_exact_b3_m64_n48", "gt_rand_b2_m300_n257"])
def test_reward_false_omits_the_key_and_changes_nothing_else(name):
    full, _ = _run(name)
    lean, _ = _run(name, reward=False)
    assert list(lean) == [k for k in KEYS if k != "reward"]
    for k in lean:
        np.testing.assert_array_equal(lean[k].view(np.uint8), full[k].view(np.uint8), err_msg=k)


@pytest.mark.parametrize("name", ["gt_exact_b3_m64_n48", "gt_rand_b1_m37_n4100", "gt_rand_b1_m4100_n37"])
def test_two_runs_are_bit_identical(name):
    g, meta = gt_ref.load_fixture(name)
    first, _ = _run(name)
    again = _matcher(th_positive=meta["th_positive"], th_negative=meta["th_negative"])(_feed(g))
    for k in KEYS:
        np.testing.assert_array_equal(again[k].cpu().numpy().view(np.uint8), first[k].view(np.uint8), err_msg=k)


def test_single_homography_equals_the_tiled_one():
    g, meta = gt_ref.load_fixture("gt_rand_b2_m300_n257")
    feed = _feed(g)
    H = feed["H_0to1"][1].clone()
    tiled = _matcher()({**feed, "H_0to1": H[None].repeat(2, 1, 1)})
    single = _matcher()({**feed, "H_0to1": H})
    assert single["assignment"].any()
    for k in KEYS:
        assert torch.equal(single[k], tiled[k]), k
    # pair 1 under its own H is what the fixture run gave
    full, _ = _run("gt_rand_b2_m300_n257")
    np.testing.assert_array_equal(single["matches0"][1].cpu().numpy(), full["matches0"][1])


def test_one_point_per_image():
    m = _matcher(th_positive=3.0, th_negative=3.0)
    kp = torch.tensor([[[10.0, 20.0]]], device=DEV)
    near = m({"keypoints0": kp, "keypoints1": kp + 1.0, "H_0to1": torch.eye(3, device=DEV)})
    assert near["assignment"].shape == (1, 1, 1) and bool(near["assignment"][0, 0, 0])
    assert near["matches0"].tolist() == [[0]] and near["matches1"].tolist() == [[0]] and near["reward"].tolist() == [[[1.0]]]
    far = m({"keypoints0": kp, "keypoints1": kp + 50.0, "H_0to1": torch.eye(3, device=DEV)})
    assert not bool(far["assignment"].any()) and far["matches0"].tolist() == [[-1]] and far["reward"].tolist() == [[[-1.0]]]


@pytest.mark.parametrize("M,N", [(0, 5), (5, 0)])
def test_empty_side_returns_the_documented_dict(M, N):
    out = _matcher()({"keypoints0": torch.zeros(2, M, 2, device=DEV), "keypoints1": torch.zeros(2, N, 2, device=DEV),
                      "H_0to1": torch.eye(3, device=DEV)})
    assert list(out) == KEYS
    ref_a, ref_m0, ref_m1 = gt_ref.gt_matches_from_homography(torch.zeros(2, M, 2), torch.zeros(2, N, 2), torch.eye(3))
    assert out["assignment"].dtype == torch.bool and out["assignment"].shape == ref_a.shape and not out["assignment"].any()
    assert torch.equal(out["matches0"].cpu(), ref_m0) and torch.equal(out["matches1"].cpu(), ref_m1)
    assert out["reward"].shape == (2, M, N) and out["proj_0to1"].shape == (2, M, 2) and out["proj_1to0"].shape == (2, N, 2)
    assert not out["matching_scores0"].any() and not out["matching_scores1"].any()


def test_unaligned_pair_bases_and_views():
    """A reward / assignment whose second pair starts off a 16-byte boundary (odd M * N) and
    non-contiguous, non-fp32 inputs: equal to the contiguous fp32 run."""
    g, meta = gt_ref.load_fixture("gt_rand_b2_m300_n257")
    feed = _feed(g)
    sub = {"keypoints0": feed["keypoints0"][:, :299], "keypoints1": feed["keypoints1"][:, :255], "H_0to1": feed["H_0to1"]}
    a = _matcher()(sub)
    b = _matcher()({k: v.double() for k, v in sub.items()})  # fp32 values held as fp64: cast back exactly
    ref = gt_ref.gt_matches_from_homography(sub["keypoints0"].cpu(), sub["keypoints1"].cpu(), sub["H_0to1"].cpu(), 3.0, 3.0)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    # the full fixture has no undecidable item, and dropping points only widens gaps or leaves them
    mg = gt_ref.margins(sub["keypoints0"].cpu(), sub["keypoints1"].cpu(), sub["H_0to1"].cpu(), 3.0, 3.0, meta["tau"])
    ok_r, ok_c, ok_e = ~mg["und_rows"], ~mg["und_cols"], ~mg["und_reward"]
    np.testing.assert_array_equal(a["matches0"].cpu().numpy()[ok_r], ref["matches0"].numpy()[ok_r])
    np.testing.assert_array_equal(a["matches1"].cpu().numpy()[ok_c], ref["matches1"].numpy()[ok_c])
    np.testing.assert_array_equal(a["reward"].cpu().numpy()[ok_e], ref["reward"].numpy()[ok_e])


# ---------------------------------------------------------------------------------------------
# end to end: the pipeline's training step
def _e2e_data(B=2, M=128, seed=21):
    from lightglue_amd.sg_weights import synthetic_scores
    from lightglue_amd.weights import synthetic_pair

    rng = np.random.Generator(np.random.PCG64(seed))
    p = synthetic_pair(B=B, M=M, N=M, seed=seed, width=640, height=480)
    H = np.tile(np.eye(3), (B, 1, 1))
    H[:, :2, :2] += rng.standard_normal((B, 2, 2)) * 0.05
    H[:, :2, 2] = rng.uniform(-30.0, 30.0, (B, 2))
    H[:, 2, :2] = rng.standard_normal((B, 2)) * 1e-4
    kp0 = p["keypoints0"].astype(np.float64)
    kp1 = np.empty_like(kp0)
    for b in range(B):  # image 1: image 0 warped plus noise, shuffled -- positives exist
        ph = np.concatenate([kp0[b], np.ones((M, 1))], 1) @ H[b].T
        kp1[b] = (ph[:, :2] / ph[:, 2:] + rng.standard_normal((M, 2)))[rng.permutation(M)]
    kp1 = np.clip(kp1, 0.0, np.array([639.0, 479.0]))  # SuperGlue asserts the keypoints lie in the image
    data = {"keypoints0": p["keypoints0"], "keypoints1": kp1.astype(np.float32), "descriptors0": p["descriptors0"],
            "descriptors1": p["descriptors1"], "H_0to1": H.astype(np.float32),
            "keypoint_scores0": synthetic_scores(B, M, seed=seed + 1), "keypoint_scores1": synthetic_scores(B, M, seed=seed + 2)}
    feed = {k: torch.from_numpy(v).to(DEV) for k, v in data.items()}
    size = torch.tensor([[640.0, 480.0]] * B, device=DEV)
    view = {"image_size": size, "image": torch.zeros(B, 1, 480, 640, device=DEV)}
    feed.update({"view0": dict(view), "view1": dict(view)})
    return data, feed


def _matcher_conf(kind):
    if kind == "lightglue":
        return {"name": "matchers.lightglue", "n_layers": 3}
    return {"name": "gluefactory_nonfree.superglue", "GNN_layers": ["self", "cross"]}


@pytest.mark.parametrize("kind", ["lightglue", "superglue"])
def test_pipeline_loss_and_backward_equal_the_direct_call(kind):
    from lightglue_amd.pipeline import TwoViewPipeline
    from lightglue_amd.weights import synthetic_state_dict

    torch.manual_seed(0)
    pipe = TwoViewPipeline({"matcher": _matcher_conf(kind), "ground_truth": {"name": "matchers.homography_matcher"}}).to(DEV)
    if kind == "lightglue":
        sd = synthetic_state_dict({"n_layers": 3}, seed=4)
        pipe.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    pipe.train()
    data, feed = _e2e_data()

    def grads():
        out = {n: p.grad.clone() for n, p in pipe.named_parameters() if p.grad is not None}
        pipe.zero_grad(set_to_none=True)
        return out

    pred = pipe(feed)
    assert not any(k.startswith("gt_") for k in pred)
    losses, _ = pipe.loss(pred, feed)
    torch.mean(losses["total"]).backward()  # train.py:436,450
    g_pipe = grads()
    assert g_pipe and all(torch.isfinite(g).all() for g in g_pipe.values())
    assert any(bool(g.abs().max() > 0) for g in g_pipe.values())
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
    tau = gt_ref.tau_of(data["keypoints0"], data["keypoints1"], data["H_0to1"], 3.0, 3.0)
    mg = gt_ref.margins(data["keypoints0"], data["keypoints1"], data["H_0to1"], 3.0, 3.0, tau)
    ref = gt_ref.gt_matches_from_homography(*(torch.from_numpy(data[k]) for k in ("keypoints0", "keypoints1", "H_0to1")),
                                            pos_th=3.0, neg_th=3.0)
    ok_r, ok_c, ok_e = ~mg["und_rows"], ~mg["und_cols"], ~mg["und_reward"]
    assert ok_r.mean() > 0.9 and ok_c.mean() > 0.9
    np.testing.assert_array_equal(gt["gt_matches0"].cpu().numpy()[ok_r], ref["matches0"].numpy()[ok_r])
    np.testing.assert_array_equal(gt["gt_matches1"].cpu().numpy()[ok_c], ref["matches1"].numpy()[ok_c])
    ok_a = ok_r[:, :, None] & ok_c[:, None, :]
    np.testing.assert_array_equal(gt["gt_assignment"].cpu().numpy()[ok_a], ref["assignment"].numpy()[ok_a])
    np.testing.assert_array_equal(gt["gt_reward"].cpu().numpy()[ok_e], ref["reward"].numpy()[ok_e])
