"""The line ground truth on the device (lightglue_amd.line_gt, csrc/gt_lines.hip) against the fixtures the
reference produced (tests/golden/make_line_gt_golden.py) -- needs an MI355X.

Bars: stage A equal to the fixture on decided entries and inside the recorded bounds elsewhere, the exact
fixtures bit for bit; stage B on the fixture's own counts equal to the reference's labels with no gating;
the solver equal to SciPy's recorded assignation (and to the NumPy port of tests/line_gt_ref.py on the
shapes no fixture has); end to end bit for bit on the exact fixtures, on the random ones equal to the
reference for every pair without an undecidable entry and to stage B on the device's own counts otherwise;
the pipeline's loss from ground truth to value bit-identical to ``GlueStick.loss`` on the same tensors."""
import functools

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import line_gt_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAMES = R.fixture_names()
EXACT = [n for n in NAMES if R.load_fixture(n)[1]["exact"]]


def _lg():
    from lightglue_amd import line_gt

    return line_gt


def _dev(g, *keys):
    return [torch.from_numpy(g[k]).to(DEV) for k in keys]


def _np(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


@functools.lru_cache(maxsize=None)
def _stage_a(name):
    """One device run of stage A per fixture, shared by the tests below (read-only)."""
    g, meta = R.load_fixture(name)
    out = _lg().close_point_counts_from_homography(*_dev(g, "lines0", "lines1"), meta["shape"], meta["shape"],
                                                   *_dev(g, "H_0to1"), meta["npts"], meta["dist_th"], meta["min_visibility_th"])
    return out, dict(zip(("cnt0", "cnt1t", "out_of0", "out_of1"), _np(out)))


@functools.lru_cache(maxsize=None)
def _end_to_end(name):
    g, meta = R.load_fixture(name)
    out = _lg().gt_line_matches_from_homography(*_dev(g, "lines0", "lines1", "valid_lines0", "valid_lines1"), meta["shape"],
                                                meta["shape"], *_dev(g, "H_0to1"), meta["npts"], meta["dist_th"],
                                                meta["overlap_th"], meta["min_visibility_th"])
    return out, _np(out)


# ------------------------------------------------------------------ stage A
@pytest.mark.parametrize("name", NAMES)
def test_stage_a_counts(name):
    g, meta = R.load_fixture(name)
    dev, got = _stage_a(name)
    assert dev[0].dtype == dev[1].dtype == torch.uint8 and dev[2].dtype == dev[3].dtype == torch.bool
    B, n0, n1 = meta["B"], meta["n0"], meta["n1"]
    assert [tuple(t.shape) for t in dev] == [(B, n0, n1), (B, n0, n1), (B, n1), (B, n0)]
    for k, und in (("cnt0", "und0"), ("cnt1t", "und1t")):
        if not meta["exact"]:
            print(f"{name} {k}: {int((got[k] != g[k]).sum())} entries differ from the fp32 reference, "
                  f"{int((g[und] > 0).sum())} undecidable, {int((g[k] > 0).sum())} nonzero")
    R.check_counts(got, g, meta)


# ------------------------------------------------------------------ stage B
@pytest.mark.parametrize("name", NAMES)
def test_stage_b_labels_from_the_fixture_counts(name):
    g, meta = R.load_fixture(name)
    out = _lg().line_labels_from_counts(*_dev(g, "cnt0", "cnt1t", "out_of0", "out_of1", "valid_lines0", "valid_lines1"),
                                        meta["npts"], meta["overlap_th"])
    assert out[0].dtype == torch.bool and out[1].dtype == out[2].dtype == torch.int64
    R.check_labels(_np(out), g)


# ------------------------------------------------------------------ the solver
def _solve(cost):
    return np.stack(_np(_lg().linear_sum_assignment(cost)), axis=-2)  # [..., 2, k]


@pytest.mark.parametrize("name", NAMES)
def test_solver_on_the_recorded_cost_matrices(name):
    g, _ = R.load_fixture(name)
    got = _solve(torch.from_numpy(g["cost"]).to(DEV))
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, g["assignation"])


def _matrices():
    rng = np.random.Generator(np.random.PCG64(77))
    out = {}
    for shape in ((1, 1), (1, 5), (5, 1), (64, 64), (65, 63), (63, 65), (8, 2400), (2400, 8)):
        out[f"ties{shape}"] = rng.integers(-4, 1, shape).astype(np.float64) * 625.0
    out["random(65, 63)"] = rng.random((65, 63))
    out["equal(64, 64)"] = np.full((64, 64), 3.0)
    out["equal(70, 130)"] = np.zeros((70, 130))
    blocked = -(rng.integers(0, 3, (96, 130)) * rng.integers(0, 3, (96, 130)) * 625.0)
    blocked[rng.random(96) < 0.5] = 1e6
    blocked[:, rng.random(130) < 0.5] = 1e6
    out["blocked(96, 130)"] = blocked
    return out


MATRICES = _matrices()


@pytest.mark.parametrize("key", sorted(MATRICES))
def test_solver_on_small_tied_and_long_matrices(key):
    """1x1, 1x5, 5x1, 64x64, 65x63, an all-equal matrix, and 8x2400 / 2400x8, whose state does not fit the
    LDS (the global-memory route), against the NumPy port of SciPy's algorithm."""
    C = MATRICES[key]
    got = _solve(torch.from_numpy(C).to(DEV))
    np.testing.assert_array_equal(got, np.stack(R.lsap(C)))
    assert got.shape == (2, min(C.shape))


def test_solver_dtypes_batching_and_infeasible():
    rng = np.random.Generator(np.random.PCG64(78))
    C = rng.integers(-6, 3, (4, 37, 41))
    want = np.stack([np.stack(R.lsap(c)) for c in C])
    for dtype in (torch.float32, torch.int32, torch.float64):
        np.testing.assert_array_equal(_solve(torch.from_numpy(C).to(DEV).to(dtype)), want)
    # a pair alone against the same pair inside a batch
    np.testing.assert_array_equal(_solve(torch.from_numpy(C[2]).to(DEV).float()), want[2])
    # a non-contiguous view
    np.testing.assert_array_equal(_solve(torch.from_numpy(C).to(DEV).double().transpose(1, 2)),
                                  np.stack([np.stack(R.lsap(c.T)) for c in C]))
    # no finite assignment: -1 everywhere (SciPy raises), the other pair of the batch unaffected
    D = torch.from_numpy(C[:2]).to(DEV).double()
    D[0, 3] = float("inf")
    got = _solve(D)
    assert (got[0] == -1).all()
    np.testing.assert_array_equal(got[1], want[1])
    empty = _lg().linear_sum_assignment(torch.zeros(2, 0, 5, device=DEV))
    assert tuple(empty[0].shape) == (2, 0) and empty[0].dtype == torch.int64


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", NAMES)
def test_end_to_end(name):
    g, meta = R.load_fixture(name)
    dev, got = _end_to_end(name)
    assert dev[0].dtype == torch.bool and dev[1].dtype == dev[2].dtype == torch.int64
    if meta["exact"]:
        R.check_labels(got, g)
        return
    decided = R.pair_decided(g, meta)
    print(f"{name}: {int(decided.sum())} of {meta['B']} pairs without an undecidable entry")
    if decided.any():
        R.check_labels(got, g, pairs=decided)
    # every pair: the reference's stage B on the device's own counts
    _, a = _stage_a(name)
    want = R.stage_b(*(torch.from_numpy(a[k]) for k in ("cnt0", "cnt1t", "out_of0", "out_of1")),
                     torch.from_numpy(g["valid_lines0"]), torch.from_numpy(g["valid_lines1"]), meta["npts"], meta["overlap_th"])
    for x, w, k in zip(got, want[:3], ("positive", "m0", "m1")):
        np.testing.assert_array_equal(x, w.numpy(), err_msg=k)


@pytest.mark.parametrize("name", NAMES)
def test_structure_of_the_labels(name):
    g, _ = R.load_fixture(name)
    _, (pos, m0, m1) = _end_to_end(name)
    assert pos.sum(2).max() <= 1 and pos.sum(1).max() <= 1
    np.testing.assert_array_equal(m0 == -2, ~g["valid_lines0"])
    np.testing.assert_array_equal(m1 == -2, ~g["valid_lines1"])
    for b in range(pos.shape[0]):
        i = np.nonzero(m0[b] >= 0)[0]
        np.testing.assert_array_equal(m1[b][m0[b][i]], i)
        j = np.nonzero(m1[b] >= 0)[0]
        np.testing.assert_array_equal(m0[b][m1[b][j]], j)
        np.testing.assert_array_equal(np.argwhere(pos[b]), np.stack([i, m0[b][i]], 1))
    assert pos.any()


# ------------------------------------------------------------------ edges
def _call(l0, l1, v0, v1, H, shape=(120, 160), **kw):
    return _np(_lg().gt_line_matches_from_homography(l0, l1, v0, v1, shape, shape, H, **kw))


def _small(seed=3, B=2, n0=21, n1=18):
    rng = np.random.Generator(np.random.PCG64(seed))
    l0 = (rng.random((B, n0, 4)) * [160, 120, 160, 120]).astype(np.float32)
    l1 = np.concatenate([l0[:, :12] + rng.standard_normal((B, 12, 4)).astype(np.float32), l0[:, : n1 - 12] * 0.5], 1)
    H = np.tile(np.eye(3, dtype=np.float32), (B, 1, 1))
    t = [torch.from_numpy(x).to(DEV) for x in (l0, l1)]
    return t + [torch.ones(B, n0, dtype=torch.bool, device=DEV), torch.ones(B, n1, dtype=torch.bool, device=DEV),
                torch.from_numpy(H).to(DEV)]


def test_empty_sides_give_the_reference_tuple():
    l0, l1, v0, v1, H = _small()
    for a, b, va, vb in ((l0[:, :0], l1, v0[:, :0], v1), (l0, l1[:, :0], v0, v1[:, :0])):
        out = _lg().gt_line_matches_from_homography(a, b, va, vb, (120, 160), (120, 160), H)
        want = R.gt_line_matches_from_homography(a.cpu(), b.cpu(), va.cpu(), vb.cpu(), (120, 160), (120, 160), H.cpu())
        assert tuple(out[0].shape) == (2, a.shape[1], b.shape[1]) and out[0].dtype == torch.bool and not out[0].any()
        assert tuple(out[1].shape) == tuple(out[2].shape) == (2, 0) and out[1].dtype == torch.bool
        assert tuple(want[0].shape) == tuple(out[0].shape)


def test_degenerate_lines():
    l0, l1, v0, v1, H = _small()
    base = _call(l0, l1, v0, v1, H)
    assert base[0].any()
    want = R.gt_line_matches_from_homography(l0.cpu(), l1.cpu(), v0.cpu(), v1.cpu(), (120, 160), (120, 160), H.cpu())
    ca = R.stage_a(l0.cpu(), l1.cpu(), (120, 160), (120, 160), H.cpu())
    da = _np(_lg().close_point_counts_from_homography(l0, l1, (120, 160), (120, 160), H))
    if all(np.array_equal(d, c.numpy()) for d, c in zip(da, ca)):  # no near-tie flipped a count
        for x, w in zip(base, want):
            np.testing.assert_array_equal(x, w.numpy())
    # a zero-length line: NaNs in its direction, so nothing is close to it; its own samples may still
    # be close to a segment of the other image
    z0 = l0.clone()
    z0[:, 0, 2:] = z0[:, 0, :2]
    cnt0, cnt1t, _, _ = _np(_lg().close_point_counts_from_homography(z0, l1, (120, 160), (120, 160), H))
    assert (cnt0[:, 0] == 0).all()
    pos, m0, m1 = _call(z0, l1, v0, v1, H)
    assert (m0[:, 0] == -1).all() and not pos[:, 0].any()
    # all lines invalid
    pos, m0, m1 = _call(l0, l1, ~v0, ~v1, H)
    assert not pos.any() and (m0 == -2).all() and (m1 == -2).all()
    # lines wholly outside the image: clamped to a point on the border, unmatched
    far = l0 + 1000.0
    pos, m0, m1 = _call(far, l1, v0, v1, H)
    assert not pos.any() and (m0 == -1).all() and (m1 == -1).all()
    # a shift that takes every sample out of the other image
    Hs = H.clone()
    Hs[:, 0, 2] = 5000.0
    cnt = _lg().close_point_counts_from_homography(l0, l1, (120, 160), (120, 160), Hs)
    assert cnt[2].all() and cnt[3].all()
    pos, m0, m1 = _call(l0, l1, v0, v1, Hs)
    assert not pos.any() and (m0 == -1).all() and (m1 == -1).all()


def test_layouts_dtypes_and_repeatability():
    l0, l1, v0, v1, H = _small(seed=4)
    base = _call(l0, l1, v0, v1, H)
    again = _call(l0, l1, v0, v1, H)
    for x, y in zip(base, again):
        np.testing.assert_array_equal(x, y)
    variants = {
        "[B,n,2,2]": (l0.reshape(2, -1, 2, 2), l1.reshape(2, -1, 2, 2), H),
        "[B,n,k,2] first and last": (torch.stack([l0[..., :2], l0[..., :2] * 0 - 7, l0[..., 2:]], 2),
                                     torch.stack([l1[..., :2], l1[..., 2:] + 9, l1[..., :2] - 3, l1[..., 2:]], 2), H),
        "non-contiguous fp64": (torch.cat([l0, l0], -1).double()[..., :4],
                                l1.double().transpose(0, 1).contiguous().transpose(0, 1), H.double()),
        "a single [3,3] H": (l0, l1, H[0]),
    }
    assert not variants["non-contiguous fp64"][1].is_contiguous()
    for label, (a, b, h) in variants.items():
        for x, y in zip(base, _call(a, b, v0, v1, h)):
            np.testing.assert_array_equal(x, y, err_msg=label)


# ------------------------------------------------------------------ the pipeline
def test_pipeline_loss_from_line_ground_truth():
    from gluestick_golden_util import model_data
    from lightglue_amd.gs_weights import gluestick_state_dict, wireframe_pair
    from lightglue_amd.pipeline import TwoViewPipeline

    conf = {"GNN_layers": ["self", "cross"] * 2}
    recipe = {"B": 2, "image_wh": [640, 480], "image_size": True}
    pair = wireframe_pair(2, (40, 44), (88, 84), (40, 44), seed=61, noise=0.05, width=640, height=480)
    pipe = TwoViewPipeline({"matcher": {"name": "matchers.gluestick", **conf},
                            "ground_truth": {"name": "matchers.line_homography_matcher"}}).eval().cuda()
    sd = gluestick_state_dict(conf, seed=12, proj_gain=15.0, line_gain=0.5)
    pipe.matcher.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    data = {k: v for k, v in model_data(recipe, pair, "cuda").items() if not k.startswith("gt_")}
    B = 2
    assert data["keypoints0"].shape[1] == 128 and data["lines0"].shape[1:] == (40, 2, 2)
    data["H_0to1"] = torch.eye(3, device=DEV).repeat(B, 1, 1)  # view 1 is view 0 plus 2 px of noise
    data["valid_lines0"] = torch.ones(B, 40, dtype=torch.bool, device=DEV)
    data["valid_lines1"] = torch.ones(B, 44, dtype=torch.bool, device=DEV)
    data["valid_lines1"][:, 5] = False
    with torch.no_grad():
        pred = pipe(data)
        assert not any(k.startswith("gt_") for k in pred)
        losses, metrics = pipe.loss(pred, data)
    torch.cuda.synchronize()
    for k in ("gt_line_assignment", "gt_line_matches0", "gt_line_matches1", "gt_assignment", "gt_matches0", "gt_matches1"):
        assert k in pred, k
    assert pred["gt_line_assignment"].any() and pred["gt_line_assignment"].dtype == torch.bool
    assert (pred["gt_line_matches1"][:, 5] == -2).all()
    # most of the lines the generator shares between the views are found again
    shared = torch.from_numpy(pair["gt_line_assignment"]).to(DEV)
    assert int((pred["gt_line_assignment"] & shared).sum()) >= 0.5 * int(shared.sum())
    assert "line_assignment_nll" in losses and torch.isfinite(losses["line_assignment_nll"]).all()
    assert torch.isfinite(losses["total"]).all()
    direct, _ = pipe.matcher.loss(pred, {**pred, **data})
    assert set(direct) <= set(losses)
    for k, v in direct.items():
        assert torch.equal(torch.as_tensor(losses[k]), torch.as_tensor(v)), k
