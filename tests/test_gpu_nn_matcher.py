"""The nearest-neighbour matcher on the device (lightglue_amd.nn_matcher, csrc/nn_match.hip) through
``get_model``, against the fixtures the reference produced (tests/golden/make_nn_golden.py) -- needs
an MI355X.

Bars: ``matches0/1`` equal the reference on every item the fixture's fp64 margins decide
(tests/nn_ref.py); ``similarity`` within the fixture's ``tol = 4 max(e, 2.4e-7 S)`` of the fp64
similarity; ``log_assignment`` within the project's log-assignment bar (1e-3) of the
fp64 value, its border exactly 0; everything else exact (switches, ragged batches, ties, streams).
"""
import functools

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import nn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ["matches0", "matches1", "matching_scores0", "matching_scores1", "similarity", "log_assignment"]
DTYPES = [torch.int64, torch.int64, torch.float32, torch.float32, torch.float32, torch.float32]
LA_BAR = 1e-3
RAGGED = "nn_ragged_b3_m300_n257_d256"


def _net(**conf):
    from lightglue_amd.pipeline import get_model

    return get_model("matchers.nearest_neighbor_matcher")(conf)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return nn_ref.load_fixture(name)


@functools.lru_cache(maxsize=None)
def _fp64(name):
    """fp64 similarity and log assignment of a fixture, computed once on the CPU (read-only)."""
    g, _ = _fixture(name)
    return nn_ref.sim64(g["descriptors0"], g["descriptors1"]).numpy(), nn_ref.log_assignment64(
        g["descriptors0"], g["descriptors1"]).numpy()


def _feed(g, meta):
    data = {"descriptors0": torch.from_numpy(g["descriptors0"]).to(DEV), "descriptors1": torch.from_numpy(g["descriptors1"]).to(DEV)}
    if meta["counts"] is not None:
        data["num_keypoints0"] = torch.tensor(meta["counts"][0])
        data["num_keypoints1"] = torch.tensor(meta["counts"][1], device=DEV, dtype=torch.int32)
    return data


@functools.lru_cache(maxsize=None)
def _run(name, ratio=None, dist=None, mutual=True, similarity=True, log_assignment=True):
    """One device run per fixture and flavour, shared by the tests below (read-only)."""
    g, meta = _fixture(name)
    out = _net(ratio_thresh=ratio, distance_thresh=dist, mutual_check=mutual, similarity=similarity,
               log_assignment=log_assignment)(_feed(g, meta))
    return _np(out), [(k, v.dtype, tuple(v.shape), v.device.type) for k, v in out.items()]


@pytest.mark.parametrize("name", nn_ref.fixture_names())
def test_matcher_matches_reference_fixture(name):
    g, meta = _fixture(name)
    B, M, N = meta["B"], meta["M"], meta["N"]
    for ratio, dist, mutual in nn_ref.FLAVOURS:
        got, info = _run(name, ratio, dist, mutual)
        assert [k for k, *_ in info] == KEYS and [d for _, d, *_ in info] == DTYPES
        assert [s for *_, s, _ in info] == [(B, M), (B, N), (B, M), (B, N), (B, M, N), (B, M + 1, N + 1)]
        nn_ref.check_against_fixture(got, g, meta, ratio, dist, mutual)
        for k, size in (("matches0", N), ("matches1", M)):
            assert got[k].min() >= -1 and got[k].max() < size
        if mutual:  # whatever the undecidable items became, the result is mutual
            for b in range(B):
                i = np.nonzero(got["matches0"][b] >= 0)[0]
                assert np.array_equal(got["matches1"][b][got["matches0"][b][i]], i)
                j = np.nonzero(got["matches1"][b] >= 0)[0]
                assert np.array_equal(got["matches0"][b][got["matches1"][b][j]], j)


@pytest.mark.parametrize("name", nn_ref.fixture_names())
def test_similarity_and_log_assignment(name):
    """Measured on an MI355X (max |log_assignment - fp64| over the real blocks of all fixtures): see
    DESIGN.md §10i."""
    g, meta = _fixture(name)
    got, _ = _run(name)
    s64, la64 = _fp64(name)
    B, M, N = meta["B"], meta["M"], meta["N"]
    counts = meta["counts"] if meta["counts"] is not None else ([M] * B, [N] * B)
    sim, la = got["similarity"], got["log_assignment"]
    assert (la[:, M, :] == 0).all() and (la[:, :, N] == 0).all()  # the border, exactly
    worst_s = worst_la = 0.0
    for b in range(B):
        a, c = counts[0][b], counts[1][b]
        real = np.zeros((M, N), bool)
        real[:a, :c] = True
        assert (sim[b][~real] == 0).all()
        assert np.isneginf(la[b, :M, :N][~real]).all()
        worst_s = max(worst_s, float(np.abs(sim[b, :a, :c] - s64[b, :a, :c]).max()))
        if meta["counts"] is None:
            ref = la64[b, :a, :c]
        else:  # the pair alone: its softmaxes run over its own block
            ref = nn_ref.log_assignment64(g["descriptors0"][b:b + 1, :a], g["descriptors1"][b:b + 1, :c]).numpy()[0, :a, :c]
        worst_la = max(worst_la, float(np.abs(la[b, :a, :c] - ref).max()))
    print(f"{name}: max |sim - fp64| {worst_s:.3e} (tol {meta['tol']:.3e}), max |la - fp64| {worst_la:.3e}")
    assert worst_s <= meta["tol"]
    assert worst_la <= LA_BAR
    if meta["exact"]:  # exactly representable operands: the fp16x3 product is exact too
        assert np.array_equal(sim.view(np.uint32), g["similarity"].view(np.uint32))


@pytest.mark.parametrize("name", ["nn_b2_m300_n257_d256", "nn_b2_m130_n77_d100", RAGGED])
def test_dense_outputs_off_change_nothing_else(name):
    for ratio, dist, mutual in ((None, None, True), (0.8, 0.7, True)):
        full, _ = _run(name, ratio, dist, mutual)
        for s, l in ((False, True), (True, False), (False, False)):
            got, info = _run(name, ratio, dist, mutual, s, l)
            assert list(got) == [k for k in KEYS if (k != "similarity" or s) and (k != "log_assignment" or l)]
            for k in got:
                assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), (k, s, l)


@pytest.mark.parametrize("name", ["nn_b2_m513_n512_d256", RAGGED])
def test_two_runs_are_bit_identical(name):
    g, meta = _fixture(name)
    first, _ = _run(name, 0.8, 0.7, True)
    again = _np(_net(ratio_thresh=0.8, distance_thresh=0.7)(_feed(g, meta)))
    for k in KEYS:
        assert np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)), k


def test_ragged_equals_each_pair_alone():
    g, meta = _fixture(RAGGED)
    M, N = meta["M"], meta["N"]
    for ratio, dist, mutual in ((None, None, True), (None, 1.0, False), (0.8, 0.7, True), (0.95, None, False)):
        got, _ = _run(RAGGED, ratio, dist, mutual)
        for b, (a, c) in enumerate(zip(*meta["counts"])):
            for k, n in (("matches0", a), ("matches1", c)):  # the padded points: the stated fill values
                assert (got[k][b, n:] == -1).all() and (got[k.replace("matches", "matching_scores")][b, n:] == 0).all()
            if ratio and min(a, c) < 2:
                # one candidate on a side: that side scans nothing usable -> -1 (and under the mutual
                # check the other side with it); the reference cannot run this pair alone
                side = "matches1" if a < 2 else "matches0"
                assert (got[side][b] == -1).all()
                if mutual:
                    assert (got["matches0"][b] == -1).all() and (got["matches1"][b] == -1).all()
                continue
            alone = _np(_net(ratio_thresh=ratio, distance_thresh=dist, mutual_check=mutual)({
                "descriptors0": torch.from_numpy(g["descriptors0"][b:b + 1, :a]).to(DEV),
                "descriptors1": torch.from_numpy(g["descriptors1"][b:b + 1, :c]).to(DEV)}))
            assert np.array_equal(got["matches0"][b, :a], alone["matches0"][0])
            assert np.array_equal(got["matches1"][b, :c], alone["matches1"][0])
            assert np.array_equal(got["similarity"][b, :a, :c].view(np.uint32), alone["similarity"][0].view(np.uint32))
            assert np.array_equal(got["log_assignment"][b, :a, :c].view(np.uint32),
                                  alone["log_assignment"][0, :a, :c].view(np.uint32))
            assert (got["log_assignment"][b, M, :] == 0).all() and (got["log_assignment"][b, :, N] == 0).all()


def test_exact_ties_pick_the_lowest_index():
    """Duplicated rows 256 apart (different tiles) in both images: bit-identical similarities, the
    lower index wins on both sides, and the ratio test rejects the tie for r < 1."""
    M = N = 600
    rng = np.random.Generator(np.random.PCG64(41))
    d1 = rng.standard_normal((1, N, 64))
    d0 = rng.standard_normal((1, M, 64))
    J = np.arange(10, 40, 3)   # columns duplicated at J + 256
    I = np.arange(100, 130, 3)  # rows that look at them, duplicated at I + 256
    d1[0, J + 256] = d1[0, J]
    d0[0, I] = d1[0, J] + 0.05 * rng.standard_normal((len(J), 64))
    d0[0, I + 256] = d0[0, I]
    d0 /= np.linalg.norm(d0, axis=-1, keepdims=True)
    d1 /= np.linalg.norm(d1, axis=-1, keepdims=True)
    data = {"descriptors0": torch.from_numpy(d0.astype(np.float32)).to(DEV),
            "descriptors1": torch.from_numpy(d1.astype(np.float32)).to(DEV)}
    got = _np(_net(mutual_check=False)(data))
    sim = got["similarity"][0]
    assert np.array_equal(sim[:, J].view(np.uint32), sim[:, J + 256].view(np.uint32))
    assert np.array_equal(sim[I].view(np.uint32), sim[I + 256].view(np.uint32))
    assert np.array_equal(got["matches0"][0, I], J) and np.array_equal(got["matches0"][0, I + 256], J)
    assert np.array_equal(got["matches1"][0, J], I) and np.array_equal(got["matches1"][0, J + 256], I)
    # every row / column against the first maximum of the device's own similarity
    assert np.array_equal(got["matches0"][0], sim.argmax(1)) and np.array_equal(got["matches1"][0], sim.argmax(0))
    mut = _np(_net(mutual_check=True)(data))
    assert np.array_equal(mut["matches0"][0, I], J) and (mut["matches0"][0, I + 256] == -1).all()
    assert np.array_equal(mut["matches1"][0, J], I) and (mut["matches1"][0, J + 256] == -1).all()
    rat = _np(_net(ratio_thresh=0.99, mutual_check=False)(data))
    for k, idx in (("matches0", np.concatenate([I, I + 256])), ("matches1", np.concatenate([J, J + 256]))):
        assert (rat[k][0, idx] == -1).all() and (rat[k.replace("matches", "matching_scores")][0, idx] == 0).all()


def _tiny(M, N, D=8, seed=5):
    """Well separated: image-1 point j is image-0 point j % M plus noise that grows with j."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d0 = np.eye(M, D)[None] + 0.05 * rng.standard_normal((1, M, D))
    d1 = d0[:, np.arange(N) % M] + 0.02 * (1 + np.arange(N))[None, :, None] * rng.standard_normal((1, N, D))
    d0 /= np.linalg.norm(d0, axis=-1, keepdims=True)
    d1 /= np.linalg.norm(d1, axis=-1, keepdims=True)
    return torch.from_numpy(d0.astype(np.float32)), torch.from_numpy(d1.astype(np.float32))


@pytest.mark.parametrize("M,N,ratio", [(2, 2, 0.9), (1, 5, None), (5, 1, None), (1, 1, None), (3, 2, 0.99)])
def test_small_shapes(M, N, ratio):
    d0, d1 = _tiny(M, N)
    for mutual in (True, False):
        want = nn_ref.nn_forward(d0.double(), d1.double(), ratio, 1.0, mutual)
        got = _np(_net(ratio_thresh=ratio, distance_thresh=1.0, mutual_check=mutual)(
            {"descriptors0": d0.to(DEV), "descriptors1": d1.to(DEV)}))
        e, S, tol = nn_ref.tol_of(d0, d1)
        mg = nn_ref.margins(d0, d1, ratio, 1.0, mutual, tol)
        assert not mg["und_rows"].any() and not mg["und_cols"].any()  # the construction
        for k in ("matches0", "matches1"):
            assert np.array_equal(got[k], want[k].numpy()), k
        assert np.abs(got["similarity"] - want["similarity"].numpy()).max() <= tol
        assert np.abs(got["log_assignment"] - want["log_assignment"].numpy()).max() <= LA_BAR


@pytest.mark.parametrize("D", [1, 7, 33, 512])
def test_descriptor_widths(D):
    """The ends of the supported range, a width that is no multiple of 4 (scalar reads into the
    zero-padded copy) and one just past a k-block; for D = 32-multiples also a view that starts 4 bytes
    into its buffer."""
    B, M, N = 2, 70, 45
    rng = np.random.Generator(np.random.PCG64(50 + D))
    d = [rng.standard_normal((B, n, D)) for n in (M, N)]
    d[1][:, :30] = d[0][:, 5:35] + 0.3 * rng.standard_normal((B, 30, D))
    d = [torch.from_numpy((x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)) for x in d]
    e, S, tol = nn_ref.tol_of(d[0], d[1])
    mg = nn_ref.margins(d[0], d[1], None, 1.0, True, tol)
    want = nn_ref.nn_forward(d[0].double(), d[1].double(), None, 1.0, True)
    feeds = [[x.to(DEV) for x in d]]
    if D % 32 == 0:
        flat = [torch.zeros(x.numel() + 1, device=DEV) for x in d]
        for f, x in zip(flat, d):
            f[1:] = x.flatten().to(DEV)
        feeds.append([f[1:].view(x.shape) for f, x in zip(flat, d)])
        assert all(v.data_ptr() % 16 == 4 for v in feeds[1])
    for d0, d1 in feeds:
        got = _np(_net(distance_thresh=1.0)({"descriptors0": d0, "descriptors1": d1}))
        assert np.abs(got["similarity"] - want["similarity"].numpy()).max() <= tol
        assert np.abs(got["log_assignment"] - want["log_assignment"].numpy()).max() <= LA_BAR
        for k, und in (("matches0", mg["und_rows"]), ("matches1", mg["und_cols"])):
            assert np.array_equal(got[k][~und], want[k].numpy()[~und]), k
    if D > 1:  # D = 1: every similarity is +-1, all ties
        assert mg["und_rows"].mean() < 0.03 and (want["matches0"] > -1).any()


def test_empty_sides_and_the_single_candidate_ratio_error():
    for M, N in ((0, 7), (7, 0), (0, 0)):
        out = _net(ratio_thresh=0.8)({"descriptors0": torch.zeros(2, M, 16, device=DEV),
                                      "descriptors1": torch.zeros(2, N, 16, device=DEV)})
        assert list(out) == KEYS and [v.dtype for v in out.values()] == DTYPES
        assert [tuple(v.shape) for v in out.values()] == [(2, M), (2, N), (2, M), (2, N), (2, M, N), (2, M + 1, N + 1)]
        assert (out["matches0"] == -1).all() and (out["matches1"] == -1).all()
        assert (out["matching_scores0"] == 0).all() and (out["matching_scores1"] == 0).all()
        assert (out["log_assignment"] == 0).all()
        assert all(v.device.type == "cuda" for v in out.values())
    for M, N in ((1, 5), (5, 1)):
        d0, d1 = _tiny(M, N)
        with pytest.raises(ValueError, match="ratio_thresh"):
            _net(ratio_thresh=0.8)({"descriptors0": d0.to(DEV), "descriptors1": d1.to(DEV)})


def test_range_scaling_of_unnormalised_descriptors():
    """Descriptors x 64 leave the fp16x3 operand range and are scaled by a power of two on the
    device: the same matches with the thresholds off, the similarity (x 4096) within tol x 4096."""
    name = "nn_b2_m300_n257_d256"
    g, meta = _fixture(name)
    s64, _ = _fp64(name)
    got = _np(_net(mutual_check=False)({"descriptors0": torch.from_numpy(g["descriptors0"] * 64).to(DEV),
                                        "descriptors1": torch.from_numpy(g["descriptors1"] * 64).to(DEV)}))
    nn_ref.check_against_fixture(got, g, meta, None, None, False)
    assert np.abs(got["similarity"] - 4096.0 * s64).max() <= meta["tol"] * 4096


def test_non_default_stream_and_device_context():
    name = "nn_b2_m130_n77_d100"
    g, meta = _fixture(name)
    base, _ = _run(name, 0.8, 0.7, True)
    data = _feed(g, meta)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        out = _net(ratio_thresh=0.8, distance_thresh=0.7)(data)
    s.synchronize()
    with torch.cuda.device(DEV):
        out2 = _net(ratio_thresh=0.8, distance_thresh=0.7)(data)
    for o in (_np(out), _np(out2)):
        for k in KEYS:
            assert np.array_equal(o[k].view(np.uint8), base[k].view(np.uint8)), k


def _pipeline_data(name="nn_b2_m130_n77_d100"):
    g, meta = _fixture(name)
    rng = np.random.Generator(np.random.PCG64(9))
    B, M, N = meta["B"], meta["M"], meta["N"]
    kp = [torch.from_numpy((rng.random((B, n, 2)) * [640.0, 480.0]).astype(np.float32)).to(DEV) for n in (M, N)]
    d = [torch.from_numpy(g[k]).to(DEV) for k in ("descriptors0", "descriptors1")]
    return {"view0": {"cache": {"keypoints": kp[0], "descriptors": d[0]}},
            "view1": {"cache": {"keypoints": kp[1], "descriptors": d[1]}},
            "H_0to1": torch.eye(3, device=DEV).repeat(B, 1, 1)}, name


def test_pipeline_forward_returns_the_six_keys():
    from lightglue_amd.pipeline import TwoViewPipeline

    data, name = _pipeline_data()
    pipe = TwoViewPipeline({"extractor": {"name": None}, "allow_no_extract": True,
                            "matcher": {"name": "matchers.nearest_neighbor_matcher", "ratio_thresh": 0.8, "distance_thresh": 0.7}})
    pred = pipe(data)
    assert set(KEYS) <= set(pred) and {"descriptors0", "descriptors1", "keypoints0", "keypoints1"} <= set(pred)
    base, _ = _run(name, 0.8, 0.7, True)
    got = _np({k: pred[k] for k in KEYS})
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint8), base[k].view(np.uint8)), k


def test_pipeline_loss_skips_the_matcher():
    from lightglue_amd.pipeline import TwoViewPipeline

    data, _ = _pipeline_data()
    pipe = TwoViewPipeline({"extractor": {"name": None}, "allow_no_extract": True,
                            "matcher": {"name": "matchers.nearest_neighbor_matcher"},
                            "ground_truth": {"name": "matchers.homography_matcher"}})
    pred = pipe(data)
    losses, metrics = pipe.loss(pred, data)
    assert losses["total"] == 0 and metrics == {}
    assert "gt_matches0" in pred and pred["gt_matches0"].shape == pred["matches0"].shape
