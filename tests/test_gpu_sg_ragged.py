"""Ragged batches (per-pair keypoint counts) for SuperGlue and the Sinkhorn head on the GPU.

The yardstick is the CPU oracle run pair by pair at the pair's own sizes (tests/sg_ragged_ref.py), at
the bars the uniform tests hold for the same quantities: Sinkhorn Z atol 1e-4 / rtol 1e-5
(tests/test_gpu_parity.py), SuperGlue GNN descriptors, cost and matching scores 1e-4, the log
assignment on seeded random weights 2e-3, matches exact outside the 1e-4 near-tie band
(tests/test_gpu_superglue.py).  Padding is NaN throughout; padded outputs must be exactly
-1 / 0 / 0 / -inf.  The near-tie share of every seeded case is capped in test_sg_ragged_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import sg_ragged_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def cpu(t):
    return t.detach().cpu().numpy()


def counts_t(counts):
    n0 = torch.tensor([c[0] for c in counts], dtype=torch.int32, device=DEV)
    n1 = torch.tensor([c[1] for c in counts], dtype=torch.int64)  # any integer dtype, any device
    return n0, n1


def assert_frame(Z, want, atol, rtol=0.0, what="Z"):
    """The -inf pattern exactly, nothing else non-finite, the finite values within the bar."""
    Z, want = np.asarray(Z), np.asarray(want)
    hole = np.isneginf(want)
    np.testing.assert_array_equal(np.isneginf(Z), hole, err_msg=f"{what}: -inf pattern")
    assert np.isfinite(Z[~hole]).all(), what
    err = np.abs(Z[~hole] - want[~hole])
    print(what, "max err", float(err.max()) if err.size else 0.0)
    np.testing.assert_allclose(Z[~hole], want[~hole], atol=atol, rtol=rtol, err_msg=what)


# ---------------------------------------------------------------- 1. Sinkhorn alone
@pytest.mark.parametrize("name", sorted(ref.SK_CASES))
def test_sinkhorn_ragged_matches_per_pair_oracle(name):
    from lightglue_amd import log_optimal_transport

    (M, N), counts, iters, _ = ref.SK_CASES[name]
    scores = ref.nan_padded(ref.sk_scores(name), counts, {1: 0, 2: 1})
    n0, n1 = counts_t(counts)
    Z = cpu(log_optimal_transport(torch.from_numpy(scores).to(DEV), ref.SK_ALPHA, iters, n0, n1))
    assert_frame(Z, ref.sk_expected(name), atol=1e-4, rtol=1e-5, what=name)


def _underflow_case(planted):
    """tests/test_gpu_parity.py::test_sinkhorn_underflow_column_takes_exact_path at N = 72, pair 1
    padded to 72 from 60 columns (NaN)."""
    g = torch.Generator().manual_seed(11)
    scores = torch.randn((2, 50, 72), generator=g) * 2.0
    if planted:
        scores[:, :, 5] = -300.0  # a real column of both pairs
        scores[1, 7, :] = -250.0
    counts = ((50, 72), (50, 60))
    return ref.nan_padded(scores.numpy(), counts, {1: 0, 2: 1}), counts


@pytest.mark.parametrize("planted", [True, False])
def test_sinkhorn_ragged_underflow_flag(planted):
    """The underflow flag is the real columns' alone: the ragged call reruns the exact kernels exactly
    when one of its pairs, run alone at its own size through the uniform entry, does; the padded
    columns -- empty sums -- never raise it (without the planted column: no rerun at all)."""
    from lightglue_amd import _lib, log_optimal_transport

    lib = _lib.load()
    scores, counts = _underflow_case(planted)
    want = ref.sk_reference(np.nan_to_num(scores, nan=0.0), counts, 1.0, 20)
    assert np.isfinite(want[~np.isneginf(want)]).all()
    n0, n1 = counts_t(counts)
    before = lib.lg_sinkhorn_rerun_count()
    Z = cpu(log_optimal_transport(torch.from_numpy(scores).to(DEV), 1.0, 20, n0, n1))
    ragged_reruns = lib.lg_sinkhorn_rerun_count() - before
    alone = []
    for b, (m, n) in enumerate(counts):
        before = lib.lg_sinkhorn_rerun_count()
        log_optimal_transport(torch.from_numpy(scores[b:b + 1, :m, :n].copy()).to(DEV), 1.0, 20)
        alone.append(lib.lg_sinkhorn_rerun_count() - before)
    print("planted", planted, "reruns: ragged", ragged_reruns, "pairs alone", alone)
    assert ragged_reruns == (1 if any(alone) else 0)
    if not planted:
        assert ragged_reruns == 0
    assert_frame(Z, want, atol=1e-4, rtol=1e-5, what=f"planted={planted}")


@pytest.mark.parametrize("name", ["fused_odd", "four_wave"])
def test_sinkhorn_ragged_exact_kernels(name):
    """The rerun's kernels (running max per column), forced: ragged like the scaled ones."""
    from lightglue_amd import _lib, log_optimal_transport

    lib = _lib.load()
    (M, N), counts, iters, _ = ref.SK_CASES[name]
    scores = ref.nan_padded(ref.sk_scores(name), counts, {1: 0, 2: 1})
    prev = lib.lg_sinkhorn_force_exact(1)
    try:
        Z = cpu(log_optimal_transport(torch.from_numpy(scores).to(DEV), ref.SK_ALPHA, iters, *counts_t(counts)))
    finally:
        lib.lg_sinkhorn_force_exact(prev)
    assert_frame(Z, ref.sk_expected(name), atol=1e-4, rtol=1e-5, what=f"exact {name}")


def test_filter_matches_ragged_matches_per_pair_oracle():
    import oracle
    from lightglue_amd import filter_matches

    (M, N), counts, _, _ = ref.SK_CASES["fused_odd"]
    Z = ref.sk_expected("fused_odd")
    per = []
    for b, (n0, n1) in enumerate(counts):
        z = np.concatenate([np.concatenate([Z[b, :n0, :n1], Z[b, :n0, N:]], 1),
                            np.concatenate([Z[b, M:, :n1], Z[b, M:, N:]], 1)], 0)
        m0, m1, s0, s1 = oracle.filter_matches(torch.from_numpy(z[None].copy()), 0.01)
        per.append({"la": z, "m0": m0[0].numpy(), "m1": m1[0].numpy(), "s0": s0[0].numpy(), "s1": s1[0].numpy()})
    want = ref.to_capacity(per, M, N, counts)
    Zin = np.where(np.isneginf(Z), np.nan, Z)  # whatever lies outside the frame is never read
    got = filter_matches(torch.from_numpy(Zin).to(DEV), 0.01, *counts_t(counts))
    for g, k in zip(got, ("matches0", "matches1", "matching_scores0", "matching_scores1")):
        if k.startswith("matches"):
            np.testing.assert_array_equal(cpu(g), want[k], err_msg=k)
        else:
            np.testing.assert_allclose(cpu(g), want[k], atol=1e-6, rtol=0, err_msg=k)


# ---------------------------------------------------------------- 2. SuperGlue forward
@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            from lightglue_amd import SuperGlue

            sd, _ = ref.sg_inputs(name)
            m = SuperGlue(ref.SG_CASES[name]["conf"]).eval().to(DEV)
            full = m.state_dict()
            full.update({k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd.items()})
            m.load_state_dict(full, strict=True)
            cache[name] = m
        return cache[name]

    return get


def sg_feed(name, pad="nan", counts=True):
    _, data = ref.sg_inputs(name)
    cnt = ref.SG_CASES[name]["counts"]
    out = {}
    for k, v in data.items():
        if k == "image_size":
            continue
        v = ref.nan_padded(v, cnt, {1: int(k[-1])}) if pad == "nan" else v.copy()
        out[k] = torch.from_numpy(v).to(DEV)
    view = {"image_size": torch.from_numpy(data["image_size"].copy()).to(DEV)}
    out["view0"], out["view1"] = view, dict(view)
    if counts:
        out["num_keypoints0"], out["num_keypoints1"] = counts_t(cnt)
    return out


def run_sg(model, data):
    with torch.no_grad():
        out = model(data, return_descriptors=True)
    torch.cuda.synchronize()
    return {k: cpu(v) for k, v in out.items()}


@pytest.mark.parametrize("name", ["small", "full"])
def test_superglue_ragged_matches_per_pair_oracle(models, name):
    c = ref.SG_CASES[name]
    want = ref.sg_expected(name)
    out = run_sg(models(name), sg_feed(name, pad="nan"))
    for k, v in out.items():
        assert not np.isnan(v).any() and not np.isposinf(v).any(), k
    assert_frame(out["log_assignment"], want["log_assignment"], atol=2e-3, what="log_assignment")
    for k in ("gnn_descriptors0", "gnn_descriptors1", "sinkhorn_cost", "matching_scores0", "matching_scores1"):
        print(k, "max err", float(np.abs(out[k] - want[k]).max()))
        np.testing.assert_allclose(out[k], want[k], atol=1e-4, rtol=0, err_msg=k)
    r, col, share = ref.sg_decided(name)
    assert share <= ref.NEAR_TIE_CAP
    assert out["matches0"].dtype == np.int64
    np.testing.assert_array_equal(out["matches0"][r], want["matches0"][r])
    np.testing.assert_array_equal(out["matches1"][col], want["matches1"][col])
    for b, (n0, n1) in enumerate(c["counts"]):  # the padding, exactly
        assert (out["matches0"][b, n0:] == -1).all() and (out["matches1"][b, n1:] == -1).all()
        assert (out["matching_scores0"][b, n0:] == 0).all() and (out["matching_scores1"][b, n1:] == 0).all()
        assert (out["sinkhorn_cost"][b, n0:] == 0).all() and (out["sinkhorn_cost"][b, :, n1:] == 0).all()
        assert (out["gnn_descriptors0"][b, n0:] == 0).all() and (out["gnn_descriptors1"][b, n1:] == 0).all()
        if n0 == 0 or n1 == 0:  # the empty branch: nothing at all
            assert (out["matches0"][b] == -1).all() and (out["matches1"][b] == -1).all()
            assert (out["matching_scores0"][b] == 0).all() and (out["sinkhorn_cost"][b] == 0).all()


def test_empty_pair_does_not_disturb_the_others(models):
    """Pair 3 of the small case is empty, (50, 0): nothing of it runs, so pairs 0-2 give the same bits
    whatever its slot holds -- 50 real points and NaN padding, or NaN everywhere with counts (0, 0)."""
    m = models("small")
    a = run_sg(m, sg_feed("small"))
    d = sg_feed("small")
    for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "keypoint_scores0", "keypoint_scores1"):
        d[k][3] = float("nan")
    d["num_keypoints0"] = torch.tensor([96, 37, 1, 0], dtype=torch.int32, device=DEV)
    d["num_keypoints1"] = torch.tensor([80, 41, 5, -3], dtype=torch.int32, device=DEV)  # clamped on the device
    b = run_sg(m, d)
    for k, v in a.items():
        assert v.tobytes() == b[k].tobytes(), k
    assert np.isneginf(a["log_assignment"][3]).sum() == 97 * 81 - 1 and a["log_assignment"][3, 96, 80] == 0


def test_full_counts_equal_the_uniform_forward_bit_for_bit(models):
    m = models("small")
    c = ref.SG_CASES["small"]
    B = len(c["counts"])
    uniform = run_sg(m, sg_feed("small", pad="keep", counts=False))
    d = sg_feed("small", pad="keep", counts=False)
    d["num_keypoints0"] = torch.full((B,), c["M"], dtype=torch.int32, device=DEV)
    d["num_keypoints1"] = torch.full((B,), c["N"] + 5, dtype=torch.int64, device=DEV)  # clamped on the device
    ragged = run_sg(m, d)
    for k, v in uniform.items():
        assert v.tobytes() == ragged[k].tobytes(), k


def test_sg_forward_ragged_through_ctypes(models):
    """The C entry directly: NULL counts are sg_forward's bits; with counts, the Python path's."""
    from lightglue_amd import _lib

    m = models("small")
    c = ref.SG_CASES["small"]
    B, M, N = len(c["counts"]), c["M"], c["N"]
    lib = m._ensure_handle(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    nb = ctypes.c_size_t()
    _lib.check(lib.sg_workspace_bytes(m._handle, B, M, N, ctypes.byref(nb)), "sg_workspace_bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(d, n0, n1, ragged_entry):
        o = {"m0": torch.empty((B, M), dtype=torch.int64, device=DEV), "m1": torch.empty((B, N), dtype=torch.int64, device=DEV),
             "s0": torch.empty((B, M), device=DEV), "s1": torch.empty((B, N), device=DEV),
             "cost": torch.empty((B, M, N), device=DEV), "la": torch.empty((B, M + 1, N + 1), device=DEV)}
        inp = _lib.SGInputs(B, M, N, p(d["keypoints0"]), p(d["keypoints1"]), p(d["descriptors0"]), p(d["descriptors1"]),
                            p(d["keypoint_scores0"]), p(d["keypoint_scores1"]), p(d["view0"]["image_size"]),
                            p(d["view1"]["image_size"]), 0, 0, 0, 0)
        out = _lib.SGOutputs(p(o["m0"]), p(o["m1"]), p(o["s0"]), p(o["s1"]), p(o["cost"]), p(o["la"]), None, None)
        if ragged_entry:
            rc = lib.sg_forward_ragged(m._handle, ctypes.byref(inp), None if n0 is None else p(n0),
                                       None if n1 is None else p(n1), ctypes.byref(out), p(ws), nb.value, stream)
        else:
            rc = lib.sg_forward(m._handle, ctypes.byref(inp), ctypes.byref(out), p(ws), nb.value, stream)
        torch.cuda.synchronize()
        return rc, {k: cpu(v) for k, v in o.items()}

    clean = sg_feed("small", pad="keep", counts=False)
    rc0, a = call(clean, None, None, False)
    rc1, b = call(clean, None, None, True)
    assert rc0 == 0 and rc1 == 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    d = sg_feed("small", pad="nan")
    n0 = d["num_keypoints0"]
    n1 = d["num_keypoints1"].to(device=DEV, dtype=torch.int32)
    rc2, g = call(d, n0, n1, True)
    assert rc2 == 0
    py = run_sg(m, d)
    for k, pk in (("m0", "matches0"), ("m1", "matches1"), ("s0", "matching_scores0"), ("s1", "matching_scores1"),
                  ("cost", "sinkhorn_cost"), ("la", "log_assignment")):
        assert g[k].tobytes() == py[pk].tobytes(), k
    rc3, _ = call(d, n0, None, True)
    assert rc3 == _lib.LG_E_INVALID


# ---------------------------------------------------------------- 3. sinkhorn_match on a ragged LightGlue batch
def test_sinkhorn_match_on_a_ragged_lightglue_batch():
    from lightglue_amd import LightGlue
    from lightglue_amd.assignment import sinkhorn_match
    from test_gpu_hpatches_auc import crafted_state_dict, homography_pairs

    cap, counts = 128, ((128, 128), (100, 77), (33, 120))
    conf = {"filter_threshold": 0.1, "return_similarity": True}
    model = LightGlue(conf).eval().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in crafted_state_dict({"filter_threshold": 0.1}).items()})
    data, _ = homography_pairs(len(counts), cap, seed=13)

    def feed(sel, n0, n1, pad_counts=None):
        d = {}
        for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1"):
            v = data[k][sel, :(n0 if k[-1] == "0" else n1)].copy()
            if pad_counts is not None:
                v = ref.nan_padded(v, pad_counts, {1: int(k[-1])})
            d[k] = torch.from_numpy(v).to(DEV)
        d["view0"] = {"image_size": torch.from_numpy(data["image_size0"][sel].copy()).to(DEV)}
        d["view1"] = {"image_size": torch.from_numpy(data["image_size1"][sel].copy()).to(DEV)}
        return d

    with torch.no_grad():
        d = feed(slice(None), cap, cap, counts)
        d["num_keypoints0"], d["num_keypoints1"] = counts_t(counts)
        out, Z = sinkhorn_match(model, d)
        per = []
        for b, (n0, n1) in enumerate(counts):
            o, z = sinkhorn_match(model, feed(slice(b, b + 1), n0, n1))
            per.append({"la": cpu(z[0]), "m0": cpu(o["matches0"][0]), "m1": cpu(o["matches1"][0]),
                        "s0": cpu(o["matching_scores0"][0]), "s1": cpu(o["matching_scores1"][0])})
    want = ref.to_capacity(per, cap, cap, counts)
    assert_frame(cpu(Z), want["log_assignment"], atol=1e-4, rtol=1e-5, what="sinkhorn_match Z")
    np.testing.assert_allclose(cpu(out["matching_scores0"]), want["matching_scores0"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(cpu(out["matching_scores1"]), want["matching_scores1"], atol=1e-4, rtol=0)
    for b, (n0, n1) in enumerate(counts):
        r, c = ref.decided(per[b]["la"], 0.2)
        np.testing.assert_array_equal(cpu(out["matches0"])[b, :n0][r], per[b]["m0"][r])
        np.testing.assert_array_equal(cpu(out["matches1"])[b, :n1][c], per[b]["m1"][c])
        assert (cpu(out["matches0"])[b, n0:] == -1).all() and (cpu(out["matches1"])[b, n1:] == -1).all()


# ---------------------------------------------------------------- 4. SuperPoint -> SuperGlue through the pipeline
def test_pipeline_superpoint_to_superglue_ragged():
    from lightglue_amd.pipeline import TwoViewPipeline
    from lightglue_amd.sg_weights import superglue_state_dict
    from lightglue_amd.sp_weights import superpoint_state_dict, synthetic_images

    sg_conf = {"GNN_layers": ["self", "cross"] * 2, "num_sinkhorn_iterations": 20, "weights": None}
    conf = {"extractor": {"name": "gluefactory_nonfree.superpoint", "max_num_keypoints": -1},
            "matcher": {"name": "gluefactory_nonfree.superglue", **sg_conf}}
    pipe = TwoViewPipeline(conf).eval().to(DEV)
    sp_sd = superpoint_state_dict({"max_num_keypoints": -1}, seed=9)
    pipe.extractor.load_state_dict({k: torch.from_numpy(v) for k, v in sp_sd.items()}, strict=False)
    full = pipe.matcher.state_dict()
    full.update({k: torch.from_numpy(np.asarray(v).copy()) for k, v in superglue_state_dict(sg_conf, seed=4).items()})
    pipe.matcher.load_state_dict(full, strict=True)
    # two images of different texture: image 1 keeps a quarter of its area, so the counts differ
    image = torch.from_numpy(synthetic_images(2, 1, 64, 64, seed=109)).to(DEV)
    size = torch.tensor([[64.0, 64.0], [32.0, 32.0]], device=DEV)
    with torch.no_grad():
        pred = pipe({"view0": {"image": image, "image_size": size, "ragged_keypoints": True},
                     "view1": {"image": image.flip(0), "image_size": size.flip(0), "ragged_keypoints": True}})
        n0, n1 = pred["num_keypoints0"].tolist(), pred["num_keypoints1"].tolist()
        assert n0 == n1[::-1] and n0[0] != n0[1]
        for b in range(2):
            one = pipe({"view0": {"image": image[b:b + 1], "image_size": size[b:b + 1]},
                        "view1": {"image": image.flip(0)[b:b + 1], "image_size": size.flip(0)[b:b + 1]}})
            assert one["keypoints0"].shape[1] == n0[b] and one["keypoints1"].shape[1] == n1[b]
            la = cpu(one["log_assignment"][0])
            want = ref.to_capacity([{"la": la}], pred["keypoints0"].shape[1], pred["keypoints1"].shape[1], [(n0[b], n1[b])])
            assert_frame(cpu(pred["log_assignment"][b:b + 1]), want["log_assignment"], atol=1e-4, what=f"pipeline la {b}")
            np.testing.assert_allclose(cpu(pred["matching_scores0"][b, :n0[b]]), cpu(one["matching_scores0"][0]), atol=1e-4)
            r, c = ref.decided(la, 0.2)
            np.testing.assert_array_equal(cpu(pred["matches0"][b, :n0[b]])[r], cpu(one["matches0"][0])[r])
            np.testing.assert_array_equal(cpu(pred["matches1"][b, :n1[b]])[c], cpu(one["matches1"][0])[c])
            assert (pred["matches0"][b, n0[b]:] == -1).all() and (pred["matches1"][b, n1[b]:] == -1).all()
