"""Batched matching of pairs with different keypoint counts (data["num_keypoints0/1"],
lg_inputs_t.num_keypoints0/1).

The contract: pair b of a ragged batch gives what pair b gives alone at M = n0[b], N = n1[b].  The
reference of every case is the CPU oracle on each pair alone, sliced to its own counts
(ragged_util.oracle_pair).  Bars are the project's own (test_gpu_parity.py): match indices equal,
scores within 1e-4, log assignment within 1e-3 on the real block and 1e-4 on the dustbins.  No
near-tie exclusions: the oracle's smallest row / column top-1 / top-2 margin over all pairs is
3.5e-3, asserted below (and on the CPU in test_ragged_host.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ragged_util as ru

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SCORE_ATOL, LA_ATOL, DUST_ATOL = 1e-4, 1e-3, 1e-4
L = 9


@functools.lru_cache(maxsize=None)
def _model_cached(conf_items, sd_key):
    from lightglue_amd import LightGlue

    conf = dict(conf_items)
    sd = ru.state_dict() if sd_key == "crafted" else prune_state_dict()
    model = LightGlue(conf).eval().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def model_for(conf=None, sd_key="crafted"):
    return _model_cached(tuple(sorted((conf or ru.CONF).items())), sd_key)


def run(model, data):
    with torch.no_grad():
        pred = model(data)
    torch.cuda.synchronize()
    return pred


def cpu(t):
    return t.detach().cpu().numpy()


def check_against_oracle(name, pred):
    """Every pair of the ragged prediction against the oracle on that pair alone; the
    log-assignment layout and the padded-point outputs."""
    cap, counts, _ = ru.CASES[name]
    la_all = cpu(pred["log_assignment"])
    assert la_all.shape == (len(counts), cap + 1, cap + 1)
    worst = {"score": 0.0, "la": 0.0, "dust": 0.0}
    for b, (n0, n1) in enumerate(counts):
        ref = ru.oracle_pair(name, b)
        rla = ref["log_assignment"][0]
        # the issue's two facts about the fixture, from the oracle
        assert ru.top2_margin(rla[:-1, :-1]) >= 1e-3, (name, b)
        assert (ref["matches0"] > -1).sum() > 0, (name, b)
        for side, n in (("0", n0), ("1", n1)):
            m, s = cpu(pred["matches" + side])[b], cpu(pred["matching_scores" + side])[b]
            np.testing.assert_array_equal(m[:n], ref["matches" + side][0], err_msg=f"{name} pair {b} matches{side}")
            worst["score"] = max(worst["score"], float(np.abs(s[:n] - ref["matching_scores" + side][0]).max()))
            # padded points: matches -1, scores 0, prune 0; real points ran every layer
            assert (m[n:] == -1).all() and (s[n:] == 0).all()
            pr = cpu(pred["prune" + side])[b]
            assert (pr[:n] == L).all() and (pr[n:] == 0).all()
        la = la_all[b]
        worst["la"] = max(worst["la"], float(np.abs(la[:n0, :n1] - rla[:-1, :-1]).max()))
        worst["dust"] = max(worst["dust"], float(np.abs(la[:n0, cap] - rla[:-1, -1]).max()),
                            float(np.abs(la[cap, :n1] - rla[-1, :-1]).max()))
        assert la[cap, cap] == 0
        # everything else is -inf, so la[:, :-1, :-1].max(...) keeps its meaning
        rest = np.ones_like(la, dtype=bool)
        rest[:n0, :n1] = False
        rest[:n0, cap] = False
        rest[cap, :n1] = False
        rest[cap, cap] = False
        assert np.isneginf(la[rest]).all(), f"{name} pair {b}: padding of the log assignment"
        assert np.isfinite(la[~rest]).all()
    print(f"{name}: max |score diff| {worst['score']:.3e}, |la diff| {worst['la']:.3e}, |dustbin diff| {worst['dust']:.3e}")
    assert worst["score"] <= SCORE_ATOL and worst["la"] <= LA_ATOL and worst["dust"] <= DUST_ATOL, worst
    np.testing.assert_array_equal(cpu(pred["num_keypoints0"]), [c[0] for c in counts])
    np.testing.assert_array_equal(cpu(pred["num_keypoints1"]), [c[1] for c in counts])


# ---------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("precision", ["auto", "bf16x6"])
@pytest.mark.parametrize("name", ["b3", "b8"])
def test_ragged_batch_equals_the_oracle_pair_by_pair(name, precision):
    model = model_for(dict(ru.CONF, precision=precision))
    pred = run(model, ru.feed(name, DEV))
    assert model.last_precision_used == ("fp16x3" if precision == "auto" else "bf16x6")
    check_against_oracle(name, pred)


# ---------------------------------------------------------------- 2. poisoned padding
@pytest.mark.parametrize("with_size", [True, False], ids=["image_size", "kpt_extent"])
def test_padding_contents_never_reach_a_result(with_size):
    model = model_for()
    zero = run(model, ru.feed("b3", DEV, pad="zero", with_size=with_size))
    nan = run(model, ru.feed("b3", DEV, pad="nan", with_size=with_size))
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        a, b = cpu(zero[k]), cpu(nan[k])
        assert np.isfinite(a).all() and np.isfinite(b).all(), k
        assert a.tobytes() == b.tobytes(), f"{k} depends on the padding"
    # the extent fallback reduces over real points only: the pair alone gives the same matches
    for b, (n0, n1) in enumerate(ru.CASES["b3"][1]):
        ref = ru.oracle_pair("b3", b, with_size)
        np.testing.assert_array_equal(cpu(nan["matches0"])[b, :n0], ref["matches0"][0])
        np.testing.assert_allclose(cpu(nan["matching_scores0"])[b, :n0], ref["matching_scores0"][0], atol=SCORE_ATOL)


@pytest.mark.parametrize("precision", ["auto", "bf16x6"])
def test_padding_with_an_input_projection(precision):
    """input_dim != 256: the input range pass, the descriptor plane image and the projection GEMM
    cover real rows only.  128-d descriptors (the first half of the case's), zero against NaN
    padding, and pair 1 (oracle margin 7e-3, scores 3e-2 away from the threshold, checked on the
    CPU) against the oracle and against the same pair alone through the B = 1 path."""
    import oracle
    from lightglue_amd import LightGlue
    from test_gpu_hpatches_auc import crafted_state_dict

    conf = dict(ru.CONF, input_dim=128, precision=precision)
    sd = crafted_state_dict(conf)
    model = LightGlue(conf).eval().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)

    def narrow(d):
        return dict(d, descriptors0=d["descriptors0"][..., :128].contiguous(), descriptors1=d["descriptors1"][..., :128].contiguous())

    zero, nan = run(model, narrow(ru.feed("b3", DEV, pad="zero"))), run(model, narrow(ru.feed("b3", DEV, pad="nan")))
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        assert np.isfinite(cpu(nan[k])).all() and cpu(zero[k]).tobytes() == cpu(nan[k]).tobytes(), k
    n0, n1 = ru.CASES["b3"][1][1]
    one = ru.pair_data("b3", 1)
    alone = {k: torch.from_numpy(one[k]).to(DEV) for k in ru.POINT_KEYS}
    alone["view0"] = {"image_size": torch.from_numpy(one["image_size0"]).to(DEV)}
    alone["view1"] = {"image_size": torch.from_numpy(one["image_size1"]).to(DEV)}
    single = run(model, narrow(alone))
    one128 = dict(one, descriptors0=one["descriptors0"][..., :128].copy(), descriptors1=one["descriptors1"][..., :128].copy())
    with torch.no_grad():
        ref = oracle.lightglue_forward(sd, one128, conf)
    assert ru.top2_margin(ref["log_assignment"][0].numpy()[:-1, :-1]) >= 1e-3 and (ref["matches0"] > -1).sum() > 0
    for got in (cpu(nan["matches0"])[1, :n0], cpu(single["matches0"])[0]):
        np.testing.assert_array_equal(got, ref["matches0"][0].numpy())
    np.testing.assert_array_equal(cpu(nan["matches1"])[1, :n1], ref["matches1"][0].numpy())
    np.testing.assert_allclose(cpu(nan["matching_scores0"])[1, :n0], ref["matching_scores0"][0].numpy(), atol=SCORE_ATOL, rtol=0)


# ---------------------------------------------------------------- 3. capacity not a multiple of 16
def test_ragged_unfused_assignment_capacity_300():
    model = model_for()
    pred = run(model, ru.feed("odd", DEV))
    check_against_oracle("odd", pred)


# ---------------------------------------------------------------- 4. uniform equivalence
def test_full_counts_equal_no_counts():
    model = model_for()
    plain = ru.feed("b3", DEV, counts=False)
    full = dict(plain, num_keypoints0=torch.full((3,), 320), num_keypoints1=torch.full((3,), 320, dtype=torch.int16))
    for d in (plain, full):  # every slot full: the data is the unpadded case
        for k in ru.POINT_KEYS:
            d[k] = torch.from_numpy(ru.case_data("b3")[k].copy()).to(DEV)
    a, b = run(model, plain), run(model, full)
    assert "num_keypoints0" not in a
    for side in "01":
        np.testing.assert_array_equal(cpu(a["matches" + side]), cpu(b["matches" + side]))
        np.testing.assert_allclose(cpu(a["matching_scores" + side]), cpu(b["matching_scores" + side]), atol=SCORE_ATOL, rtol=0)
    np.testing.assert_allclose(cpu(a["log_assignment"]), cpu(b["log_assignment"]), atol=LA_ATOL, rtol=0)


# ---------------------------------------------------------------- 5. ragged and alone agree
def test_pair_of_a_ragged_batch_equals_the_pair_alone():
    model = model_for()
    pred = run(model, ru.feed("b3", DEV))
    n0, n1 = ru.CASES["b3"][1][1]
    one = ru.pair_data("b3", 1)
    alone = {k: torch.from_numpy(one[k].copy()).to(DEV) for k in ru.POINT_KEYS}
    alone["view0"] = {"image_size": torch.from_numpy(one["image_size0"]).to(DEV)}
    alone["view1"] = {"image_size": torch.from_numpy(one["image_size1"]).to(DEV)}
    single = run(model, alone)  # the existing B = 1 path, no counts
    np.testing.assert_array_equal(cpu(pred["matches0"])[1, :n0], cpu(single["matches0"])[0])
    np.testing.assert_array_equal(cpu(pred["matches1"])[1, :n1], cpu(single["matches1"])[0])


# ---------------------------------------------------------------- 6. pruning and early stop
PRUNE_CONF = {"filter_threshold": 0.0, "width_confidence": 0.95, "depth_confidence": 0.93}
TOKEN_BIAS = 2.0


@functools.lru_cache(maxsize=None)
def prune_state_dict():
    """The seeded random weights with golden_util.PRUNE_BIAS matchability biases (points really
    are pruned: 320 -> ~155 after layer 0) and a token-confidence bias that makes pairs stop."""
    from golden_util import PRUNE_BIAS
    from lightglue_amd.weights import synthetic_state_dict

    sd = synthetic_state_dict(PRUNE_CONF, seed=0)
    for i, v in enumerate(PRUNE_BIAS):
        sd[f"log_assignment.{i}.matchability.bias"][:] = v
        sd[f"token_confidence.{i}.token.0.bias"][:] = TOKEN_BIAS
    return sd


def test_ragged_with_pruning_and_early_stop_equals_the_oracle():
    """Pair 2 (17 + 300 points in slots of 320 + 320) is the pair whose stop decision depends on
    the divisor: found by printing, per layer, the oracle's count c of confident points and both
    ratios.  After layer 1 it has 1 - c / 317 = 0.880 (its own m + n: goes on, stops after layer 2
    at 0.968) but 1 - c / 640 = 0.941 (the capacities: would stop after layer 1) against
    depth_confidence 0.93.  Asserted from the oracle's layer descriptors below."""
    import oracle
    from oracle.lightglue_ref import _linear, _t, confidence_threshold

    sd = prune_state_dict()
    model = model_for(PRUNE_CONF, "prune")
    pred = run(model, ru.feed("b3", DEV, pad="nan"))
    cap, counts, _ = ru.CASES["b3"]
    differs = []
    for b, (n0, n1) in enumerate(counts):
        with torch.no_grad():
            ref = oracle.lightglue_forward(sd, ru.pair_data("b3", b), PRUNE_CONF, return_layers=True)
        stop = int(ref["stop_layer"])
        assert int(pred["stop_layer"][b]) == stop, (b, pred["stop_layer"], stop)
        for side, n in (("0", n0), ("1", n1)):
            np.testing.assert_array_equal(cpu(pred["matches" + side])[b, :n], ref["matches" + side][0].numpy())
            np.testing.assert_array_equal(cpu(pred["prune" + side])[b, :n], ref["prune" + side][0].numpy())
            assert (cpu(pred["matches" + side])[b, n:] == -1).all() and (cpu(pred["prune" + side])[b, n:] == 0).all()
            assert (cpu(pred["matching_scores" + side])[b, n:] == 0).all()
            np.testing.assert_allclose(cpu(pred["matching_scores" + side])[b, :n], ref["matching_scores" + side][0].numpy(),
                                       atol=SCORE_ATOL, rtol=0)
        assert (ref["matches0"] > -1).sum() > 0 and ref["prune0"].min() < stop + 1  # matched, and really pruned
        # would dividing by the capacities have stopped this pair at an earlier layer?
        for i, (d0, d1) in enumerate(ref["layers"][:stop]):
            tw = _t(sd[f"token_confidence.{i}.token.0.weight"], torch.float32)
            tb = _t(sd[f"token_confidence.{i}.token.0.bias"], torch.float32)
            tok = torch.cat([torch.sigmoid(_linear(d0, tw, tb)), torch.sigmoid(_linear(d1, tw, tb))], 1)
            c = float((tok < confidence_threshold(i, L)).sum())
            if 1.0 - c / (2 * cap) > PRUNE_CONF["depth_confidence"]:
                differs.append(b)
                break
    assert 2 in differs, "no pair of this case tells the two divisors apart"


# ---------------------------------------------------------------- 7. zero count
def test_pair_with_an_empty_image_has_no_matches_and_disturbs_nobody():
    model = model_for()
    data = ru.feed("b3", DEV, pad="nan")
    data["num_keypoints0"] = torch.tensor([320, 0, 17])
    for k in ("keypoints0", "descriptors0"):
        data[k][1] = float("nan")
    pred = run(model, data)
    for side in "01":
        assert (cpu(pred["matches" + side])[1] == -1).all()
        assert (cpu(pred["matching_scores" + side])[1] == 0).all()
        assert (cpu(pred["prune" + side])[1] == 0).all()
    # the other two pairs, run without it
    keep = [0, 2]
    two = {k: v[keep] for k, v in ru.feed("b3", DEV).items() if isinstance(v, torch.Tensor)}
    two["view0"] = {"image_size": data["view0"]["image_size"][keep]}
    two["view1"] = {"image_size": data["view1"]["image_size"][keep]}
    ref = run(model, two)
    for side in "01":
        np.testing.assert_array_equal(cpu(pred["matches" + side])[keep], cpu(ref["matches" + side]))
        np.testing.assert_allclose(cpu(pred["matching_scores" + side])[keep], cpu(ref["matching_scores" + side]),
                                   atol=SCORE_ATOL, rtol=0)


# ---------------------------------------------------------------- 8. graph path
def test_ragged_forward_replays_through_the_graph_mode():
    from lightglue_amd import LightGlue

    eager = run(model_for(), ru.feed("b3", DEV))
    model = LightGlue(ru.CONF).eval().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in ru.state_dict().items()}, strict=True)
    model.compile()
    run(model, ru.feed("b3", DEV, pad="nan"))  # captures
    full = ru.feed("b3", DEV, counts=False)
    run(model, full)  # another signature: no counts
    pred = run(model, ru.feed("b3", DEV))  # replays
    assert len(model._graphs) == 2
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "log_assignment", "prune0"):
        assert cpu(pred[k]).tobytes() == cpu(eager[k]).tobytes(), k


# ---------------------------------------------------------------- 9. SuperPoint ragged_keypoints
def _sp_case():
    from lightglue_amd.sp_weights import superpoint_state_dict, synthetic_images

    conf = {"max_num_keypoints": -1}  # the inputs of test_gpu_superpoint.py::test_superpoint_errors
    sd = superpoint_state_dict(conf, seed=9)
    image = torch.from_numpy(synthetic_images(2, 1, 64, 64, seed=109)).to(DEV)
    size = torch.tensor([[64.0, 64.0], [32.0, 32.0]], device=DEV)  # image 1: a quarter of the area
    return conf, sd, image, size


def test_superpoint_ragged_keypoints():
    from lightglue_amd import SuperPoint

    conf, sd, image, size = _sp_case()
    sp = SuperPoint(conf).eval().to(DEV)
    sp.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    with torch.no_grad():
        out = sp({"image": image, "image_size": size, "ragged_keypoints": True})
        ones = [sp({"image": image[b:b + 1], "image_size": size[b:b + 1]}) for b in range(2)]
    n = out["num_keypoints"]
    assert n.dtype == torch.int32 and n.device.type == "cuda" and n.shape == (2,)
    n = n.tolist()
    assert n[0] != n[1] and out["keypoints"].shape == (2, max(n), 2) and out["descriptors"].shape == (2, max(n), 256)
    # test_gpu_superpoint.py's bars: keypoints (integer pixels) identical, scores 2e-6, descriptors 2e-5
    atol = {"keypoints": 0.0, "keypoint_scores": 2e-6, "descriptors": 2e-5}
    for b in range(2):
        assert ones[b]["keypoints"].shape[1] == n[b]
        for k in ("keypoints", "keypoint_scores", "descriptors"):
            np.testing.assert_allclose(cpu(out[k][b, :n[b]]), cpu(ones[b][k][0]), atol=atol[k], rtol=0, err_msg=f"{b} {k}")
            assert (out[k][b, n[b]:] == 0).all(), (b, k)


def test_ragged_counts_reach_the_matcher_through_the_pipeline():
    from lightglue_amd.pipeline import TwoViewPipeline
    from lightglue_amd.weights import synthetic_state_dict

    _, sd, image, size = _sp_case()
    conf = {"extractor": {"name": "gluefactory_nonfree.superpoint", "max_num_keypoints": -1},
            "matcher": {"name": "matchers.lightglue", "filter_threshold": 0.1}}
    pipe = TwoViewPipeline(conf).eval().to(DEV)
    pipe.extractor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    pipe.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict({}, seed=0).items()})
    seen = {}
    hook = pipe.matcher.register_forward_pre_hook(lambda mod, args: seen.update(args[0]))
    view0 = {"image": image, "image_size": size, "ragged_keypoints": True}
    view1 = {"image": image.flip(0), "image_size": size.flip(0), "ragged_keypoints": True}
    with torch.no_grad():
        pred = pipe({"view0": view0, "view1": view1})
    hook.remove()
    n0, n1 = seen["num_keypoints0"].tolist(), seen["num_keypoints1"].tolist()
    assert n0 == n1[::-1] and n0[0] != n0[1]
    assert pred["num_keypoints0"].tolist() == n0 and pred["num_keypoints1"].tolist() == n1
    for b in range(2):
        assert (pred["matches0"][b, n0[b]:] == -1).all() and (pred["matches1"][b, n1[b]:] == -1).all()
        m = pred["matches0"][b, :n0[b]]
        assert (m < n1[b]).all()  # no real point is matched to padding


# ---------------------------------------------------------------- 10. C ABI
def test_lg_forward_with_counts_through_ctypes():
    from lightglue_amd import _lib

    model = model_for()
    data = ru.feed("b3", DEV, pad="nan")
    ref = run(model, data)
    cap, counts, _ = ru.CASES["b3"]
    B = len(counts)
    lib = model._ensure_handle(DEV)
    n0 = torch.tensor([c[0] for c in counts], dtype=torch.int32, device=DEV)
    n1 = torch.tensor([c[1] for c in counts], dtype=torch.int32, device=DEV)
    m0 = torch.empty((B, cap), dtype=torch.int64, device=DEV)
    m1 = torch.empty_like(m0)
    s0 = torch.empty((B, cap), dtype=torch.float32, device=DEV)
    s1 = torch.empty_like(s0)
    nbytes = ctypes.c_size_t()
    _lib.check(lib.lg_workspace_bytes(model._handle, B, cap, cap, ctypes.byref(nbytes)), "lg_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    inp = _lib.LGInputs(B, cap, cap, p(data["keypoints0"]), p(data["keypoints1"]), p(data["descriptors0"]),
                        p(data["descriptors1"]), p(data["view0"]["image_size"]), p(data["view1"]["image_size"]),
                        None, None, None, None, 0, p(n0), p(n1))
    out = _lib.LGOutputs(p(m0), p(m1), p(s0), p(s1))
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(lib.lg_forward(model._handle, ctypes.byref(inp), ctypes.byref(out), p(ws), nbytes.value,
                              ctypes.c_void_p(stream)), "lg_forward")
    torch.cuda.synchronize()
    assert out.precision_used == 0
    for got, key in ((m0, "matches0"), (m1, "matches1"), (s0, "matching_scores0"), (s1, "matching_scores1")):
        assert cpu(got).tobytes() == cpu(ref[key]).tobytes(), key
    # one of the two count pointers alone is a caller error
    inp.num_keypoints1 = None
    rc = lib.lg_forward(model._handle, ctypes.byref(inp), ctypes.byref(out), p(ws), nbytes.value, ctypes.c_void_p(stream))
    assert rc == -1, rc  # LG_E_INVALID
