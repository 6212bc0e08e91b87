"""`LightGlue({"mp": True})`: the eval forward with fp16 GEMMs and fp16 attention, against the CPU oracle
run with fp16 linears (mp_ref.py) -- needs an MI355X.

Model case: flash_ref.model_case's (B = 2, M = 300, N = 257, 9 layers, weights seed 1, pair seed 5).  F1 /
F2 are the oracle in the upstream (autocast) form and in the library's form.  d_s is their spread over the
matching scores, d_m over the decision margin (top-1 minus top-2 of F1's log-assignment row or column, at
F1's indices in both).  A row is left out of the match comparison when F1 != F2 on it, its F1 margin is
below 2 d_m, or its best non-dustbin score is within 2 d_s of the filter threshold; at most 10 % of the
rows may be left out (asserted on the CPU, test_mp_host.py: d_s = 1.5e-2, d_m = 0.17, F1 != F2 on 0 rows,
5.2 % left out).  On every other row G's matches equal F1's and its scores are within max(2 d_s, 1e-4).
Measured on an MI355X when the test was added (the oracles computed on that machine's CPU, whose fp32
summation order moves the spreads): d_s = 1.52e-2, d_m = 0.218, 6.3 % of the rows left out, G = F1 on every
row (the left-out ones included), max |score(G) - score(F1)| on the kept rows 1.78e-2 = 1.17 d_s (bar 2 d_s).
Ragged batch against each pair alone: scores 3.0e-8, log assignment 3.8e-6, dustbins 0.
"""
import ctypes

import numpy as np
import pytest
import torch

import flash_ref as fr
import lgamd  # noqa: F401
import mp_ref as mp
import ragged_util as ru
import test_gpu_flash_forward as tf
from golden_util import case_inputs, load
from test_gpu_flash_forward import build, cpu, feed, run

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAME = "fp16gemm+fp16attn"


@pytest.fixture(scope="module")
def model_run():
    sd, data, *_ = mp.model_case()
    model = build(dict(fr.MODEL_CONF, mp=True), sd)
    G = run(model, feed(data))
    used = model.last_precision_used
    plain = build(fr.MODEL_CONF, sd)
    P = run(plain, feed(data))
    return G, used, P, plain.last_precision_used


def test_mp_forward_matches_the_upstream_oracle(model_run):
    _, _, _, F1, F2 = mp.model_case()
    G = model_run[0]
    d_s, d_m = mp.spreads(F1, F2)
    x0, x1 = mp.excluded_masks(F1, F2, fr.MODEL_CONF["filter_threshold"])
    share = mp.excluded_share(x0, x1)
    assert share <= mp.EXCLUDED_CAP
    worst, flips = 0.0, 0
    for side, x in (("0", x0.numpy()), ("1", x1.numpy())):
        m, mref = cpu(G["matches" + side]), F1["matches" + side].numpy()
        s, sref = cpu(G["matching_scores" + side]), F1["matching_scores" + side].numpy()
        flips += int((m != mref).sum())
        worst = max(worst, float(np.abs(s - sref)[~x].max()))
    bar = max(2 * d_s, 1e-4)
    print(f"MP-FORWARD d_s {d_s:.3e}, d_m {d_m:.3e}, rows left out {share:.4f}, G != F1 on {flips} rows in all, "
          f"max |score(G) - score(F1)| on kept rows {worst:.3e} = {worst / d_s:.3f} d_s (bar {bar:.3e})")
    for side, x in (("0", x0.numpy()), ("1", x1.numpy())):
        np.testing.assert_array_equal(cpu(G["matches" + side])[~x], F1["matches" + side].numpy()[~x],
                                      err_msg=f"matches{side} on the kept rows")
    assert worst <= bar


def test_mp_really_acts_and_reports_its_flags(model_run):
    G, used, P, used_plain = model_run
    assert used == NAME and used_plain == "fp16x3"
    la, lp = cpu(G["log_assignment"]), cpu(P["log_assignment"])
    fin = np.isfinite(la) & np.isfinite(lp)
    assert np.abs(la[fin] - lp[fin]).max() > 1e-4


@pytest.mark.parametrize("precision", [0x400, 0x500])
def test_lg_create_accepts_the_flags(precision):
    from lightglue_amd import LightGlue, _lib

    lib = _lib.load()
    cfg = LightGlue({"mp": True})._lib_config()
    assert cfg.precision == 0x500
    cfg.precision = precision
    h = ctypes.c_void_p()
    _lib.check(lib.lg_create(ctypes.byref(cfg), 0, ctypes.byref(h)), "lg_create")
    assert h.value
    lib.lg_destroy(h)


def test_pipeline_returns_what_the_bare_model_returns(model_run):
    from lightglue_amd.pipeline import TwoViewPipeline

    sd, data, *_ = mp.model_case()
    pipe = TwoViewPipeline({"matcher": {"name": "matchers.lightglue", "mp": True, **fr.MODEL_CONF}}).eval().to(DEV)
    pipe.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    batch = {}
    for i in (0, 1):
        batch[f"view{i}"] = {
            "image_size": torch.from_numpy(data[f"image_size{i}"]).to(DEV),
            "scales": torch.ones(data[f"image_size{i}"].shape, device=DEV),
            "cache": {"keypoints": torch.from_numpy(data[f"keypoints{i}"]).to(DEV),
                      "descriptors": torch.from_numpy(data[f"descriptors{i}"]).to(DEV)},
        }
    pred = run(pipe, batch)
    assert pipe.matcher.last_precision_used == NAME
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "log_assignment"):
        assert cpu(pred[k]).tobytes() == cpu(model_run[0][k]).tobytes(), k


def test_ragged_batch_gives_each_pair_what_it_gives_alone():
    """The criterion of test_gpu_ragged.py (indices equal, scores 1e-4, log assignment 1e-3, dustbins 1e-4,
    padding -inf / -1 / 0), the reference being the same pair alone under `mp: true`; capacity 300, counts
    (300, 257), (130, 77), (64, 300)."""
    cap, counts = tf.CAP, tf.COUNTS
    assert cap == 300 and counts == ((300, 257), (130, 77), (64, 300))
    batch, pair_alone = tf.ragged_inputs()
    model = build(dict(ru.CONF, mp=True), ru.state_dict())
    pred = run(model, batch)
    assert model.last_precision_used == NAME
    la_all = cpu(pred["log_assignment"])
    assert la_all.shape == (len(counts), cap + 1, cap + 1)
    worst = {"score": 0.0, "la": 0.0, "dust": 0.0}
    for b, (n0, n1) in enumerate(counts):
        alone = run(model, feed(pair_alone(b)))
        rla = cpu(alone["log_assignment"])[0]
        for side, n in (("0", n0), ("1", n1)):
            m, s = cpu(pred["matches" + side])[b], cpu(pred["matching_scores" + side])[b]
            np.testing.assert_array_equal(m[:n], cpu(alone["matches" + side])[0], err_msg=f"pair {b} matches{side}")
            worst["score"] = max(worst["score"], float(np.abs(s[:n] - cpu(alone["matching_scores" + side])[0]).max()))
            assert (m[n:] == -1).all() and (s[n:] == 0).all()
        la = la_all[b]
        worst["la"] = max(worst["la"], float(np.abs(la[:n0, :n1] - rla[:-1, :-1]).max()))
        worst["dust"] = max(worst["dust"], float(np.abs(la[:n0, cap] - rla[:-1, -1]).max()),
                            float(np.abs(la[cap, :n1] - rla[-1, :-1]).max()))
        rest = np.ones_like(la, dtype=bool)
        rest[:n0, :n1] = False
        rest[:n0, cap] = False
        rest[cap, :n1] = False
        rest[cap, cap] = False
        assert np.isneginf(la[rest]).all() and np.isfinite(la[~rest]).all(), f"pair {b}: log-assignment layout"
    print(f"MP-RAGGED max |score diff| {worst['score']:.3e}, |la diff| {worst['la']:.3e}, |dustbin diff| {worst['dust']:.3e}")
    assert worst["score"] <= tf.SCORE_ATOL and worst["la"] <= tf.LA_ATOL and worst["dust"] <= tf.DUST_ATOL, worst


def test_pruning_and_early_stop_keep_the_output_contract():
    """B = 1, N = 512, width = depth = 0.95 on the pruning golden's inputs.  No index comparison: pruning
    decisions sit on thresholds that fp16 noise may cross."""
    conf, sd, data = case_inputs(load("prune_depth_width_n512")["meta"])
    assert conf["width_confidence"] == 0.95 and conf["depth_confidence"] == 0.95
    L = conf.get("n_layers", 9)
    model = build(dict(conf, mp=True), sd)
    a, b = run(model, feed(data)), run(model, feed(data))
    assert model.last_precision_used == NAME
    M, N = data["keypoints0"].shape[1], data["keypoints1"].shape[1]
    m0, m1 = cpu(a["matches0"])[0], cpu(a["matches1"])[0]
    assert m0.shape == (M,) and m1.shape == (N,)
    assert cpu(a["matching_scores0"]).shape == (1, M) and cpu(a["matching_scores1"]).shape == (1, N)
    assert ((m0 >= -1) & (m0 < N)).all() and ((m1 >= -1) & (m1 < M)).all() and (m0 > -1).sum() > 0
    i = np.nonzero(m0 > -1)[0]
    assert (m1[m0[i]] == i).all(), "matches0 / matches1 are mutually consistent"
    j = np.nonzero(m1 > -1)[0]
    assert (m0[m1[j]] == j).all()
    for k in ("matching_scores0", "matching_scores1"):
        s = cpu(a[k])
        assert np.isfinite(s).all() and (s >= 0).all() and (s <= 1).all()
    for k in ("prune0", "prune1"):
        p = cpu(a[k])
        assert (p >= 0).all() and (p <= L).all()
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1"):
        assert cpu(a[k]).tobytes() == cpu(b[k]).tobytes(), f"{k}: two runs differ"


def test_training_mode_ignores_mp():
    """The training path is fp32-class whatever `mp` says: forward and gradients of a small case (N = 128,
    2 layers) are bit-identical under mp true / false."""
    from lightglue_amd.weights import synthetic_pair, synthetic_state_dict

    conf = {"filter_threshold": 0.1, "n_layers": 2}
    sd = synthetic_state_dict(conf, seed=3)
    data = synthetic_pair(B=1, M=128, seed=4)
    out = []
    for flag in (False, True):
        model = build(dict(conf, mp=flag), sd, train=True)
        gd = feed(data, grad=True)
        pred = model(gd)
        loss = (pred["ref_descriptors0"] ** 2).sum() + (pred["ref_descriptors1"] ** 2).sum()
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: cpu(p.grad) for n, p in model.named_parameters() if p.grad is not None}
        grads["descriptors0"], grads["descriptors1"] = cpu(gd["descriptors0"].grad), cpu(gd["descriptors1"].grad)
        out.append((cpu(pred["ref_descriptors0"]), cpu(pred["ref_descriptors1"]), grads))
    (r0a, r1a, ga), (r0b, r1b, gb) = out
    assert r0a.tobytes() == r0b.tobytes() and r1a.tobytes() == r1b.tobytes()
    assert ga.keys() == gb.keys() and len(ga) > 10
    for n in ga:
        assert np.isfinite(ga[n]).all() and ga[n].tobytes() == gb[n].tobytes(), n
