"""`LightGlue({"flash": True})`: the eval forward with fp16 attention, against the CPU oracle run with
half-precision attention emulations (flash_ref.py) -- needs an MI355X.

Model case: B = 2, M = 300, N = 257, 9 layers, sharpened synthetic weights (seed 1), synthetic pair
seed 5.  F1 / F2 are the oracle with the upstream-form and the library-form emulation; their spread
(d_s over the matching scores, d_la over the finite log-assignment entries) measures how far two
members of the fp16-attention family lie apart on this input: d_s = 1.9e-3 to 2.1e-3 and d_la =
3.8e-2 to 3.9e-2 (the CPU's fp32 summation order moves them).  Rows on which F1 and F2 disagree or
whose top-1 / top-2 margin in F1 is below 4 d_la are near ties and are left out of the match
comparison: 2.1 % to 2.2 % of the rows for this seed (cap 5 %, asserted on the CPU in
test_flash_host.py).  Measured on an MI355X: matches equal on every other row, max |score(G) -
score(F1)| = 1.9e-3 = 1.01 d_s (bar 4 d_s).
"""
import numpy as np
import pytest
import torch

import flash_ref as fr
import lgamd  # noqa: F401
import ragged_util as ru
from golden_util import case_inputs, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SCORE_ATOL, LA_ATOL, DUST_ATOL = 1e-4, 1e-3, 1e-4  # the project's bars (test_gpu_ragged.py)


def build(conf, sd, train=False):
    from lightglue_amd import LightGlue

    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.train() if train else model.eval()


def feed(data, grad=False):
    gd = {k: torch.from_numpy(v).to(DEV) for k, v in data.items() if not k.startswith("image_size")}
    if grad:
        gd["descriptors0"].requires_grad_()
        gd["descriptors1"].requires_grad_()
    gd["view0"] = {"image_size": torch.from_numpy(data["image_size0"]).to(DEV)}
    gd["view1"] = {"image_size": torch.from_numpy(data["image_size1"]).to(DEV)}
    return gd


def run(model, gd):
    with torch.no_grad():
        pred = model(gd)
    torch.cuda.synchronize()
    return pred


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def model_run():
    sd, data, A, F1, F2 = fr.model_case()
    flash = build(dict(fr.MODEL_CONF, flash=True), sd)
    G = run(flash, feed(data))
    used = flash.last_precision_used
    plain = build(fr.MODEL_CONF, sd)
    P = run(plain, feed(data))
    return G, used, P, plain.last_precision_used


def test_flash_forward_matches_the_flash_oracle(model_run):
    _, _, _, F1, F2 = fr.model_case()
    G = model_run[0]
    d_s, d_la = fr.spreads(F1, F2)
    tie0, tie1 = fr.near_tie_masks(F1, F2)
    share = (tie0.sum().item() + tie1.sum().item()) / (tie0.numel() + tie1.numel())
    assert share <= fr.NEAR_TIE_CAP
    worst = 0.0
    for side, tie in (("0", tie0.numpy()), ("1", tie1.numpy())):
        m, mref = cpu(G["matches" + side]), F1["matches" + side].numpy()
        np.testing.assert_array_equal(m[~tie], mref[~tie], err_msg=f"matches{side} outside the near ties")
        agree = m == mref
        s, sref = cpu(G["matching_scores" + side]), F1["matching_scores" + side].numpy()
        worst = max(worst, float(np.abs(s - sref)[agree].max()))
    bar = max(4 * d_s, 1e-4)
    print(f"d_s {d_s:.3e}, d_la {d_la:.3e}, near-tie rows {share:.4f}, "
          f"max |score(G) - score(F1)| {worst:.3e} = {worst / d_s:.3f} d_s (bar {bar:.3e})")
    assert worst <= bar


def test_flash_really_acts(model_run):
    G, used, P, used_plain = model_run
    assert used == "fp16x3+fp16attn" and used_plain == "fp16x3"
    la, lp = cpu(G["log_assignment"]), cpu(P["log_assignment"])
    fin = np.isfinite(la) & np.isfinite(lp)
    assert np.abs(la[fin] - lp[fin]).max() > 1e-5


def test_lg_create_accepts_the_flag():
    import ctypes

    from lightglue_amd import LightGlue, _lib

    lib = _lib.load()
    cfg = LightGlue({"flash": True})._lib_config()
    assert cfg.precision == (_lib.PRECISIONS["auto"] | _lib.PREC_ATTN_F16)
    h = ctypes.c_void_p()
    _lib.check(lib.lg_create(ctypes.byref(cfg), 0, ctypes.byref(h)), "lg_create")
    assert h.value
    lib.lg_destroy(h)


def test_pipeline_returns_what_the_bare_model_returns(model_run):
    from lightglue_amd.pipeline import TwoViewPipeline

    sd, data, *_ = fr.model_case()
    pipe = TwoViewPipeline({"matcher": {"name": "matchers.lightglue", "flash": True, **fr.MODEL_CONF}}).eval().to(DEV)
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
    assert pipe.matcher.last_precision_used == "fp16x3+fp16attn"
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "log_assignment"):
        assert cpu(pred[k]).tobytes() == cpu(model_run[0][k]).tobytes(), k


# ---------------------------------------------------------------- ragged batches
# capacity, per-pair (n0, n1), seed: a case of this file's own on ragged_util's inputs and weights
CAP, COUNTS, RAGGED_SEED = 300, ((300, 257), (130, 77), (64, 300)), 11


def ragged_inputs():
    from test_gpu_hpatches_auc import homography_pairs

    data, _ = homography_pairs(len(COUNTS), CAP, seed=RAGGED_SEED)
    batch = {}
    for k in ru.POINT_KEYS:
        v = data[k].copy()
        for b, c in enumerate(COUNTS):
            v[b, c[int(k[-1])]:] = np.nan  # the padding never reaches a result
        batch[k] = torch.from_numpy(v).to(DEV)
    batch["view0"] = {"image_size": torch.from_numpy(data["image_size0"].copy()).to(DEV)}
    batch["view1"] = {"image_size": torch.from_numpy(data["image_size1"].copy()).to(DEV)}
    batch["num_keypoints0"] = torch.tensor([c[0] for c in COUNTS], dtype=torch.int64)
    batch["num_keypoints1"] = torch.tensor([c[1] for c in COUNTS], dtype=torch.int32, device=DEV)

    def alone(b):
        n = COUNTS[b]
        one = {k: data[k][b:b + 1, :n[int(k[-1])]].copy() for k in ru.POINT_KEYS}
        one["image_size0"], one["image_size1"] = data["image_size0"][b:b + 1].copy(), data["image_size1"][b:b + 1].copy()
        return one

    return batch, alone


def test_ragged_batch_gives_each_pair_what_it_gives_alone():
    """The criterion of test_gpu_ragged.py (indices equal, scores 1e-4, log assignment 1e-3, dustbins
    1e-4, padding -inf / -1 / 0), the reference being the same pair alone under `flash: true`."""
    cap, counts = CAP, COUNTS
    batch, pair_alone = ragged_inputs()
    model = build(dict(ru.CONF, flash=True), ru.state_dict())
    pred = run(model, batch)
    assert model.last_precision_used == "fp16x3+fp16attn"
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
    print(f"ragged flash: max |score diff| {worst['score']:.3e}, |la diff| {worst['la']:.3e}, |dustbin diff| {worst['dust']:.3e}")
    assert worst["score"] <= SCORE_ATOL and worst["la"] <= LA_ATOL and worst["dust"] <= DUST_ATOL, worst


# ---------------------------------------------------------------- pruning / early stop
def test_pruning_and_early_stop_keep_the_output_contract():
    """B = 1, N = 512, width = depth = 0.95 on the pruning golden's weights.  No index comparison:
    pruning decisions sit on thresholds that fp16 noise may cross."""
    conf, sd, data = case_inputs(load("prune_depth_width_n512")["meta"])
    assert conf["width_confidence"] == 0.95 and conf["depth_confidence"] == 0.95
    L = conf.get("n_layers", 9)
    model = build(dict(conf, flash=True), sd)
    a, b = run(model, feed(data)), run(model, feed(data))
    assert model.last_precision_used == "fp16x3+fp16attn"
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


# ---------------------------------------------------------------- training mode
def test_training_mode_ignores_flash():
    """The training path is fp32-class whatever `flash` says: forward and gradients of a small case
    (N = 128, 2 layers) are bit-identical under flash true / false."""
    from lightglue_amd.weights import synthetic_pair, synthetic_state_dict

    conf = {"filter_threshold": 0.1, "n_layers": 2}
    sd = synthetic_state_dict(conf, seed=3)
    data = synthetic_pair(B=1, M=128, seed=4)
    out = []
    for flash in (False, True):
        model = build(dict(conf, flash=flash), sd, train=True)
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
