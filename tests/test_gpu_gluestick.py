"""GlueStick on the GPU (lightglue_amd.GlueStick, include/gluestick_mi355x.h) -- needs an MI355X.

* golden parity: every fixture of tests/golden/gluestick (the REAL reference in fp64) within
  max(1e-4, 6 e), e the reference's own fp32-vs-fp64 deviation stored in the fixture; matches equal
  wherever the fixture's gap and threshold margins exceed 1e-4 (the rest counted and printed); loss
  values at rtol 1e-5;
* run-time cases against tests/gluestick_ref.py in fp64 (e from its own fp32 run): rows across the
  256-row padding and lines across 64, two line iterations, no lines in one / in both images;
* the three new kernels alone against fp64; repeatability (bit-identical forwards: the per-junction
  mean has a fixed order); weights follow an in-place change after reload_weights().
"""
import ctypes

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
from gluestick_golden_util import (BAND, FLOAT_KEYS, REF_ERR_FACTOR, case_names, compare_matches, decided, load_case,
                                   model_data, recipe_inputs, ref_data)
import gluestick_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-4  # the bar tests/test_gpu_superglue.py holds this arithmetic to
L4 = {"GNN_layers": ["self", "cross"] * 2}
COMMON = dict(noise=0.05, proj_gain=15.0, line_gain=0.5, image_wh=[640, 480], image_size=True, pad_junc=(0, 0))
RUNTIME = {
    # rows cross the 256-row padding (513 + 447), endpoints cross 64 and 256
    "big": dict(B=1, conf=L4, junc=(300, 257), pts=(213, 190), lines=(150, 129), seed=51, w_seed=8),
    "iters2": dict(B=2, conf={**L4, "num_line_iterations": 2}, junc=(24, 30), pts=(45, 61), lines=(21, 25), seed=52, w_seed=9),
    "no_lines0": dict(B=2, conf=L4, junc=(24, 30), pts=(45, 61), lines=(0, 25), seed=53, w_seed=10),
    "no_lines": dict(B=2, conf=L4, junc=(24, 30), pts=(45, 61), lines=(0, 0), seed=54, w_seed=11),
}


def _model(conf, sd):
    from lightglue_amd import GlueStick

    m = GlueStick(conf).eval().cuda()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m


def _forward(recipe, sd, pair):
    m = _model(recipe["conf"], sd)
    data = model_data(recipe, pair, "cuda")
    with torch.no_grad():
        pred = m(data, return_descriptors=True)
    torch.cuda.synchronize()
    return m, data, pred


def _check(pred, ref, e, th, label, lines=True, stored=None):
    """Float outputs within max(BAR, 6 e); matches equal where decided.  ref: numpy, fp64-derived;
    stored: a fixture's margins per head (default: computed from ref's log assignments)."""
    for k in FLOAT_KEYS:
        got = pred[k].cpu().numpy().astype(np.float64)
        assert got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
        err = float(np.abs(got - ref[k]).max()) if got.size else 0.0
        bar = max(BAR, REF_ERR_FACTOR * e[k])
        print(f"{label} {k}: max err {err:.3e}, bar {bar:.3e} (e {e[k]:.2e})")
        assert err <= bar, (label, k, err, bar)
    for head in ("", "line_") if lines else ("",):
        ok0, ok1 = decided(ref[head + "log_assignment"], th, BAND, stored[head] if stored else None)
        n0 = compare_matches(pred[head + "matches0"].cpu().numpy(), ref[head + "matches0"], ok0, label + " " + head + "matches0")
        n1 = compare_matches(pred[head + "matches1"].cpu().numpy(), ref[head + "matches1"], ok1, label + " " + head + "matches1")
        print(f"{label} {head}matches: {n0} rows / {n1} columns inside the {BAND} band (not compared), "
              f"{int((ref[head + 'matches0'] >= 0).sum())} matched")
    assert pred["matches0"].dtype == torch.int64 and pred["line_matches0"].dtype == torch.int64


# ------------------------------------------------------------------ golden parity
@pytest.fixture(scope="module", params=case_names())
def golden(request):
    z, meta = load_case(request.param)
    sd, pair = recipe_inputs(meta["recipe"])
    m, data, pred = _forward(meta["recipe"], sd, pair)
    return request.param, z, meta, m, data, pred


def test_golden_parity(golden):
    name, z, meta, _, _, pred = golden
    ref = {k: z["out_" + k].astype(np.float64) if z["out_" + k].dtype.kind == "f" else z["out_" + k]
           for k in list(FLOAT_KEYS) + ["matches0", "matches1", "line_matches0", "line_matches1"]}
    assert set(pred) == set(FLOAT_KEYS) | {"matches0", "matches1", "line_matches0", "line_matches1"}
    stored = {h: {k: z[f"margin_{h}{k}"] for k in ("row_gap", "col_gap", "row_th", "col_th")} for h in ("", "line_")}
    _check(pred, ref, meta["e"], meta["filter_threshold"], name, stored=stored)


def test_golden_loss(golden):
    name, z, meta, m, data, pred = golden
    losses, metrics = m.loss(pred, data)
    want = {k[5:] for k in z.files if k.startswith("loss_")}
    assert set(losses) == want and metrics == {}
    for k in sorted(want):
        got = losses[k].detach().cpu().numpy() if torch.is_tensor(losses[k]) else np.asarray(losses[k])
        print(f"{name} loss {k}: {np.ravel(got)} vs {np.ravel(z['loss_' + k])}")
        np.testing.assert_allclose(got, z["loss_" + k], rtol=1e-5, err_msg=k)


def test_repeatable(golden):
    """Two forwards on the same inputs are bit-identical in every output."""
    _, _, _, m, data, pred = golden
    with torch.no_grad():
        again = m(data, return_descriptors=True)
    for k in pred:
        assert torch.equal(pred[k], again[k]), k


# ------------------------------------------------------------------ run-time cases against the restatement
def _restated(recipe):
    sd, pair = recipe_inputs(recipe)
    data = ref_data(recipe, pair)
    with torch.no_grad():
        r64 = R.gluestick_forward(sd, data, recipe["conf"], torch.float64)
        r32 = R.gluestick_forward(sd, data, recipe["conf"], torch.float32)
    ref = {k: v.numpy() for k, v in r64.items() if torch.is_tensor(v)}
    e = {k: float((r32[k].double() - r64[k]).abs().max()) if r64[k].numel() else 0.0 for k in FLOAT_KEYS}
    return sd, pair, ref, e


@pytest.mark.parametrize("name", ["big", "iters2"])
def test_against_restatement(name):
    recipe = {**COMMON, **RUNTIME[name]}
    sd, pair, ref, e = _restated(recipe)
    _, _, pred = _forward(recipe, sd, pair)
    _check(pred, ref, e, 0.2, name)


@pytest.mark.parametrize("name", ["no_lines0", "no_lines"])
def test_without_lines(name):
    """No lines in image 0 (or in both): the line layers are skipped -- the reference skips them
    when either image has none -- the point outputs equal the restatement, the line outputs are the
    reference's zeros / -1."""
    recipe = {**COMMON, **RUNTIME[name]}
    sd, pair, ref, e = _restated(recipe)
    B, (L0, L1) = recipe["B"], recipe["lines"]
    _, _, pred = _forward(recipe, sd, pair)
    _check(pred, ref, e, 0.2, name, lines=False)
    for k, shape, fill in (("line_log_assignment", (B, L0, L1), 0), ("raw_line_scores", (B, L0, L1), 0),
                           ("line_matches0", (B, L0), -1), ("line_matches1", (B, L1), -1),
                           ("line_matching_scores0", (B, L0), 0), ("line_matching_scores1", (B, L1), 0)):
        assert tuple(pred[k].shape) == shape and bool((pred[k] == fill).all()), k
    # the same weights with the line iterations switched off give the same point outputs bit for bit
    off, _, pred_off = _forward({**recipe, "conf": {**recipe["conf"], "num_line_iterations": 0}}, sd, pair)
    assert torch.equal(pred["log_assignment"], pred_off["log_assignment"])


def test_bad_junction_index_raises():
    recipe = {**COMMON, **RUNTIME["iters2"]}
    sd, pair = recipe_inputs(recipe)
    m = _model(recipe["conf"], sd)
    data = model_data(recipe, pair, "cuda")
    for bad in (-1, pair["keypoints1"].shape[1]):
        d = dict(data)
        d["lines_junc_idx1"] = data["lines_junc_idx1"].clone()
        d["lines_junc_idx1"][1, 3, 0] = bad
        with pytest.raises(IndexError):
            m(d)


def test_weights_follow_reload():
    recipe = {**COMMON, **RUNTIME["iters2"]}
    sd, pair = recipe_inputs(recipe)
    m, data, before = _forward(recipe, sd, pair)
    with torch.no_grad():
        m.gnn.line_layers[0].mlp[3].weight.data.mul_(0.5)
        m.final_line_proj.bias.data.add_(0.25)
    m.reload_weights()
    with torch.no_grad():
        after = m(data, return_descriptors=True)
    sd2 = dict(sd)
    sd2["gnn.line_layers.0.mlp.3.weight"] = sd["gnn.line_layers.0.mlp.3.weight"] * np.float32(0.5)
    sd2["final_line_proj.bias"] = sd["final_line_proj.bias"] + np.float32(0.25)
    with torch.no_grad():
        r64 = R.gluestick_forward(sd2, ref_data(recipe, pair), recipe["conf"], torch.float64)
        r32 = R.gluestick_forward(sd2, ref_data(recipe, pair), recipe["conf"], torch.float32)
    ref = {k: v.numpy() for k, v in r64.items() if torch.is_tensor(v)}
    e = {k: float((r32[k].double() - r64[k]).abs().max()) for k in FLOAT_KEYS}
    _check(after, ref, e, 0.2, "reloaded")
    assert float((after["gnn_descriptors0"] - before["gnn_descriptors0"]).abs().max()) > 100 * BAR
    assert float((after["raw_line_scores"] - before["raw_line_scores"]).abs().max()) > 100 * BAR


# ------------------------------------------------------------------ the new kernels alone, float64
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _ulp32(x):
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def test_kernel_line_update():
    from lightglue_amd import _lib
    from lightglue_amd.gs_weights import gluestick_state_dict

    sd = gluestick_state_dict(L4, seed=12, line_gain=3.0)
    m = _model(L4, sd)
    lib = m._ensure_handle(torch.device("cuda", torch.cuda.current_device()))
    rng = np.random.Generator(np.random.PCG64(7))
    B, n, L = 2, 41, 37  # 74 endpoints per image: more than one wave's worth, odd line count
    X = (rng.standard_normal((B, n, 256)) * 0.5).astype(np.float32)
    enc = (rng.standard_normal((B, 2 * L, 256)) * 0.5).astype(np.float32)
    idx = rng.integers(1, n - 1, (B, 2 * L))  # junction n - 1: degree 0
    idx[:, 0:14:2] = 0                        # junction 0: degree 7, partners all different
    deg = np.bincount(idx[0], minlength=n)
    assert deg[0] == 7 and deg[n - 1] == 0 and deg.max() >= 7
    sd_t = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    for layer in (0, 1):
        p = f"gnn.line_layers.{layer}"
        r64 = R.line_update({k: v.double() for k, v in sd_t.items() if v.is_floating_point()}, p,
                            torch.from_numpy(X).double(), torch.from_numpy(enc).double(), torch.from_numpy(idx))
        r32 = R.line_update({k: v for k, v in sd_t.items() if v.is_floating_point()}, p, torch.from_numpy(X),
                            torch.from_numpy(enc), torch.from_numpy(idx))
        upd = float((r64 - torch.from_numpy(X).double()).abs().max())
        assert 0.3 * np.abs(X).max() <= upd <= 3 * np.abs(X).max(), upd  # an update of x's own magnitude
        e32 = float((r32.double() - r64).abs().max())
        Xd, encd, idxd = torch.from_numpy(X).cuda(), torch.from_numpy(enc).cuda(), torch.from_numpy(idx).cuda()
        out = torch.empty_like(Xd)
        _lib.check(lib.sg_gluestick_line_update(m._handle, layer, _p(Xd), _p(encd), _p(idxd), B, n, L, _p(out), _stream()),
                   "sg_gluestick_line_update")
        got = out.cpu().double()
        err = float((got - r64).abs().max())
        bar = max(BAR, REF_ERR_FACTOR * e32)
        print(f"line_update layer {layer}: update {upd:.3f}, max err {err:.3e}, bar {bar:.3e} (e32 {e32:.2e})")
        assert err <= bar
        assert torch.equal(out[:, n - 1].cpu(), torch.from_numpy(X)[:, n - 1])  # no endpoint: untouched, bit for bit
    assert lib.sg_gluestick_line_update(m._handle, 2, _p(Xd), _p(encd), _p(idxd), B, n, L, _p(out), _stream()) == _lib.LG_E_INVALID


@pytest.mark.parametrize("M,N", [(1, 1), (5, 300), (257, 64)])
def test_kernel_double_softmax(M, N):
    from lightglue_amd import _lib

    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(100 * M + N))
    B, bin_score = 2, 17.0
    s = ((rng.random((B, M, N)) * 2 - 1) * 16).astype(np.float32)  # spread to +-16, the bin above every score
    r64 = R.double_softmax(torch.from_numpy(s).double(), bin_score)
    r32 = R.double_softmax(torch.from_numpy(s), np.float32(bin_score))
    e32 = float((r32.double() - r64).abs().max())
    sd = torch.from_numpy(s).cuda()
    out = torch.full((B, M + 1, N + 1), float("nan"), device="cuda")
    _lib.check(lib.sg_gluestick_double_softmax(_p(sd), bin_score, B, M, N, _p(out), _stream()), "sg_gluestick_double_softmax")
    got = out.cpu().double()
    err = float((got - r64).abs().max())
    bar = max(REF_ERR_FACTOR * e32, 8 * _ulp32(float(r64.abs().max())))
    print(f"double_softmax {M}x{N}: max err {err:.3e}, bar {bar:.3e} (e32 {e32:.2e}, max |ref| {float(r64.abs().max()):.2f})")
    assert err <= bar
    assert bool((out[:, M, N] == 0).all())  # the corner entry is exactly 0


def test_kernel_line_scores():
    from lightglue_amd import _lib

    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(5))
    B, n0, n1, L0, L1 = 2, 30, 41, 9, 13
    md0 = rng.standard_normal((B, n0, 256)).astype(np.float32) * 2
    md1 = rng.standard_normal((B, n1, 256)).astype(np.float32) * 2
    idx0 = rng.integers(0, n0, (B, L0, 2))
    idx1 = rng.integers(0, n1, (B, L1, 2))
    # line 0 of image 1 is line 0 of image 0 with its endpoints swapped: the flipped orientation wins
    idx0[:, 0] = (2, 5)
    idx1[:, 0] = (0, 1)
    md1[:, 0], md1[:, 1] = md0[:, 5], md0[:, 2]
    t = [torch.from_numpy(a) for a in (md0, md1, idx0, idx1)]
    r64 = R.line_scores(t[0].double(), t[1].double(), t[2], t[3])
    r32 = R.line_scores(t[0], t[1], t[2], t[3])
    e0 = torch.gather(t[0].double(), 1, t[2].reshape(B, -1)[..., None].expand(-1, -1, 256))
    e1 = torch.gather(t[1].double(), 1, t[3].reshape(B, -1)[..., None].expand(-1, -1, 256))
    s = (e0 @ e1.transpose(1, 2) / 16).view(B, L0, 2, L1, 2)
    flipped = (s[:, :, 0, :, 1] + s[:, :, 1, :, 0]) > (s[:, :, 0, :, 0] + s[:, :, 1, :, 1])
    assert bool(flipped[:, 0, 0].all()) and 0 < int(flipped.sum()) < flipped.numel()
    e32 = float((r32.double() - r64).abs().max())
    d = [a.cuda() for a in t]
    out = torch.empty((B, L0, L1), device="cuda")
    _lib.check(lib.sg_gluestick_line_scores(_p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), B, n0, n1, L0, L1, _p(out), _stream()),
               "sg_gluestick_line_scores")
    err = float((out.cpu().double() - r64).abs().max())
    bar = max(REF_ERR_FACTOR * e32, 8 * _ulp32(float(r64.abs().max())))
    print(f"line_scores: max err {err:.3e}, bar {bar:.3e} (e32 {e32:.2e}, max |ref| {float(r64.abs().max()):.2f})")
    assert err <= bar
