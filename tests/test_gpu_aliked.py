"""ALIKED on the GPU (lightglue_amd.ALIKED -> sp_aliked_* of liblightglue_mi355x.so) against the
reference's own outputs (tests/golden/aliked/*.npz, tests/golden/make_aliked_golden.py), against the
CPU restatement in fp64 (tests/aliked_ref.py, held to the same fixtures by
tests/test_aliked_golden.py) on further seeded cases, and the deformable convolution alone against
float64.

Bars (tests/aliked_golden_util.py): scores max(2e-6, 6 e_scores), descriptors max(2e-5, 6 e_desc),
keypoints and dispersity max(6 e, (4 radius / T) score bar), where e_* is the reference's own
fp32-vs-fp64 error of the case (stored in the fixture; the restatement's fp32-vs-fp64 error for
the seeded cases).  The keypoint SET is asserted identical (every case has its selection gaps
above 4x the score bar, asserted from the reference side); inside the sorted order only keypoints
whose NMS scores differ by less than the score bar may trade places.  Each test prints its measured
maxima before it asserts (DESIGN.md §9c records them).
"""
import ctypes

import numpy as np
import pytest
import torch

import aliked_ref
from aliked_golden_util import aliked_bars, aliked_case_inputs, aliked_case_names, aliked_load, compare, fixture_bars
from lightglue_amd import _lib
from lightglue_amd.aliked_weights import aliked_state_dict
from lightglue_amd.sp_weights import synthetic_images

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OUT_KEYS = ("keypoints", "descriptors", "keypoint_scores", "score_dispersity", "score_map")


def as_torch_sd(sd):
    return {k: torch.from_numpy(v.copy()) if v.ndim else torch.tensor(int(v)) for k, v in sd.items()}


def make_model(conf, sd):
    from lightglue_amd import ALIKED

    m = ALIKED(conf).eval().to(DEV)
    m.load_state_dict(as_torch_sd(sd), strict=True)
    return m


def run(m, data, **extra):
    d = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in data.items()}
    d.update(extra)
    with torch.no_grad():
        out = m(d)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def as_np(out):
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else [t.numpy() for t in v]) for k, v in out.items() if k in OUT_KEYS}


@pytest.mark.parametrize("name", aliked_case_names())
def test_aliked_matches_reference_golden(name):
    g = aliked_load(name)
    conf, sd, data = aliked_case_inputs(g["meta"])
    out = run(make_model(conf, sd), data)
    ref = {k[4:]: v for k, v in g.items() if k.startswith("out_")}
    assert set(OUT_KEYS) <= set(out)
    compare(as_np(out), ref, fixture_bars(g["meta"]), name)


_REF_CACHE = {}


def reference_with_margins(key, sd, data, conf):
    """The restatement in fp64 (the reference of the seeded cases), the bars from its own
    fp32-vs-fp64 error, and the decidability of the case asserted from the reference side."""
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    r64 = aliked_ref.aliked_forward(sd, data, conf, torch.float64)
    r32 = aliked_ref.aliked_forward(sd, data, conf, torch.float32)
    e = {"scores": float((r32["score_map"].double() - r64["score_map"]).abs().max()), "kpts": 0.0, "desc": 0.0, "disp": 0.0}
    for b in range(len(r64["indices"])):
        assert torch.equal(r32["indices"][b], r64["indices"][b]), "the case is undecidable: fp32 and fp64 selections differ"
        e["kpts"] = max(e["kpts"], float((r32["keypoints"][b].double() - r64["keypoints"][b]).abs().max()))
        e["desc"] = max(e["desc"], float((r32["descriptors"][b].double() - r64["descriptors"][b]).abs().max()))
        e["disp"] = max(e["disp"], float((r32["keypoint_scores"][b].double() - r64["keypoint_scores"][b]).abs().max()))
        e["scores"] = max(e["scores"], float((r32["score_dispersity"][b].double() - r64["score_dispersity"][b]).abs().max()))
    radius = int(conf.get("nms_radius", 2))
    bars = aliked_bars(e["scores"], e["desc"], e["kpts"], e["disp"], radius)
    k, thr = int(conf.get("max_num_keypoints", -1)), float(conf.get("detection_threshold", 0.2))
    flat = r64["nms_map"].reshape(len(r64["indices"]), -1)
    order = []
    for b in range(flat.shape[0]):
        v = torch.sort(flat[b], descending=True).values
        if thr <= 0 and k > 0:
            assert int((v > 0).sum()) >= k, "fewer than k positive candidates"
            assert float(v[k - 1] - v[k]) > 4 * bars["score"], ("k-th gap", float(v[k - 1] - v[k]), bars["score"])
        else:
            t = thr if thr > 0 else float(r64["score_map"][b].mean())
            assert float((v[v > 0] - t).abs().min()) > 4 * bars["score"], "a candidate sits on the threshold"
        order.append(flat[b][r64["indices"][b]].numpy())
    ref = as_np(r64)
    ref["order_scores"] = order
    _REF_CACHE[key] = (ref, bars, r64)
    return _REF_CACHE[key]


SEEDED = {
    # name: (model, B, H, W, conf, img seed, weight seed, gamma sign)
    "negative_gammas_w64": ("aliked-n16", 1, 40, 64, {"max_num_keypoints": 24, "detection_threshold": 0.0}, 41, 11, "negative"),
    "positive_gammas_h64_t16": ("aliked-t16", 1, 64, 70, {"max_num_keypoints": 24, "detection_threshold": 0.0}, 42, 12, "positive"),
    "nms_radius_3": ("aliked-n16", 1, 48, 80, {"max_num_keypoints": 16, "detection_threshold": 0.0, "nms_radius": 3}, 43, 13, "mixed"),
    "padded_height_32": ("aliked-n16", 1, 20, 72, {"max_num_keypoints": 10, "detection_threshold": 0.0}, 44, 14, "mixed"),
    "batch_3": ("aliked-n16", 3, 56, 72, {"max_num_keypoints": 32, "detection_threshold": 0.0}, 45, 15, "mixed"),
    "mean_threshold": ("aliked-n16", 1, 48, 64, {"max_num_keypoints": -1, "detection_threshold": 0.0}, 46, 16, "mixed"),
}


def seeded(name):
    model, B, H, W, conf, img_seed, w_seed, sign = SEEDED[name]
    conf = dict(conf, model_name=model)
    return conf, aliked_state_dict(model, seed=w_seed, gamma_sign=sign), {"image": synthetic_images(B, 3, H, W, seed=img_seed)}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_aliked_matches_restatement(name):
    conf, sd, data = seeded(name)
    ref, bars, _ = reference_with_margins(name, sd, data, conf)
    out = run(make_model(conf, sd), data)
    compare(as_np(out), ref, bars, name)


# ---- the deformable convolution alone -----------------------------------------------------------
def deform_offsets(B, H, W, rng):
    """Offsets of a few pixels, with planted values: exactly integer, far beyond max(h, w) / 4 (the
    entry does not clamp: that is the caller's offset convolution), and positions just inside and
    just outside the -1 and H (or W) limits."""
    off = rng.standard_normal((B, 18, H, W)) * 1.5
    eps = 1e-3
    y, x = H // 2, W // 2
    off[0, 8:10, y, x] = [1.0, -1.0]                        # centre tap, integer
    off[0, 0:2, 0, 0] = [0.0, 0.0]                          # tap (0,0) at pixel (0,0): position (-1,-1), outside
    off[0, 2:4, 0, 0] = [eps, 0.0]                          # tap (0,1): y = -1 + eps, just inside
    off[0, 4:6, 0, 0] = [-eps, 0.0]                         # y = -1 - eps, just outside
    off[0, 16:18, H - 1, W - 1] = [-eps, -eps]              # tap (2,2): (H - eps, W - eps), just inside
    off[0, 14:16, H - 1, W - 1] = [eps, 0.0]                # tap (2,1): y = H + eps, outside
    off[0, 12:14, H - 1, W - 1] = [0.0, 0.0]                # tap (2,0): y = H exactly, outside
    off[0, 10:12, y, x] = [3.0 * max(H, W), -2.5 * max(H, W)]  # far beyond the clamp
    off[-1, 6:8, y, x] = [-0.5 - y, 0.25]                   # tap (1,0): row -0.5, half of row 0
    return off.astype(np.float32)


@pytest.mark.parametrize("H,W", [(9, 13), (1, 3)])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 64)])
def test_deform_conv_matches_float64(cin, cout, H, W):
    """Bound per output: the fp32 dot product of K = 9 cin terms accumulated in any order errs by at
    most K u sum|w x|, u = 2^-24; the bilinear value is 7 roundings more on each term and the bias
    one: (K + 8) u (sum|w| |x|_sampled + |b|), with the sum taken in float64 over the absolute
    values.  The sample position itself is an fp32 sum (pixel + offset, at most P = max(H, W) + 1 in
    magnitude where it counts), off by at most u P per axis; a bilinear value moves by at most
    2 max|x_c| per unit of position, which adds 4 u P sum_c (sum_t |w|) max|x_c|."""
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(100 * cin + H))
    B = 2
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    off = deform_offsets(B, H, W, rng)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    xd, od, wd, bd = t(x), t(off), t(w), t(bias)
    y = torch.full((B, cout, H, W), float("nan"), device=DEV)
    scratch = torch.empty((9 * cin + 1) * cout, device=DEV)
    p = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.sp_aliked_deform_conv(p(xd), p(od), p(wd), p(bd), B, cin, cout, H, W, p(y), p(scratch),
                                         scratch.numel() * 4, stream), "sp_aliked_deform_conv")
    torch.cuda.synchronize()
    d = lambda a: torch.from_numpy(a).double()  # noqa: E731
    ref = aliked_ref.deform_conv2d(d(x), d(off), d(w), d(bias), padding=1)
    mag = aliked_ref.deform_conv2d(d(x).abs(), d(off), d(w).abs(), d(bias).abs(), padding=1)
    grad = torch.einsum("oc,bc->bo", d(w).abs().sum((2, 3)), d(x).abs().amax((2, 3)))[:, :, None, None]
    bound = (9 * cin + 8) * 2.0 ** -24 * mag + 4 * 2.0 ** -24 * (max(H, W) + 1) * grad
    err = (y.cpu().double() - ref).abs()
    print(f"deform {cin}->{cout} {H}x{W}: max error {float(err.max()):.3g}, max error / bound {float((err / bound).max()):.3g}")
    assert bool(torch.isfinite(y).all())
    assert bool((err <= bound).all())


# ---- batches -------------------------------------------------------------------------------------
def test_aliked_batch_invariance():
    """An image gives the same bits alone and inside a batch of 3."""
    conf, sd, data = seeded("batch_3")
    m = make_model(conf, sd)
    full = run(m, data)
    for b in (0, 2):
        solo = run(m, {"image": data["image"][b:b + 1]})
        for k in OUT_KEYS:
            assert torch.equal(solo[k][0], full[k][b]), (b, k)
    print("batch of 3 against solo runs: identical bits")


def test_aliked_threshold_mode_ragged():
    """Threshold mode with unequal counts: stacking raises, ragged_keypoints returns each image as
    its solo run with zero padding and the counts."""
    model = "aliked-n16"
    sd = aliked_state_dict(model, seed=17)
    image = synthetic_images(3, 3, 48, 64, seed=47)
    conf = {"model_name": model, "max_num_keypoints": -1, "detection_threshold": 0.45}
    m = make_model(conf, sd)
    out = run(m, {"image": image}, ragged_keypoints=True)
    n = out["num_keypoints"].tolist()
    print("threshold-mode counts", n)
    assert len(set(n)) > 1 and min(n) > 0 and out["keypoints"].shape == (3, max(n), 2)
    with pytest.raises(RuntimeError, match="equal size"):
        run(m, {"image": image})
    for b in range(3):
        solo = run(m, {"image": image[b:b + 1]})
        assert solo["keypoints"].shape[1] == n[b]
        for k in ("keypoints", "descriptors", "keypoint_scores", "score_dispersity"):
            assert torch.equal(out[k][b, :n[b]], solo[k][0]), (b, k)
            assert bool((out[k][b, n[b]:] == 0).all()), (b, k)
        assert torch.equal(out["score_map"][b], solo["score_map"][0])
    # row-major order in threshold mode (aliked.py:152)
    px = out["keypoints"][0, :n[0]]
    assert n[0] < 2 or bool((torch.diff(torch.round(px[:, 1])) >= -2.5).all())


def test_aliked_capped_threshold_mode_sorts():
    """More candidates than n_limit: the n_limit best, sorted by score (aliked.py:153-157)."""
    conf, sd, data = seeded("mean_threshold")
    _, _, r64 = reference_with_margins("mean_threshold", sd, data, conf)
    total = len(r64["indices"][0])
    assert total > 12
    capped = dict(conf, max_num_keypoints=8, detection_threshold=1e-6)
    ref = aliked_ref.aliked_forward(sd, data, capped, torch.float64)
    out = run(make_model(capped, sd), data)
    assert out["keypoints"].shape == (1, 8, 2)
    err = float((out["keypoints"][0].double() - ref["keypoints"][0]).abs().max())
    print(f"capped threshold mode: 8 of {int((r64['nms_map'] > 0).sum())} candidates, max keypoint error {err:.3g} px")
    assert err < 0.01


# ---- through the pipeline ------------------------------------------------------------------------
@pytest.mark.parametrize("matcher", [{"name": "matchers.lightglue", "input_dim": 128, "filter_threshold": 0.1},
                                     {"name": "matchers.nearest_neighbor_matcher"}])
def test_aliked_feeds_the_matchers_through_the_pipeline(matcher):
    """TwoViewPipeline(extractor=aliked, matcher=...): the aliked+* configs' shape -- the extractor's
    outputs are the matcher's inputs, all on the device."""
    from lightglue_amd.pipeline import TwoViewPipeline
    from lightglue_amd.weights import synthetic_state_dict

    conf = {"extractor": {"name": "extractors.aliked", "max_num_keypoints": 64, "detection_threshold": 0.0},
            "matcher": matcher}
    pipe = TwoViewPipeline(conf).eval().to(DEV)
    pipe.extractor.load_state_dict(as_torch_sd(aliked_state_dict("aliked-n16", seed=2)), strict=True)
    if matcher["name"] == "matchers.lightglue":
        sd = synthetic_state_dict({"input_dim": 128}, seed=0)
        pipe.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    img = torch.from_numpy(synthetic_images(2, 3, 96, 128, seed=4)).to(DEV)
    view0 = {"image": img[:1], "image_size": torch.tensor([[128.0, 96.0]], device=DEV)}
    view1 = {"image": img[1:], "image_size": torch.tensor([[128.0, 96.0]], device=DEV)}
    with torch.no_grad():
        pred = pipe({"view0": view0, "view1": view1})
        direct = pipe.matcher({"keypoints0": pred["keypoints0"], "keypoints1": pred["keypoints1"],
                               "descriptors0": pred["descriptors0"], "descriptors1": pred["descriptors1"],
                               "view0": view0, "view1": view1})
    assert pred["keypoints0"].shape == (1, 64, 2) and pred["descriptors1"].shape == (1, 64, 128)
    assert pred["keypoint_scores0"].shape == (1, 64) and pred["matches0"].shape == (1, 64)
    assert not torch.equal(pred["keypoints0"], pred["keypoints1"])
    print("matches", int((pred["matches0"] > -1).sum()))
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        torch.testing.assert_close(pred[k], direct[k], rtol=0, atol=0)
