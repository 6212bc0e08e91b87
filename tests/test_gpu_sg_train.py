"""SuperGlue TRAINING step on the GPU (lightglue_amd.SuperGlue in training mode -> sg_train_forward /
sg_train_backward / sg_nll_backward of liblightglue_mi355x.so) against the reference's own autograd
step (tests/golden/sgtrain_*.npz, make_sg_grad_golden.py) and the float64 oracle
(oracle/superglue_train_ref.py) -- needs an MI355X.

Bars, per parameter tensor: max |g_gpu - g64| <= 8 spread32 + 1e-6 max|g64| + 1e-12, where
spread32 is the distance of a float32 autograd gradient from float64: the larger of the
reference's own float32 run (stored in the golden) and the oracle's float32 run (round 5; for a
case without a golden, the oracle's alone).  The HIP step is fp32
arithmetic like the reference's float32 run with other summation orders (and float-atomic dQ
sums).  The same bar holds the descriptor gradients, the BatchNorm running statistics after the
step (the GNN's updated twice per step: forward and the checkpoint recomputation,
superglue.py:151-155) and the log assignment of the training forward.

ReLU kinks (round 5): the float64 oracle is evaluated on the HIP forward's own ReLU decisions
(``SuperGlue.last_relu_masks``, read from the saved post-ReLU activations), so both differentiate
the same piece of the piecewise-linear step; every unit where those decisions differ from
float64's must have a float64 pre-activation within KINK_TOL of 0 (a value whose side fp32 cannot
decide), and the reference golden's sampled gradients (float64's own piece) are compared after the
same piece change (oracle gradient on the HIP piece minus on its own).
"""
import numpy as np
import pytest
import torch

import train_route_cases as rc
from sg_golden_util import ground_truth
from grad_golden_util import desc_golden, desc_pick
from sg_grad_golden_util import golden_entries, load_sgtrain, oracle_sg_step, sgtrain_case, sgtrain_names

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# |float64 pre-activation| below which the HIP forward may take the other ReLU side: relative to the
# BatchNorm call's own scale (max |pre-activation|, at least 1), so a large-valued layer gets no
# looser absolute bar than fp32 rounding there allows (round 5 saw one flip, 2.5e-7 from the kink)
KINK_REL = 1e-5
# how many units may flip at all: kink noise is a handful of units, a systematic sign
# drift of a forward route is not
MAX_FLIPS, MAX_FLIPS_PER_CALL = 8, 4
# canary on the reference-spread-only bar (8 x the reference's own float32 spread, without the
# oracle's): report-level in the bar the tests assert, but a route that drifts far past the
# reference's own rounding (round 5's bf16x6 SuperGlue forward: 405x) fails here too.  Round 5's
# default routes reached 1.19 of this bar (profiles/r05/grad_routes/).
REF_ONLY_CANARY = 2.0


def _relu(masks):
    from oracle.superglue_train_ref import ReluMasks

    return ReluMasks({k: [m.cpu() for m in v] for k, v in masks.items()})


def _check_flips(relu):
    """The units where the HIP forward's ReLU decision differs from float64's sit at the kink, and
    there are few of them."""
    far, per = [], {}
    for name, k, a in relu.flips:
        scale = max(1.0, float(relu.pre[name][k].abs().max()))
        if a >= KINK_REL * scale:
            far.append((name, k, a, scale))
        per[(name, k)] = per.get((name, k), 0) + 1
    assert not far, f"ReLU decisions differ away from the kink: {far[:6]}"
    assert len(relu.flips) <= MAX_FLIPS, f"{len(relu.flips)} ReLU decisions differ: {relu.flips[:8]}"
    assert max(per.values(), default=0) <= MAX_FLIPS_PER_CALL, per
    return len(relu.flips)


def gpu_step(conf, sd, data, gt):
    from lightglue_amd import SuperGlue

    m = SuperGlue(conf).to(DEV)
    full = m.state_dict()
    full.update({k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd.items()})
    m.load_state_dict(full, strict=True)
    m.train()
    m.keep_relu_masks = True
    B = data["keypoints0"].shape[0]
    feed = {k: torch.from_numpy(v).to(DEV) for k, v in data.items() if k not in ("image_size", "image_hw")}
    d0 = feed["descriptors0"].clone().requires_grad_()
    d1 = feed["descriptors1"].clone().requires_grad_()
    feed["descriptors0"], feed["descriptors1"] = d0, d1
    hw = data.get("image_hw", (480, 640))
    view = {"image": torch.zeros(B, 1, *hw, device=DEV)}
    if data.get("image_size") is not None:
        view["image_size"] = torch.from_numpy(np.asarray(data["image_size"], np.float32)).to(DEV)
    feed.update({"view0": view, "view1": dict(view)})
    feed.update({k: torch.from_numpy(v).to(DEV) for k, v in gt.items()})
    pred = m(feed)
    losses = m.loss(pred, feed)
    loss = torch.mean(losses["total"])  # train.py:436
    loss.backward()  # train.py:450
    torch.cuda.synchronize()
    grads = {n: (p.grad.detach().double().cpu().numpy() if p.grad is not None else None) for n, p in m.named_parameters()}
    bufs = {n: b.detach().double().cpu().numpy() for n, b in m.named_buffers() if not n.endswith("num_batches_tracked")}
    nbt = {n: int(b) for n, b in m.named_buffers() if n.endswith("num_batches_tracked")}
    gpu_step.relu_masks = m.last_relu_masks
    return (float(loss.detach()), grads, d0.grad.double().cpu().numpy(), d1.grad.double().cpu().numpy(), bufs, nbt,
            pred["log_assignment"].detach().double().cpu().numpy())


def _check(tag, got, ref, tol, worst, bad):
    e = float(np.abs(got - ref).max())
    worst.append((e / tol, tag))
    if e > tol:
        bad.append((tag, e, tol))


@pytest.mark.parametrize("name", sgtrain_names())
def test_sg_training_step_matches_reference_and_oracle(name):
    g, meta = load_sgtrain(name)
    conf, sd, data, gt = sgtrain_case(meta)
    loss, grads, gd0, gd1, bufs, nbt, la = gpu_step(conf, sd, data, gt)
    assert abs(loss - float(g["loss64"])) <= 1e-5 * abs(float(g["loss64"]))
    relu = _relu(gpu_step.relu_masks)
    oloss, og, ogd0, ogd1, ostats, ola = oracle_sg_step(conf, sd, data, gt, relu=relu)
    nflip = _check_flips(relu)
    # the golden holds float64's own piece: move it onto the HIP forward's (zero without flips)
    shift = {n: 0.0 for n in meta["names"]}
    dshift = (0.0, 0.0)
    if nflip:
        _, og_own, ogd0_own, ogd1_own, _, _ = oracle_sg_step(conf, sd, data, gt)
        shift = {n: og[n] - og_own[n] for n in meta["names"]}
        dshift = (ogd0 - ogd0_own, ogd1 - ogd1_own)
    # spread32 = the larger distance from float64 of two float32 implementations of the step: the
    # reference's own run (in the golden) and the oracle's (round 5: at 512 x 512 the reference's
    # float32 rounding is up to 8x luckier than the oracle's on single tensors -- one sample of an
    # fp32 step's error is not its scale); the oracle's on the same ReLU piece
    _, og32, o32d0, o32d1, ostats32, ola32 = oracle_sg_step(conf, sd, data, gt, dtype=torch.float32,
                                                            relu=_relu(gpu_step.relu_masks))

    def spread(ref32, r64, o32):
        return max(float(ref32), float(np.abs(np.asarray(o32) - r64).max()))
    worst, bad, canary = [], [], []
    for n in meta["names"]:
        assert grads[n] is not None, f"no gradient for {n}"
        tol = 8 * spread(g[f"spread32:{n}"], og[n], og32[n]) + 1e-6 * float(g[f"max64:{n}"]) + 1e-12
        idx, ref = golden_entries(g, n)
        flat = grads[n].reshape(-1)
        sh = np.broadcast_to(np.asarray(shift[n], dtype=np.float64), grads[n].shape).reshape(-1)
        _check(n, flat if idx is None else flat[idx], ref + (sh if idx is None else sh[idx]), tol, worst, bad)
        _check(n + " (oracle)", flat, og[n].reshape(-1), tol, worst, bad)
        ref_tol = 8 * float(g[f"spread32:{n}"]) + 1e-6 * float(g[f"max64:{n}"]) + 1e-12  # the reference's spread only
        e = float(np.abs((flat if idx is None else flat[idx]) - (ref + (sh if idx is None else sh[idx]))).max())
        canary.append((e / ref_tol, n))
    for got, key, r64, r32, dsh in ((gd0, "gdesc0", ogd0, o32d0, dshift[0]), (gd1, "gdesc1", ogd1, o32d1, dshift[1])):
        idx, gref, gmax = desc_golden(g, key)
        tol = 8 * spread(g[f"spread_{key}"], r64, r32) + 1e-6 * gmax + 1e-12
        dsh = np.broadcast_to(np.asarray(dsh, dtype=np.float64), got.shape)
        _check(key, desc_pick(got, idx), gref + desc_pick(dsh, idx), tol, worst, bad)
        _check(key + " (oracle)", got, r64, tol, worst, bad)
    for n, v in bufs.items():
        ref = g[f"buf64:{n}"]
        tol = 8 * spread(g[f"bufspread:{n}"], ostats[n], ostats32[n]) + 1e-6 * np.abs(ref).max() + 1e-12
        _check(n, v, ref, tol, worst, bad)
        _check(n + " (oracle)", v, ostats[n], tol, worst, bad)
    assert nbt == meta["num_batches_tracked"]
    worst.sort(reverse=True)
    canary.sort(reverse=True)
    print(name, "loss", loss, "ReLU kink flips", nflip, "worst err/tol:", [(n, round(r, 3)) for r, n in worst[:6]],
          "reference-spread-only:", [(n, round(r, 3)) for r, n in canary[:3]])
    assert not bad, bad[:12]
    assert canary[0][0] <= REF_ONLY_CANARY, canary[:4]
    # the training forward's log assignment against the oracle's (float32 oracle run for the scale)
    la_spread = float(np.abs(ola32.double().numpy() - ola.numpy()).max())
    np.testing.assert_allclose(la, ola.numpy(), atol=max(1e-5, 8 * la_spread), rtol=0)


@pytest.mark.parametrize("B,M,N,layers,iters", [(3, 50, 37, ["self", "cross"], 10), (1, 33, 70, ["cross"], 7),
                                                rc.SG_UNFUSED, rc.SG_NOT_DEFERRED])
def test_sg_training_step_ragged_against_oracle(B, M, N, layers, iters):
    """Shapes the goldens do not cover (odd sizes, M != N, B = 1 and 3) against the float64 oracle;
    the bar's spread comes from the oracle's own float32 step.  The last two cases leave the fused
    Sinkhorn (train_route_cases: N + 1 > 64 SKF_Q takes the unfused forward and backward,
    iters > SKA_TMAX the fused backward that is not deferred)."""
    from lightglue_amd.sg_weights import superglue_state_dict, synthetic_scores
    from lightglue_amd.weights import synthetic_pair

    conf = {"GNN_layers": layers, "num_sinkhorn_iterations": iters, "keypoint_encoder": [16, 32]}
    sd = superglue_state_dict(conf, seed=11)
    p = synthetic_pair(B, M, N, seed=12, width=640, height=480)
    data = {"keypoints0": p["keypoints0"], "keypoints1": p["keypoints1"], "descriptors0": p["descriptors0"],
            "descriptors1": p["descriptors1"], "keypoint_scores0": synthetic_scores(B, M, seed=13),
            "keypoint_scores1": synthetic_scores(B, N, seed=14), "image_hw": (480, 640)}
    gt = ground_truth(B, M, N, 15)
    loss, grads, gd0, gd1, bufs, nbt, la = gpu_step(conf, sd, data, gt)
    relu = _relu(gpu_step.relu_masks)
    l64, og, ogd0, ogd1, ostats, _ = oracle_sg_step(conf, sd, data, gt, relu=relu)
    _check_flips(relu)
    l32, og32, o32d0, o32d1, ostats32, _ = oracle_sg_step(conf, sd, data, gt, dtype=torch.float32,
                                                          relu=_relu(gpu_step.relu_masks))
    assert abs(loss - l64) <= 1e-5 * abs(l64)
    worst, bad = [], []
    for n, ref in og.items():
        tol = 8 * float(np.abs(og32[n] - ref).max()) + 1e-6 * float(np.abs(ref).max()) + 1e-12
        _check(n, grads[n], ref, tol, worst, bad)
    for got, ref, r32, key in ((gd0, ogd0, o32d0, "gdesc0"), (gd1, ogd1, o32d1, "gdesc1")):
        _check(key, got, ref, 8 * float(np.abs(r32 - ref).max()) + 1e-6 * np.abs(ref).max() + 1e-12, worst, bad)
    for n, ref in ostats.items():
        _check(n, bufs[n], ref, 8 * float(np.abs(ostats32[n] - ref).max()) + 1e-6 * np.abs(ref).max() + 1e-12, worst, bad)
    worst.sort(reverse=True)
    print("ragged", B, M, N, "worst err/tol:", [(n, round(r, 3)) for r, n in worst[:6]])
    assert not bad, bad[:12]
    assert all(v == (4 if n.startswith("gnn.") else 2) for n, v in nbt.items())


def test_sg_training_sinkhorn_column_fallback(monkeypatch):
    """The fused Sinkhorn iteration's column statistic S_j = sum_i e_ij a_i falls back to an exact
    two-pass LSE over the column when S_j is tiny (sk_fwd_colfinal_kernel); LG_SKF_EXACT=1 takes
    that path for every column.  Both runs match the float64 oracle's log assignment and
    gradients (the ragged test's bars) and each other's log assignment."""
    from lightglue_amd.sg_weights import superglue_state_dict, synthetic_scores
    from lightglue_amd.weights import synthetic_pair

    conf = {"GNN_layers": ["self", "cross"], "num_sinkhorn_iterations": 12, "keypoint_encoder": [16, 32]}
    sd = superglue_state_dict(conf, seed=31)
    B, M, N = 2, 45, 61
    p = synthetic_pair(B, M, N, seed=32, width=640, height=480)
    data = {"keypoints0": p["keypoints0"], "keypoints1": p["keypoints1"], "descriptors0": p["descriptors0"],
            "descriptors1": p["descriptors1"], "keypoint_scores0": synthetic_scores(B, M, seed=33),
            "keypoint_scores1": synthetic_scores(B, N, seed=34), "image_hw": (480, 640)}
    gt = ground_truth(B, M, N, 35)
    fused = gpu_step(conf, sd, data, gt)
    monkeypatch.setenv("LG_SKF_EXACT", "1")
    exact = gpu_step(conf, sd, data, gt)
    _, og, _, _, _, ola = oracle_sg_step(conf, sd, data, gt)
    _, og32, _, _, _, ola32 = oracle_sg_step(conf, sd, data, gt, dtype=torch.float32)
    spread = float(np.abs(ola32.double().numpy() - ola.numpy()).max())
    for run in (fused, exact):
        np.testing.assert_allclose(run[6], ola.numpy(), atol=max(1e-5, 8 * spread), rtol=0)
        for n, ref in og.items():  # the ragged test's bar, per run
            tol = 8 * float(np.abs(og32[n] - ref).max()) + 1e-6 * float(np.abs(ref).max()) + 1e-12
            assert float(np.abs(run[1][n] - ref).max()) <= tol, n
    np.testing.assert_allclose(fused[6], exact[6], atol=max(1e-5, 8 * spread), rtol=0)


def test_nll_losses_are_differentiable():
    """SuperGlue.loss (mode 0) and NLLLoss (mode 1) backward (sg_nll_backward) against torch autograd
    of the oracle restatements (float64), including gradients of nll_pos / nll_neg."""
    from lightglue_amd import SuperGlue
    from lightglue_amd.superglue import NLLLoss
    from oracle.superglue_ref import nll_loss, superglue_loss

    B, M = 3, 40
    gt = ground_truth(B, M, M, 4)
    rng = np.random.Generator(np.random.PCG64(9))
    la0 = (rng.standard_normal((B, M + 1, M + 1)) - 3.0).astype(np.float32)
    gtd = {k: torch.from_numpy(v).to(DEV) for k, v in gt.items()}
    w = torch.from_numpy(rng.standard_normal((3, B)).astype(np.float32))
    # SuperGlue.loss
    la = torch.from_numpy(la0).to(DEV).requires_grad_()
    out = SuperGlue({"GNN_layers": []}).to(DEV).loss({"log_assignment": la}, gtd)
    (w[0].to(DEV) * out["total"] + w[1].to(DEV) * out["nll_pos"] + w[2].to(DEV) * out["nll_neg"]).sum().backward()
    la64 = torch.from_numpy(la0).double().requires_grad_()
    ref = superglue_loss(la64, gt["gt_assignment"], gt["gt_matches0"], gt["gt_matches1"])
    (w[0].double() * ref["total"] + w[1].double() * ref["nll_pos"] + w[2].double() * ref["nll_neg"]).sum().backward()
    np.testing.assert_allclose(la.grad.cpu().double().numpy(), la64.grad.numpy(), atol=1e-7, rtol=1e-5)
    # NLLLoss (losses.py), M == N
    la = torch.from_numpy(la0).to(DEV).requires_grad_()
    total, _, metrics = NLLLoss({"nll_balancing": 0.3})({"log_assignment": la}, gtd)
    (w[0].to(DEV) * total + w[1].to(DEV) * metrics["nll_pos"]).sum().backward()
    la64 = torch.from_numpy(la0).double().requires_grad_()
    t64, m64 = nll_loss(la64, gt["gt_assignment"], gt["gt_matches0"], gt["gt_matches1"], 0.3)
    (w[0].double() * t64 + w[1].double() * m64["nll_pos"]).sum().backward()
    np.testing.assert_allclose(la.grad.cpu().double().numpy(), la64.grad.numpy(), atol=1e-7, rtol=1e-5)


def test_training_refuses_non_default_batchnorm_settings():
    """The training kernels update running statistics with nn.BatchNorm1d's defaults; a module with
    another momentum (None = cumulative average included) is refused, not silently ignored."""
    from lightglue_amd import SuperGlue
    from lightglue_amd.sg_weights import synthetic_scores
    from lightglue_amd.weights import synthetic_pair

    m = SuperGlue({"GNN_layers": ["self"], "num_sinkhorn_iterations": 3, "keypoint_encoder": [16]}).to(DEV)
    m.train()
    bn = next(mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d))
    bn.momentum = None
    p = synthetic_pair(1, 20, 24, seed=1, width=640, height=480)
    feed = {k: torch.from_numpy(v).to(DEV) for k, v in p.items() if k.startswith(("keypoints", "descriptors"))}
    feed["keypoint_scores0"] = torch.from_numpy(synthetic_scores(1, 20, seed=2)).to(DEV)
    feed["keypoint_scores1"] = torch.from_numpy(synthetic_scores(1, 24, seed=3)).to(DEV)
    view = {"image": torch.zeros(1, 1, 480, 640, device=DEV)}
    feed.update({"view0": view, "view1": dict(view)})
    with pytest.raises(NotImplementedError, match="momentum"):
        m(feed)


def test_nll_loss_workspace_entry_equals_allocating_entry():
    """sg_nll_loss_ws (caller workspace, what the binding uses) == sg_nll_loss (stream-ordered
    allocation inside) bit for bit, both modes."""
    import ctypes

    from lightglue_amd import _lib

    lib = _lib.load()
    B, M = 2, 33
    gt = ground_truth(B, M, M, 6)
    rng = np.random.Generator(np.random.PCG64(3))
    la = torch.from_numpy((rng.standard_normal((B, M + 1, M + 1)) - 3.0).astype(np.float32)).to(DEV)
    gta = torch.from_numpy(gt["gt_assignment"]).to(DEV).to(torch.uint8)
    g0 = torch.from_numpy(gt["gt_matches0"]).to(DEV, torch.int64)
    g1 = torch.from_numpy(gt["gt_matches1"]).to(DEV, torch.int64)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    nb = ctypes.c_size_t()
    _lib.check(lib.sg_nll_workspace_bytes(B, M, ctypes.byref(nb)), "bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    for mode in (0, 1):
        a, b = torch.empty(5, B, device=DEV), torch.empty(5, B, device=DEV)
        _lib.check(lib.sg_nll_loss(p(la), B, M, M, p(gta), p(g0), p(g1), mode, 0.5, p(a), st), "nll")
        _lib.check(lib.sg_nll_loss_ws(p(la), B, M, M, p(gta), p(g0), p(g1), mode, 0.5, p(b), p(ws), nb.value, st), "ws")
        assert torch.equal(a, b)
    small = torch.empty(5, B, device=DEV)
    assert lib.sg_nll_loss_ws(p(la), B, M, M, p(gta), p(g0), p(g1), 0, 0.5, p(small), p(ws), nb.value - 8, st) == \
        _lib.LG_E_WORKSPACE
