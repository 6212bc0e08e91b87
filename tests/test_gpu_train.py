"""LightGlue backward pass on the HIP library (training path, include/lightglue_mi355x.h
"Training") -- needs an MI355X.

Gradients are checked two ways:
* against the reference's own autograd gradients (tests/golden/grad_*.npz, make_grad_golden.py:
  float64 values at seeded sample positions), and
* against the float64 autograd gradients of the oracle restatement (oracle/lightglue_train_ref.py,
  itself pinned to those goldens by tests/test_oracle_grad.py) on EVERY entry of every tensor.
Bar per tensor: max |g_gpu - g64| <= 8 * spread32 + 1e-6 * max|g64| + 1e-12, where spread32 is
how far a float32 autograd gradient lies from float64: the larger of the reference's own float32
run (stored in the golden) and the oracle's float32 run (round 5; one run's rounding luck is not
the scale -- at N = 512 the two differ by up to 8x on single tensors).
The HIP path is fp32 arithmetic like the reference's float32 run, with different summation orders
(and float-atomic dQ sums), so a few spreads of headroom are the right scale.
Kernel-level checks: the training GEMM in every transpose form (split-k included), on its bf16x6
route and on the f32 matrix cores, and the training attention forward / backward against float64
torch.  Which kernel runs follows from shape and alignment alone, so the shapes are chosen to reach
every route: train_route_cases.py lists them with the launcher conditions they rest on.
"""
import ctypes

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import train_route_cases as rc
from grad_golden_util import desc_golden, desc_pick, golden_entries, grad_case, grad_names, load_grad, oracle_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _lib():
    from lightglue_amd import _lib

    return _lib, _lib.load()


# ------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K,batch", [(200, 136, 72, 1), (37, 300, 129, 3), (256, 512, 5000, 1), (33, 17, 4100, 2)])
def test_train_gemm_matches_fp64(ta, tb, M, N, K, batch):
    L, lib = _lib()
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A = torch.randn((batch, K, M) if ta else (batch, M, K), generator=g)
    Bm = torch.randn((batch, N, K) if tb else (batch, K, N), generator=g)
    C0 = torch.randn((batch, M, N), generator=g)
    bias = torch.randn(N, generator=g)
    alpha, beta = 0.75, 1.0
    ref = alpha * ((A.transpose(1, 2) if ta else A).double() @ (Bm.transpose(1, 2) if tb else Bm).double()
                   + bias.double()) + beta * C0.double()
    Ad, Bd, Cd, bd = A.to(DEV), Bm.to(DEV), C0.to(DEV), bias.to(DEV)
    nb = ctypes.c_size_t()
    L.check(lib.lg_train_gemm_workspace_bytes(M, N, K, batch, ctypes.byref(nb)), "ws")
    ws = torch.empty(max(nb.value, 4), dtype=torch.uint8, device=DEV)
    lda = A.shape[2]
    ldb = Bm.shape[2]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.lg_train_gemm(_p(Ad), _p(Bd), _p(Cd), lda, ldb, N, A[0].numel(), Bm[0].numel(), M * N, M, N, K, batch,
                              alpha, beta, _p(bd), ta, tb, _p(ws), nb.value, st), "lg_train_gemm")
    err = (Cd.cpu().double() - ref).abs().max().item()
    # fp32 accumulation over K terms of |a b| ~ 1: a few ulps of sqrt(K)-scale sums
    assert err <= 2e-6 * max(K, 64) ** 0.5 * 8, err


def _gemm_bar(K):
    """test_train_gemm_matches_fp64's bar: bf16x6 is fp32-accurate per product, so it carries over."""
    return 2e-6 * max(K, 64) ** 0.5 * 8


def _gemm_ws(L, lib, M, N, K, batch):
    nb = ctypes.c_size_t()
    L.check(lib.lg_train_gemm_workspace_bytes(M, N, K, batch, ctypes.byref(nb)), "ws")
    return torch.empty(max(nb.value, 4), dtype=torch.uint8, device=DEV), nb.value


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("case", rc.GEMM_CASES, ids=[c["name"] for c in rc.GEMM_CASES])
def test_train_gemm_routes_match_fp64(case):
    """tgemm's bf16x6 route (every linear layer's forward, every input gradient, the heads'
    similarity) and the shapes that must leave it for the f32 kernels, each against float64 torch at
    test_train_gemm_matches_fp64's bar.  The cases and the launcher condition each one rests on are
    in train_route_cases.GEMM_CASES (checked against the launcher's text by test_host.py)."""
    L, lib = _lib()
    c = case
    ta, tb, batch, M, N, K, pad = c["ta"], c["tb"], c["batch"], c["M"], c["N"], c["K"], c["pad"]
    assert not ta
    g = torch.Generator().manual_seed(M * 7 + N + K)
    lda, ldc = K + pad, N + pad
    A = torch.randn((batch, M, lda), generator=g)
    Bm = torch.randn((batch, N, K) if tb else (batch, K, N), generator=g)
    C0 = torch.randn((batch, M, ldc), generator=g)
    bias = torch.randn(N, generator=g) if c["bias"] else None
    alpha, beta = c["alpha"], c["beta"]
    ref = A[:, :, :K].double() @ (Bm.transpose(1, 2) if tb else Bm).double()
    if bias is not None:
        ref = ref + bias.double()
    ref = alpha * ref + beta * C0[:, :, :N].double()
    off = c["a_offset"]  # floats past the (256-byte aligned) allocation
    abuf = torch.empty(A.numel() + off, device=DEV)
    abuf[off:] = A.flatten().to(DEV)
    Ad = abuf[off:]
    assert Ad.data_ptr() % 16 == 4 * off
    Cin = torch.full_like(C0, float("nan")) if c["nan_c"] else C0.clone()
    if c["nan_c"]:
        assert beta == 0.0
    Bd, Cd = Bm.to(DEV), Cin.to(DEV)
    bd = bias.to(DEV) if bias is not None else None
    ws, nb = _gemm_ws(L, lib, M, N, K, batch)
    L.check(lib.lg_train_gemm(_p(Ad), _p(Bd), _p(Cd), lda, Bm.shape[2], ldc, M * lda, Bm[0].numel(), M * ldc, M, N, K,
                              batch, alpha, beta, _p(bd), ta, tb, _p(ws), nb, _stream()), "lg_train_gemm")
    got = Cd.cpu()
    err = (got[:, :, :N].double() - ref).abs().max().item()
    print(c["name"], c["route"], f"err {err:.3g} / bar {_gemm_bar(K):.3g}")
    assert err <= _gemm_bar(K), err  # NaN (beta = 0 reading C) fails here too
    if pad:
        assert torch.equal(got[:, :, N:], C0[:, :, N:]), "C's padding columns were written"


def _gemm_ex(L, lib, A, Bm, C, lda, ldb, ldc, M, N, K, alpha, beta, bias, ta, tb, *, A1=None, lda1=0, K0=0, B1=None, ldb1=0,
             N0=0, R=None, ldr=0, colsum=None):
    ws, nb = _gemm_ws(L, lib, M, N, K, 1)
    return lib.lg_train_gemm_ex(_p(A), _p(Bm), _p(C), lda, ldb, ldc, 0, 0, 0, M, N, K, 1, alpha, beta, _p(bias), ta, tb, _p(A1),
                                lda1, K0, _p(B1), ldb1, N0, _p(R), ldr, _p(colsum), _p(ws), nb, _stream())


def test_train_gemm_two_source_a_matches_fp64():
    """ffn.0's forward: op(A) = [A | A1] along k, A1 a 256-column window of a 512-wide buffer (the
    message half of CAT), on the bf16x6 route; the reference is the product on cat([A, A1], 1)."""
    L, lib = _lib()
    s = rc.GEMM_EX["a1"]
    M, N, K, K0 = s["M"], s["N"], s["K"], s["K0"]
    g = torch.Generator().manual_seed(21)
    A, cat = torch.randn(M, K0, generator=g), torch.randn(M, 2 * (K - K0), generator=g)
    W, bias = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    ref = torch.cat([A, cat[:, K - K0:]], 1).double() @ W.double().T + bias.double()
    Ad, catd, Wd, bd = A.to(DEV), cat.to(DEV), W.to(DEV), bias.to(DEV)
    Cd = torch.full((M, N), float("nan"), device=DEV)
    L.check(_gemm_ex(L, lib, Ad, Wd, Cd, K0, K, N, M, N, K, 1.0, 0.0, bd, 0, 1, A1=catd[:, K - K0:], lda1=cat.shape[1], K0=K0),
            "lg_train_gemm_ex")
    err = (Cd.cpu().double() - ref).abs().max().item()
    print(f"a1: err {err:.3g} / bar {_gemm_bar(K):.3g}")
    assert err <= _gemm_bar(K), err


@pytest.mark.parametrize("key", ["b1_split", "b1_whole", "colsum_scalar"])
def test_train_gemm_weight_gradient_sources_and_column_sums_match_fp64(key):
    """A weight gradient dW = dY^T [X | message] with its bias gradient colsum(dY) from the same read
    of dY (TGemm::colsumA): the two-source B of the vectorised kernel with and without the k split
    (the split's last chunk partial, the column-sum partials reduced by tgemm_reduce_kernel), and the
    column sums of the non-vector kernel."""
    L, lib = _lib()
    s = rc.GEMM_EX[key]
    M, N, K, N0 = s["M"], s["N"], s["K"], s.get("N0", 0)
    g = torch.Generator().manual_seed(K + M)
    dY = torch.randn(K, M, generator=g)  # k-major A
    X = torch.randn(K, N0 or N, generator=g)
    cat = torch.randn(K, 2 * (N - N0), generator=g) if N0 else None
    Bfull = torch.cat([X, cat[:, N - N0:]], 1) if N0 else X
    ref = dY.double().T @ Bfull.double()
    ref_cs = dY.double().sum(0)
    dYd, Xd = dY.to(DEV), X.to(DEV)
    catd = cat.to(DEV) if N0 else None
    Cd = torch.full((M, N), float("nan"), device=DEV)
    cs = torch.full((M,), float("nan"), device=DEV)
    kw = dict(B1=catd[:, N - N0:], ldb1=cat.shape[1], N0=N0) if N0 else {}
    L.check(_gemm_ex(L, lib, dYd, Xd, Cd, M, X.shape[1], N, M, N, K, 1.0, 0.0, None, 1, 0, colsum=cs, **kw), "lg_train_gemm_ex")
    err = (Cd.cpu().double() - ref).abs().max().item()
    err_cs = (cs.cpu().double() - ref_cs).abs().max().item()
    print(f"{key}: err {err:.3g}, colsum err {err_cs:.3g} / bar {_gemm_bar(K):.3g}")
    assert err <= _gemm_bar(K), err
    assert err_cs <= _gemm_bar(K), err_cs  # a sum of K unit-variance terms, like one output entry


@pytest.mark.parametrize("key", ["res_x6", "res_f32"])
def test_train_gemm_residual_source_matches_fp64(key):
    """C = A B^T + bias + R with R != C (TGemm::R, ffn.3's residual): read by the bf16x6 epilogue
    (K = 256) or copied into C first for the f32 kernels (K = 72); C's initial NaNs must not be
    read and R comes back unmodified."""
    L, lib = _lib()
    s = rc.GEMM_EX[key]
    M, N, K = s["M"], s["N"], s["K"]
    g = torch.Generator().manual_seed(K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, R = torch.randn(N, generator=g), torch.randn(M, N + 4, generator=g)
    ref = A.double() @ W.double().T + bias.double() + R[:, :N].double()
    Ad, Wd, bd, Rd = A.to(DEV), W.to(DEV), bias.to(DEV), R.to(DEV)
    Cd = torch.full((M, N), float("nan"), device=DEV)
    L.check(_gemm_ex(L, lib, Ad, Wd, Cd, K, K, N, M, N, K, 1.0, 1.0, bd, 0, 1, R=Rd, ldr=N + 4), "lg_train_gemm_ex")
    err = (Cd.cpu().double() - ref).abs().max().item()
    print(f"{key}: err {err:.3g} / bar {_gemm_bar(K):.3g}")
    assert err <= _gemm_bar(K), err
    assert torch.equal(Rd.cpu(), R)


@pytest.mark.parametrize("key", ["refuse_a1", "refuse_b1"])
def test_train_gemm_refuses_operands_no_route_takes(key):
    """A two-source A off the bf16x6 route (K % 16 != 0) and a two-source B whose first part is no
    multiple of the 128-wide tile come back as LG_E_INVALID with C untouched."""
    L, lib = _lib()
    s = rc.GEMM_EX[key]
    M, N, K = s["M"], s["N"], s["K"]
    Cd = torch.full((M, N), 7.0, device=DEV)
    if key == "refuse_a1":
        K0 = s["K0"]
        Ad, A1d, Bd = torch.ones(M, K0, device=DEV), torch.ones(M, K - K0, device=DEV), torch.ones(N, K, device=DEV)
        rcode = _gemm_ex(L, lib, Ad, Bd, Cd, K0, K, N, M, N, K, 1.0, 0.0, None, 0, 1, A1=A1d, lda1=K - K0, K0=K0)
    else:
        N0 = s["N0"]
        Ad, Bd, B1d = torch.ones(K, M, device=DEV), torch.ones(K, N0, device=DEV), torch.ones(K, N - N0, device=DEV)
        rcode = _gemm_ex(L, lib, Ad, Bd, Cd, M, N0, N, M, N, K, 1.0, 0.0, None, 1, 0, B1=B1d, ldb1=N - N0, N0=N0)
    torch.cuda.synchronize()
    assert rcode == L.LG_E_INVALID, (rcode, lib.lg_last_error())
    assert bool((Cd == 7.0).all())


def _attn_ref(q, k, v, scale):
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("B,Nq,Nk", [(2, 96, 96), (1, 200, 77), (3, 33, 300), (1, 1, 5)] + rc.ATTN_MULTIBLOCK)
def test_train_attention_forward_backward_fp64(B, Nq, Nk):
    L, lib = _lib()
    H, scale = 4, 0.125
    g = torch.Generator().manual_seed(B * 1000 + Nq + Nk)
    q = torch.randn(B, Nq, 256, generator=g) * 2
    k = torch.randn(B, Nk, 256, generator=g) * 2
    v = torch.randn(B, Nk, 256, generator=g)
    go = torch.randn(B, Nq, 256, generator=g)

    def heads(t):
        return t.double().unflatten(-1, (H, 64)).transpose(1, 2)

    qd, kd, vd = (heads(t).requires_grad_() for t in (q, k, v))
    o = _attn_ref(qd, kd, vd, scale)
    o.backward(heads(go))
    o_ref = o.detach().transpose(1, 2).flatten(-2)
    dq_ref, dk_ref, dv_ref = (t.grad.transpose(1, 2).flatten(-2) for t in (qd, kd, vd))

    qg, kg, vg, gog = (t.to(DEV).contiguous() for t in (q, k, v, go))
    og = torch.empty(B, Nq, 256, device=DEV)
    lse = torch.empty(B * H * Nq, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.lg_train_attention(_p(qg), _p(kg), _p(vg), B, H, Nq, Nk, scale, _p(og), _p(lse), st), "fwd")
    np.testing.assert_allclose(og.cpu().double().numpy(), o_ref.numpy(), atol=2e-5, rtol=1e-5)
    s = torch.einsum("bhid,bhjd->bhij", heads(q), heads(k)) * scale
    lse_ref = torch.logsumexp(s, -1).flatten() / np.log(2.0)
    np.testing.assert_allclose(lse.cpu().double().numpy(), lse_ref.numpy(), atol=2e-5, rtol=1e-6)
    dq, dk, dv = (torch.empty_like(t) for t in (qg, kg, vg))
    delta = torch.empty(B * H * Nq, device=DEV)
    L.check(lib.lg_train_attention_backward(_p(qg), _p(kg), _p(vg), _p(og), _p(lse), _p(gog), B, H, Nq, Nk, scale,
                                            _p(dq), _p(dk), _p(dv), _p(delta), st), "bwd")
    for got, ref in ((dq, dq_ref), (dk, dk_ref), (dv, dv_ref)):
        r = ref.numpy()
        np.testing.assert_allclose(got.cpu().double().numpy(), r, atol=2e-5 * max(1.0, np.abs(r).max()), rtol=1e-5)


# ------------------------------------------------------------------ full backward
REF_ONLY_CANARY = 2.0  # see test_gpu_sg_train.py


def _gpu_grads(conf, sd, pair, gt):
    from lightglue_amd import LightGlue

    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.train()
    data = {k: torch.from_numpy(v).to(DEV) for k, v in pair.items()
            if not k.startswith(("image_size", "descriptors"))}
    d0 = torch.from_numpy(pair["descriptors0"]).to(DEV).requires_grad_()
    d1 = torch.from_numpy(pair["descriptors1"]).to(DEV).requires_grad_()
    data["descriptors0"], data["descriptors1"] = d0, d1
    data["view0"] = {"image_size": torch.from_numpy(pair["image_size0"]).to(DEV)}
    data["view1"] = {"image_size": torch.from_numpy(pair["image_size1"]).to(DEV)}
    data.update({k: torch.from_numpy(v).to(DEV) for k, v in gt.items()})
    pred = model(data)
    losses, _ = model.loss(pred, data)
    loss = torch.mean(losses["total"])  # train.py:436
    loss.backward()  # train.py:450
    grads = {n: (p.grad.detach().double().cpu().numpy() if p.grad is not None else None)
             for n, p in model.named_parameters()}
    return float(loss.detach()), grads, d0.grad.double().cpu().numpy(), d1.grad.double().cpu().numpy(), pred


@pytest.mark.parametrize("name", grad_names())
def test_backward_matches_reference_and_oracle(name):
    g, meta = load_grad(name)
    conf, sd, pair, gt = grad_case(meta)
    loss, grads, gd0, gd1, pred = _gpu_grads(conf, sd, pair, gt)
    assert abs(loss - float(g["loss64"])) <= 1e-4 * abs(float(g["loss64"]))
    _, og, ogd0, ogd1 = oracle_grads(conf, sd, pair, gt)
    # spread32 = the larger distance from float64 of two float32 implementations: the reference's
    # own run (golden) and the oracle's (round 5: one fp32 run's rounding luck is not the scale)
    _, og32, o32d0, o32d1 = oracle_grads(conf, sd, pair, gt, dtype=torch.float32)

    def spread(ref32, r64, o32):
        return max(float(ref32), float(np.abs(np.asarray(o32) - r64).max()))
    worst, bad, canary = [], [], []
    for n in meta["names"]:
        assert grads[n] is not None, f"no gradient for {n}"
        tol = 8 * spread(g[f"spread32:{n}"], og[n], og32[n]) + 1e-6 * float(g[f"max64:{n}"]) + 1e-12
        idx, ref = golden_entries(g, n)
        got = grads[n].reshape(-1)
        e_gold = np.abs((got if idx is None else got[idx]) - ref).max()
        e_full = np.abs(got - og[n].reshape(-1)).max()
        worst.append((max(e_gold, e_full) / tol, n))
        if e_gold > tol or e_full > tol:
            bad.append((n, float(e_gold), float(e_full), tol, float(g[f"max64:{n}"])))
        # canary on the bar of the reference's own float32 spread alone (round 5's
        # default routes reached 1.19 of it, profiles/r05/grad_routes/)
        canary.append((float(e_gold) / (8 * float(g[f"spread32:{n}"]) + 1e-6 * float(g[f"max64:{n}"]) + 1e-12), n))
    for got, ref, r32, key in ((gd0, ogd0, o32d0, "gdesc0"), (gd1, ogd1, o32d1, "gdesc1")):
        idx, gref, gmax = desc_golden(g, key)
        tol = 8 * spread(g[f"spread_{key}"], ref, r32) + 1e-6 * gmax + 1e-12
        e_gold, e_full = np.abs(desc_pick(got, idx) - gref).max(), np.abs(got - ref).max()
        worst.append((max(e_gold, e_full) / tol, key))
        if e_gold > tol or e_full > tol:
            bad.append((key, float(e_gold), float(e_full), tol, gmax))
    worst.sort(reverse=True)
    canary.sort(reverse=True)
    print(name, "loss", loss, "worst err/tol:", [(n, round(r, 3)) for r, n in worst[:6]],
          "reference-spread-only:", [(n, round(r, 3)) for r, n in canary[:3]])
    assert not bad, bad[:12]
    assert canary[0][0] <= REF_ONLY_CANARY, canary[:4]


@pytest.mark.parametrize("name", ["grad_train_b2_n64", "grad_train_l3_b2_n96_proj_ori"])
def test_checkpointed_step_matches_full_step(name):
    """conf ``checkpointed`` (lightglue.py:353,515-518; LG_FWD_CHECKPOINTED): the training call keeps
    each layer's output only and the backward recomputes every layer's activations before
    differentiating it.  The forward kernels are deterministic, so the loss and the log assignment
    equal the full step's bit for bit; the gradients equal it up to the float-atomic dQ sums'
    order (checked at the golden's bar form); the saved buffer at the configs[2] shape shrinks
    below a quarter."""
    g, meta = load_grad(name)
    conf, sd, pair, gt = grad_case(meta)
    loss_f, grads_f, gd0_f, gd1_f, pred_f = _gpu_grads(conf, sd, pair, gt)
    loss_c, grads_c, gd0_c, gd1_c, pred_c = _gpu_grads({**conf, "checkpointed": True}, sd, pair, gt)
    assert loss_c == loss_f
    assert torch.equal(pred_c["log_assignment"], pred_f["log_assignment"])
    bad = []
    for n in meta["names"]:
        tol = 8 * float(g[f"spread32:{n}"]) + 1e-6 * float(g[f"max64:{n}"]) + 1e-12
        e = float(np.abs(grads_c[n] - grads_f[n]).max())
        if e > tol:
            bad.append((n, e, tol))
    for key, a, b in (("gdesc0", gd0_c, gd0_f), ("gdesc1", gd1_c, gd1_f)):
        _, _, gmax = desc_golden(g, key)
        tol = 8 * float(g[f"spread_{key}"]) + 1e-6 * gmax + 1e-12
        if float(np.abs(a - b).max()) > tol:
            bad.append((key, float(np.abs(a - b).max()), tol))
    assert not bad, bad[:8]
    from lightglue_amd import LightGlue
    from lightglue_amd import _lib as L

    model = LightGlue({"n_layers": 9}).to(DEV)
    lib = model._ensure_handle(DEV, upload=False)
    full, ck = ctypes.c_size_t(), ctypes.c_size_t()
    L.check(lib.lg_train_saved_bytes_ex(model._handle, 32, 2048, 2048, L.LG_FWD_TRAINING_GATE, ctypes.byref(full)), "sb")
    L.check(lib.lg_train_saved_bytes_ex(model._handle, 32, 2048, 2048, L.LG_FWD_TRAINING_GATE | L.LG_FWD_CHECKPOINTED,
                                        ctypes.byref(ck)), "sb")
    plain = ctypes.c_size_t()
    L.check(lib.lg_train_saved_bytes(model._handle, 32, 2048, 2048, ctypes.byref(plain)), "sb")
    assert plain.value == full.value
    print(name, f"saved bytes at configs[2]: full {full.value / 2**30:.2f} GiB, checkpointed {ck.value / 2**30:.2f} GiB")
    assert ck.value < full.value / 4


def test_training_forward_matches_eval_forward_descriptors():
    """The autograd training forward (fp32 f32-MFMA kernels) and the no-grad training-mode forward
    (the fp16x3 eval kernels with the training gate) produce the same per-layer descriptors."""
    from lightglue_amd import LightGlue
    from lightglue_amd.weights import synthetic_pair, synthetic_state_dict

    conf = {"filter_threshold": 0.1, "n_layers": 3}
    sd = synthetic_state_dict(conf, seed=2)
    pair = synthetic_pair(B=2, M=100, N=90, seed=5)
    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train()
    data = {k: torch.from_numpy(v).to(DEV) for k, v in pair.items() if not k.startswith("image_size")}
    data["view0"] = {"image_size": torch.from_numpy(pair["image_size0"]).to(DEV)}
    data["view1"] = {"image_size": torch.from_numpy(pair["image_size1"]).to(DEV)}
    with torch.no_grad():
        ref = model(data)
    pred = model(data)
    assert pred["ref_descriptors0"].requires_grad
    for k in ("ref_descriptors0", "ref_descriptors1", "log_assignment"):
        np.testing.assert_allclose(pred[k].detach().cpu().numpy(), ref[k].cpu().numpy(), atol=1e-4, rtol=1e-4)
    assert torch.equal(pred["matches0"], ref["matches0"])


@pytest.mark.parametrize("tokens", [True, False])
def test_head_backward_from_forward_equals_recompute(tokens):
    """lg_head_backward_from_forward (the loss heads reuse their forward's md / z / similarity /
    LSEs) gives the recomputing lg_head_backward's gradients bit for bit: the forward kernels are
    deterministic, so the saved values are the recomputed ones."""
    from lightglue_amd import LightGlue
    from lightglue_amd.lightglue import _head_backward, _head_forward
    from lightglue_amd.weights import synthetic_state_dict

    conf = {"n_layers": 3}
    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(conf, seed=9).items()})
    params = model._schema_params(DEV)
    g = torch.Generator(device="cpu").manual_seed(4)
    B, M, N = 2, 150, 97
    d0 = torch.randn(B, M, 256, generator=g).to(DEV)
    d1 = torch.randn(B, N, 256, generator=g).to(DEV)
    la, _, t0, t1, scratch = _head_forward(model, 1, d0, d1, params, tokens, keep_scratch=True)
    w = torch.rand((B, M + 1, N + 1), generator=g).to(DEV)
    s_in, s_dust = torch.rand(B, generator=g).to(DEV), torch.rand(B, generator=g).to(DEV)
    gt0 = torch.randn(B, M, generator=g).to(DEV) if tokens else None
    gt1 = torch.randn(B, N, generator=g).to(DEV) if tokens else None
    needs = [True] * len(params) + [True, True]
    ref = _head_backward(model, 1, d0, d1, params, needs, w, s_in, s_dust, None, gt0, gt1)
    got = _head_backward(model, 1, d0, d1, params, needs, w, s_in, s_dust, None, gt0, gt1, fwd_scratch=scratch)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    n = 0
    for a, b in zip(got[2], ref[2]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
            n += 1
    assert n >= (6 if tokens else 4)


@pytest.mark.parametrize("B,N,layer", [(2, 150, 1), (1, 2048, 0), (3, 33, 2)])
def test_head_nll_forward_matches_stored_log_assignment(B, N, layer):
    """lg_head_nll_forward (the loss heads without a stored log assignment) against lg_head_forward
    + sg_nll_loss + torch argmaxes on the stored log assignment: the NLL terms to fp32 rounding (the
    fp64 sums are grouped differently), the argmaxes and token logits exactly; M != N raises the
    reference's error (losses.py:66-70)."""
    from lightglue_amd import LightGlue
    from lightglue_amd.lightglue import _head_forward, _head_nll_forward
    from lightglue_amd.superglue import _nll, nll_inputs
    from lightglue_amd.weights import synthetic_state_dict
    from sg_golden_util import ground_truth

    conf = {"n_layers": 3}
    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(conf, seed=12).items()})
    params = model._schema_params(DEV)
    g = torch.Generator(device="cpu").manual_seed(6)
    d0 = torch.randn(B, N, 256, generator=g).to(DEV)
    d1 = torch.randn(B, N, 256, generator=g).to(DEV)
    gt = {k: torch.from_numpy(v).to(DEV) for k, v in ground_truth(B, N, N, 8).items()}
    prepared = nll_inputs(gt, DEV)
    tokens = layer < 2
    terms, am0, am1, t0, t1, _ = _head_nll_forward(model, layer, d0, d1, params, tokens, prepared, 0.5)
    la, _, r0, r1 = _head_forward(model, layer, d0, d1, params, tokens)
    ref = _nll(la, gt, 1, 0.5, prepared)
    torch.cuda.synchronize()
    torch.testing.assert_close(terms, ref, rtol=2e-6, atol=1e-6)
    assert torch.equal(am0, la[:, :-1, :].max(-1).indices)
    assert torch.equal(am1, la[:, :, :-1].max(-2).indices)
    if tokens:
        assert torch.equal(t0, r0) and torch.equal(t1, r1)
    with pytest.raises(RuntimeError):
        _head_nll_forward(model, layer, d0, d1[:, : N - 1].contiguous(), params, False, prepared, 0.5)


@pytest.mark.parametrize("B,N,layer,reuse", [(2, 150, 1, False), (2, 148, 0, True), (1, 2048, 2, True), (3, 33, 1, True),
                                               (1, 3072, 0, True)])
def test_head_nll_backward_from_ground_truth_equals_dense_weights(B, N, layer, reuse):
    """lg_head_nll_backward (the NLL weights read from gt_assignment / gt_matches0/1, never a dense
    tensor) gives lg_head_backward's gradients on nll_weights (losses.py:62-73) bit for bit: every
    sum adds 0/1 values and every product is the same weight * scale.  M != N raises."""
    from lightglue_amd import LightGlue
    from lightglue_amd.lightglue import _head_backward, _head_forward
    from lightglue_amd.superglue import nll_inputs, nll_weights
    from lightglue_amd.weights import synthetic_state_dict
    from sg_golden_util import ground_truth

    conf = {"n_layers": 3}
    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(conf, seed=13).items()})
    params = model._schema_params(DEV)
    g = torch.Generator(device="cpu").manual_seed(7)
    d0 = torch.randn(B, N, 256, generator=g).to(DEV)
    d1 = torch.randn(B, N, 256, generator=g).to(DEV)
    gt = {k: torch.from_numpy(v).to(DEV) for k, v in ground_truth(B, N, N, 8).items()}
    prepared = nll_inputs(gt, DEV)
    w = nll_weights(d0.new_empty((B, N + 1, N + 1)), gt)
    s_in, s_dust = -torch.rand(B, generator=g).to(DEV), -torch.rand(B, generator=g).to(DEV)
    tokens = layer < 2
    gt0 = torch.randn(B, N, generator=g).to(DEV) if tokens else None
    gt1 = torch.randn(B, N, generator=g).to(DEV) if tokens else None
    needs = [True] * len(params) + [True, True]
    ref = _head_backward(model, layer, d0, d1, params, needs, w, s_in, s_dust, None, gt0, gt1)
    scratch = _head_forward(model, layer, d0, d1, params, tokens, keep_scratch=True)[4] if reuse else None
    got = _head_backward(model, layer, d0, d1, params, needs, None, s_in, s_dust, None, gt0, gt1, fwd_scratch=scratch,
                         gt=prepared)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    n = 0
    for a, b in zip(got[2], ref[2]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
            n += 1
    assert n >= (6 if tokens else 4)
    with pytest.raises(RuntimeError):
        _head_backward(model, layer, d0, d1[:, : N - 1].contiguous(), params, needs, None, s_in, s_dust, None, None, None,
                       gt=prepared)


def test_head_backward_dense_and_similarity_gradients():
    """_Head (plain autograd through log_assignment and similarity) against float64 torch."""
    from lightglue_amd import LightGlue
    from lightglue_amd.lightglue import _Head
    from lightglue_amd.weights import synthetic_state_dict
    from oracle.lightglue_ref import match_assignment

    conf = {"n_layers": 2}
    sd = synthetic_state_dict(conf, seed=4)
    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    gen = torch.Generator().manual_seed(3)
    B, M, N = 2, 70, 45
    d0 = torch.randn(B, M, 256, generator=gen)
    d1 = torch.randn(B, N, 256, generator=gen)
    gla = torch.randn(B, M + 1, N + 1, generator=gen)
    gsim = torch.randn(B, M, N, generator=gen) * 0.1
    W = {k: torch.from_numpy(v).double().requires_grad_() for k, v in sd.items()}
    x0, x1 = d0.double().requires_grad_(), d1.double().requires_grad_()
    la, sim = match_assignment(x0, x1, W, "log_assignment.0")
    ((la * gla.double()).sum() + (sim * gsim.double()).sum()).backward()
    params = model._schema_params(DEV)
    g0, g1 = d0.to(DEV).requires_grad_(), d1.to(DEV).requires_grad_()
    la_g, sim_g, _, _ = _Head.apply(model, 0, False, g0, g1, *params)
    ((la_g * gla.to(DEV)).sum() + (sim_g * gsim.to(DEV)).sum()).backward()
    for got, ref in ((g0.grad, x0.grad), (g1.grad, x1.grad)):
        r = ref.numpy()
        np.testing.assert_allclose(got.cpu().double().numpy(), r, atol=1e-5 * np.abs(r).max(), rtol=0)
    named = dict(model.named_parameters())
    for n in ("log_assignment.0.final_proj.weight", "log_assignment.0.final_proj.bias",
              "log_assignment.0.matchability.weight", "log_assignment.0.matchability.bias"):
        r = W[n].grad.numpy()
        np.testing.assert_allclose(named[n].grad.cpu().double().numpy(), r, atol=1e-5 * np.abs(r).max(), rtol=0)


HEAD_PARAMS = tuple(f"log_assignment.0.{n}" for n in ("final_proj.weight", "final_proj.bias", "matchability.weight",
                                                        "matchability.bias"))


def _head_model(seed):
    from lightglue_amd import LightGlue
    from lightglue_amd.weights import synthetic_state_dict

    conf = {"n_layers": 2}
    sd = synthetic_state_dict(conf, seed=seed)
    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model, sd


def _oracle_head(sd, d0, d1, weigh, dtype):
    """match_assignment (head 0) and its autograd gradients under loss = weigh(la, sim), in `dtype`:
    {"la", "sim", "gd0", "gd1", the four head parameters' gradients} as float64 numpy."""
    from oracle.lightglue_ref import match_assignment

    W = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in sd.items() if k.startswith("log_assignment.0.")}
    x0, x1 = d0.clone().to(dtype).requires_grad_(), d1.clone().to(dtype).requires_grad_()  # leaves of their own
    la, sim = match_assignment(x0, x1, W, "log_assignment.0")
    weigh(la, sim).backward()
    out = {"la": la.detach(), "sim": sim.detach(), "gd0": x0.grad, "gd1": x1.grad}
    out.update({n: W[n].grad for n in HEAD_PARAMS})
    return {k: v.double().numpy() for k, v in out.items()}


def _spread_check(tag, got, o64, o32):
    """The spread bar of test_backward_matches_reference_and_oracle per tensor, on the oracle's own
    float32 run: |got - o64| <= 8 |o32 - o64|_max + 1e-6 max|o64| + 1e-12.  Prints worst err / tol."""
    worst, bad = [], []
    for n, g in got.items():
        tol = 8 * float(np.abs(o32[n] - o64[n]).max()) + 1e-6 * float(np.abs(o64[n]).max()) + 1e-12
        err = float(np.abs(np.asarray(g, dtype=np.float64) - o64[n]).max())
        worst.append((err / tol, n))
        if not err <= tol:
            bad.append((n, err, tol))
    worst.sort(reverse=True)
    print(tag, "worst err/tol:", [(n, round(r, 3)) for r, n in worst[:5]])
    assert not bad, bad


@pytest.mark.parametrize("B,M,N", rc.HEAD_DENSE)
def test_head_dense_wide_n_vs_oracle(B, M, N):
    """test_head_backward_dense_and_similarity_gradients at the N regimes that pick another kernel
    (train_route_cases.HEAD_DENSE: sim_lse's fused QN = 2 / 4 and its two unfused routes, la_forward's
    generic kernel, la_grad_sums / la_grad_sim at wide N): the log assignment, the similarity, both
    descriptor gradients and the four head parameter gradients against the float64 oracle.  Bar:
    the spread bar (wide-N logsumexps move the fp32 floor; the oracle's own fp32 descriptor gradient
    sits 2.8e-6 relative from float64 at N = 2052)."""
    from lightglue_amd.lightglue import _Head

    model, sd = _head_model(4)
    gen = torch.Generator().manual_seed(3 + N)
    d0 = torch.randn(B, M, 256, generator=gen)
    d1 = torch.randn(B, N, 256, generator=gen)
    gla = torch.randn(B, M + 1, N + 1, generator=gen)
    gsim = torch.randn(B, M, N, generator=gen) * 0.1

    def weigh(la, sim):
        return (la * gla.to(la.dtype)).sum() + (sim * gsim.to(sim.dtype)).sum()

    o64 = _oracle_head(sd, d0, d1, weigh, torch.float64)
    o32 = _oracle_head(sd, d0, d1, weigh, torch.float32)
    params = model._schema_params(DEV)
    g0, g1 = d0.to(DEV).requires_grad_(), d1.to(DEV).requires_grad_()
    la_g, sim_g, _, _ = _Head.apply(model, 0, False, g0, g1, *params)
    ((la_g * gla.to(DEV)).sum() + (sim_g * gsim.to(DEV)).sum()).backward()
    named = dict(model.named_parameters())
    got = {"la": la_g.detach().cpu().numpy(), "sim": sim_g.detach().cpu().numpy(), "gd0": g0.grad.cpu().numpy(),
           "gd1": g1.grad.cpu().numpy()}
    got.update({n: named[n].grad.cpu().numpy() for n in HEAD_PARAMS})
    _spread_check(f"head dense {B, M, N}", got, o64, o32)


@pytest.mark.parametrize("B,N", rc.HEAD_NLL)
def test_head_nll_wide_n_vs_oracle(B, N):
    """The loss heads' fused kernels at the N regimes the bit-for-bit tests cannot judge (both of
    their sides read the same sim_lse output; train_route_cases.HEAD_NLL: la_nll KC = 8 / 16,
    la_grad_gt IT = 2 / 4): lg_head_nll_forward's five terms against the float64 NLL
    (oracle.superglue_ref.nll_loss) of the oracle's log assignment, and lg_head_nll_backward's
    gradients against float64 autograd on nll_weights scaled per pair -- both at the spread bar.
    The argmaxes are compared exactly with the GPU's stored log assignment (itself held to float64
    by test_head_dense_wide_n_vs_oracle): near-ties make a comparison with float64 undecidable."""
    from lightglue_amd.lightglue import _head_backward, _head_forward, _head_nll_forward
    from lightglue_amd.superglue import nll_inputs
    from oracle.superglue_ref import nll_loss
    from sg_golden_util import ground_truth

    model, sd = _head_model(13)
    params = model._schema_params(DEV)
    gen = torch.Generator().manual_seed(7 + N)
    d0 = torch.randn(B, N, 256, generator=gen)
    d1 = torch.randn(B, N, 256, generator=gen)
    s_in, s_dust = -torch.rand(B, generator=gen) - 0.5, -torch.rand(B, generator=gen) - 0.5
    gt = ground_truth(B, N, N, 8)
    bal = 0.3
    terms_ref = {}

    def weigh(la, sim):
        total, m = nll_loss(la, gt["gt_assignment"], gt["gt_matches0"], gt["gt_matches1"], bal)
        key = str(la.dtype)
        terms_ref[key] = torch.stack([total, m["nll_pos"], m["nll_neg"], m["num_matchable"], m["num_unmatchable"]])
        # d(loss)/d(la) = the NLL weights (losses.py:62-73), inner block scaled by s_in, dustbins by s_dust
        w = torch.zeros_like(la)
        w[:, :N, :N] = torch.from_numpy(gt["gt_assignment"]).to(la.dtype) * s_in.to(la.dtype)[:, None, None]
        w[:, :N, -1] = torch.from_numpy(gt["gt_matches0"] == -1).to(la.dtype) * s_dust.to(la.dtype)[:, None]
        w[:, -1, :N] = torch.from_numpy(gt["gt_matches1"] == -1).to(la.dtype) * s_dust.to(la.dtype)[:, None]
        return (la * w).sum()

    o64 = _oracle_head(sd, d0, d1, weigh, torch.float64)
    o32 = _oracle_head(sd, d0, d1, weigh, torch.float32)
    t64 = terms_ref["torch.float64"].detach().numpy()
    t32 = terms_ref["torch.float32"].detach().double().numpy()
    d0g, d1g = d0.to(DEV), d1.to(DEV)
    prepared = nll_inputs({k: torch.from_numpy(v).to(DEV) for k, v in gt.items()}, DEV)
    terms, am0, am1, _, _, scratch = _head_nll_forward(model, 0, d0g, d1g, params, False, prepared, bal)
    la = _head_forward(model, 0, d0g, d1g, params, False)[0]
    needs = [True] * len(params) + [True, True]
    gd0, gd1, grads = _head_backward(model, 0, d0g, d1g, params, needs, None, s_in.to(DEV), s_dust.to(DEV), None, None, None,
                                     fwd_scratch=scratch, gt=prepared)
    torch.cuda.synchronize()
    assert torch.equal(am0, la[:, :-1, :].max(-1).indices)
    assert torch.equal(am1, la[:, :, :-1].max(-2).indices)
    tg = terms.cpu().double().numpy()
    assert np.array_equal(tg[3:], t64[3:]), "num_matchable / num_unmatchable are counts"
    names = model._schema_names()
    got = {"gd0": gd0.cpu().numpy(), "gd1": gd1.cpu().numpy()}
    got.update({n: grads[names.index(n)].cpu().numpy() for n in HEAD_PARAMS})
    ref64 = {k: o64[k] for k in got}
    ref32 = {k: o32[k] for k in got}
    got["nll_terms"], ref64["nll_terms"], ref32["nll_terms"] = tg[:3], t64[:3], t32[:3]
    _spread_check(f"head nll {B, N}", got, ref64, ref32)


@pytest.mark.parametrize("conf,B,M,N", [({"n_layers": 2}, 2, 70, 45), ({"n_layers": 1, "input_dim": 64}, 1, 33, 130),
                                        ({"n_layers": 2, "add_scale_ori": True}, 3, 40, 40), rc.TRUNK_MULTIBLOCK])
def test_trunk_backward_ragged_vs_oracle(conf, B, M, N):
    """The training trunk (lg_train_forward / lg_train_backward) on ragged sets (M != N, sizes that
    are no multiple of any tile), input_proj and scale/ori positions, under an arbitrary loss on
    every layer's descriptors: every parameter gradient and both descriptor gradients against
    float64 autograd of the oracle (oracle/lightglue_train_ref.train_forward).  Bar: 2e-5 of each
    tensor's largest entry (fp32 arithmetic through <= 2 layers).  The 1180-row case
    (train_route_cases.TRUNK_MULTIBLOCK) reaches the split-k weight gradients with a partial last
    chunk and column-sum partials, the two-source ffn.0 gradient, and several row blocks with a
    partial last one in pe_backward, lngelu_bwd, colsum and both attention passes."""
    from lightglue_amd import LightGlue
    from lightglue_amd.weights import synthetic_pair, synthetic_state_dict
    from oracle.lightglue_train_ref import train_forward

    sd = synthetic_state_dict(conf, seed=11)
    pair = synthetic_pair(B=B, M=M, N=N, seed=12, dim=int(conf.get("input_dim", 256)))
    if conf.get("add_scale_ori"):
        rng = np.random.Generator(np.random.PCG64(5))
        for k, n in (("0", M), ("1", N)):
            pair["scales" + k] = (rng.random((B, n)) * 2).astype(np.float32)
            pair["oris" + k] = (rng.random((B, n)) * 6.28 - 3.14).astype(np.float32)
    L = int(conf["n_layers"])
    gen = torch.Generator().manual_seed(7)
    w0 = torch.randn(B, L, M, 256, generator=gen)
    w1 = torch.randn(B, L, N, 256, generator=gen)
    # float64 oracle
    W = {k: torch.from_numpy(v).double().requires_grad_() for k, v in sd.items()}
    data64 = {k: torch.from_numpy(v).double() for k, v in pair.items() if not k.startswith("descriptors")}
    x0 = torch.from_numpy(pair["descriptors0"]).double().requires_grad_()
    x1 = torch.from_numpy(pair["descriptors1"]).double().requires_grad_()
    data64["descriptors0"], data64["descriptors1"] = x0, x1
    layers, _ = train_forward(W, data64, conf)
    loss64 = sum((a * w0[:, i].double()).sum() + (b * w1[:, i].double()).sum() for i, (a, b) in enumerate(layers))
    loss64.backward()
    # HIP
    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.train()
    data = {k: torch.from_numpy(v).to(DEV) for k, v in pair.items() if not k.startswith(("image_size", "descriptors"))}
    g0 = torch.from_numpy(pair["descriptors0"]).to(DEV).requires_grad_()
    g1 = torch.from_numpy(pair["descriptors1"]).to(DEV).requires_grad_()
    data["descriptors0"], data["descriptors1"] = g0, g1
    data["view0"] = {"image_size": torch.from_numpy(pair["image_size0"]).to(DEV)}
    data["view1"] = {"image_size": torch.from_numpy(pair["image_size1"]).to(DEV)}
    pred = model(data)
    ((pred["ref_descriptors0"] * w0.to(DEV)).sum() + (pred["ref_descriptors1"] * w1.to(DEV)).sum()).backward()
    named = dict(model.named_parameters())
    bad, worst = [], []
    for n, w in W.items():
        if not n.startswith(("input_proj", "posenc.Wr", "transformers")):
            continue
        r = w.grad.numpy()
        got = named[n].grad.double().cpu().numpy()
        err, scale = np.abs(got - r).max(), np.abs(r).max()
        worst.append((float(err / (2e-5 * scale + 1e-9)), n))
        if err > 2e-5 * scale + 1e-9:
            bad.append((n, float(err), float(scale)))
    for got, ref, key in ((g0, x0, "d0"), (g1, x1, "d1")):
        r = ref.grad.numpy()
        err = np.abs(got.grad.double().cpu().numpy() - r).max()
        worst.append((float(err / (2e-5 * np.abs(r).max() + 1e-9)), key))
        if err > 2e-5 * np.abs(r).max() + 1e-9:
            bad.append((key, float(err), float(np.abs(r).max())))
    worst.sort(reverse=True)
    print("trunk", B, M, N, "worst err/tol:", [(n, round(r, 3)) for r, n in worst[:4]])
    assert not bad, bad[:8]


@pytest.mark.parametrize("frozen", ["posenc.Wr.weight", "posenc.condition_modulation.bias"])
def test_trunk_backward_with_one_posenc_parameter_frozen(frozen):
    """Freezing one positional-encoding parameter: the others still get their
    gradients -- equal to the run with every parameter trainable -- and the frozen one gets none
    (the library used to skip the posenc backward unless all three were requested, leaving the
    requested ones uninitialised)."""
    from lightglue_amd import LightGlue
    from lightglue_amd.weights import synthetic_pair, synthetic_state_dict

    conf = {"n_layers": 2}
    sd = synthetic_state_dict(conf, seed=11)
    pair = synthetic_pair(B=2, M=70, N=45, seed=12)
    gen = torch.Generator().manual_seed(7)
    w0 = torch.randn(2, 2, 70, 256, generator=gen).to(DEV)
    w1 = torch.randn(2, 2, 45, 256, generator=gen).to(DEV)

    def run(freeze):
        model = LightGlue(conf).to(DEV)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model.train()
        named = dict(model.named_parameters())
        if freeze:
            named[freeze].requires_grad_(False)
        data = {k: torch.from_numpy(v).to(DEV) for k, v in pair.items() if not k.startswith("image_size")}
        data["view0"] = {"image_size": torch.from_numpy(pair["image_size0"]).to(DEV)}
        data["view1"] = {"image_size": torch.from_numpy(pair["image_size1"]).to(DEV)}
        pred = model(data)
        ((pred["ref_descriptors0"] * w0).sum() + (pred["ref_descriptors1"] * w1).sum()).backward()
        return {n: (p.grad.clone() if p.grad is not None else None) for n, p in named.items() if n.startswith("posenc.")}

    full = run(None)
    part = run(frozen)
    assert part[frozen] is None
    # run-to-run noise: the attention backward's dQ sums are float atomics, and the
    # condition_modulation gradient is zero in exact arithmetic (a common phase cancels in q.k),
    # so compare on the scale of the Wr gradient
    scale = float(full["posenc.Wr.weight"].abs().max())
    for n, g in part.items():
        if n == frozen:
            continue
        assert g is not None and torch.isfinite(g).all(), n
        err = float((g - full[n]).abs().max())
        assert err <= 1e-4 * scale, (n, err, scale)


def test_loss_heads_backward_twice_through_a_retained_graph():
    """_HeadNLL's backward drops only the forward's scratch, not the ground truth its NLL
    weights come from, so a second backward through a retained graph recomputes the head
    (lg_head_nll_backward, from_forward = 0) and gives the first backward's gradients."""
    g, meta = load_grad("grad_train_b2_n64")
    conf, sd, pair, gt = grad_case(meta)
    from lightglue_amd import LightGlue

    model = LightGlue(conf).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.train()
    data = {k: torch.from_numpy(v).to(DEV) for k, v in pair.items() if not k.startswith("image_size")}
    data["view0"] = {"image_size": torch.from_numpy(pair["image_size0"]).to(DEV)}
    data["view1"] = {"image_size": torch.from_numpy(pair["image_size1"]).to(DEV)}
    data.update({k: torch.from_numpy(v).to(DEV) for k, v in gt.items()})
    pred = model(data)
    # the trunk's saved activations go with its first backward: differentiate the heads only
    rd0 = pred["ref_descriptors0"].detach().requires_grad_()
    rd1 = pred["ref_descriptors1"].detach().requires_grad_()
    losses, _ = model.loss({**pred, "ref_descriptors0": rd0, "ref_descriptors1": rd1}, data)
    loss = torch.mean(losses["total"])
    loss.backward(retain_graph=True)
    first = (rd0.grad.clone(), rd1.grad.clone())
    rd0.grad = rd1.grad = None
    loss.backward()
    for a, b in zip(first, (rd0.grad, rd1.grad)):
        scale = float(a.abs().max())
        assert scale > 0
        assert float((a - b).abs().max()) <= 1e-6 * scale
