"""CPU emulations of half-precision attention (``flash: true``), the references of
test_flash_host.py, test_gpu_attention_flash.py and test_gpu_flash_forward.py.

Nothing here can be bit-compared with the reference's flash path (it needs a CUDA device, and where
its kernel rounds P is an implementation detail), so two members of the family are emulated:

* ``emu_upstream``: operands ``x.half()``; scores and softmax in fp32 from those; P rounded to fp16;
  P V accumulated in fp32; the output rounded to fp16 (torch SDPA on fp16 tensors).
* ``emu_tiled``: the library's form.  The query is rounded AFTER the factor the kernel folds into it
  (``scale * log2(e)``; the cross block's ``s ** 0.5`` is already in q and k, as the GEMM epilogue
  applies it), the keys and values as they are; an online softmax over 64-key tiles in log2 units
  whose per-query reference puts a tile's largest exponent at 2^11 and is raised when a later tile
  passes 2^14; P = fp16(2^(s - reference)); l sums the unrounded exponentials in fp32; the output
  is NOT rounded.

``ref64`` is float64 attention on the unrounded inputs.  All three take head-major [B, H, N, 64]
tensors and return [B, Nq, H * 64] float64 rows (``*_heads``: [B, H, Nq, 64] float32, for the
model-level oracle).  ``lightglue_forward_flash`` runs the CPU oracle (oracle/lightglue_ref.py) with
one of the emulations as its attention, by rebinding ``_softmax_attention`` and ``cross_block`` for
the duration of the call.
"""
import contextlib
import functools
import math

import torch

import lgamd  # noqa: F401
import oracle.lightglue_ref as ref_mod

LOG2E = 1.4426950408889634
KT = 64  # keys per softmax step of the kernel
REF_EXP, RAISE_EXP = 11.0, 14.0  # csrc/attention.hip LG_ATTN_REF / LG_ATTN_RAISE


def _rows(o):
    return o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], -1).double()


def ref64(q, k, v, scale):
    s = torch.einsum("bhqd,bhkd->bhqk", q.double(), k.double()) * scale
    return _rows(torch.softmax(s, dim=-1) @ v.double())


def emu_upstream_heads(q, k, v, scale):
    qh, kh, vh = (t.half().float() for t in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", qh, kh) * torch.tensor(scale, dtype=torch.float32)
    p = torch.softmax(s, dim=-1).half().float()
    return (p @ vh).half().float()


def emu_tiled_heads(q, k, v, scale):
    y = (q.float() * torch.tensor(scale * LOG2E, dtype=torch.float32)).half().float()
    kh, vh = k.half().float(), v.half().float()
    B, H, Nq, _ = q.shape
    Nk = k.shape[2]
    m = torch.zeros(B, H, Nq, 1)
    l = torch.zeros(B, H, Nq, 1)
    o = torch.zeros(B, H, Nq, v.shape[-1])
    for t0 in range(0, Nk, KT):
        a = torch.einsum("bhqd,bhkd->bhqk", y, kh[:, :, t0:t0 + KT]) - m + REF_EXP  # log2(p 2^11)
        tmax = a.amax(-1, keepdim=True)
        raise_ = torch.ones_like(tmax, dtype=torch.bool) if t0 == 0 else tmax > RAISE_EXP
        d = torch.where(raise_, tmax - REF_EXP, torch.zeros_like(tmax))
        m = m + d
        a = a - d
        alpha = torch.exp2(-d)
        e = torch.exp2(a)
        l = l * alpha + e.sum(-1, keepdim=True)
        o = o * alpha + e.half().float() @ vh[:, :, t0:t0 + KT]
    return o / l


def emu_upstream(q, k, v, scale):
    return _rows(emu_upstream_heads(q, k, v, scale))


def emu_tiled(q, k, v, scale):
    return _rows(emu_tiled_heads(q, k, v, scale))


def hard_cap(q, k, v, scale):
    """(expm1(2^-9 L) + 2^-9) max|v| + 2e-6, L = max scale sum_d |q_d k_d|: one fp16 rounding each of
    q and k moves a logit by <= 2^-10 L, a logit perturbation d moves a softmax-weighted mean by
    <= (e^{2d} - 1) max|v|, the roundings of P, V and the sum l add <= 2^-11 max|v| each, and the
    last 2^-11 with the 2e-6 floor cover the fp32 arithmetic."""
    L = (scale * torch.einsum("bhqd,bhkd->bhqk", q.double().abs(), k.double().abs())).max().item()
    return (math.expm1(2.0 ** -9 * L) + 2.0 ** -9) * v.abs().max().item() + 2e-6


VARIANTS = {"upstream": emu_upstream_heads, "tiled": emu_tiled_heads}


@contextlib.contextmanager
def _flash_oracle(variant):
    emu = VARIANTS[variant]
    linear, ffn = ref_mod._linear, ref_mod._ffn

    def softmax_attention(q, k, v, scale):
        return emu(q, k, v, scale)

    def cross_block(x0, x1, W, p, H):
        """lightglue.py:220-249 with the flash branch (:229-233): m0 = flash(qk0, qk1, v1),
        m1 = flash(qk1, qk0, v0).  Upstream hands SDPA the unscaled qk (scale 1/sqrt(d) inside);
        the library scales both by s ** 0.5 in the to_qk epilogue and runs the attention at scale 1."""
        def heads(t):
            return t.unflatten(-1, (H, -1)).transpose(1, 2)

        qk0 = heads(linear(x0, W[p + ".to_qk.weight"], W[p + ".to_qk.bias"]))
        qk1 = heads(linear(x1, W[p + ".to_qk.weight"], W[p + ".to_qk.bias"]))
        v0 = heads(linear(x0, W[p + ".to_v.weight"], W[p + ".to_v.bias"]))
        v1 = heads(linear(x1, W[p + ".to_v.weight"], W[p + ".to_v.bias"]))
        s = (x0.shape[-1] // H) ** -0.5
        if variant == "tiled":
            qk0, qk1, s = qk0 * s ** 0.5, qk1 * s ** 0.5, 1.0
        m0, m1 = emu(qk0, qk1, v1, s), emu(qk1, qk0, v0, s)
        m0 = linear(m0.transpose(1, 2).flatten(-2), W[p + ".to_out.weight"], W[p + ".to_out.bias"])
        m1 = linear(m1.transpose(1, 2).flatten(-2), W[p + ".to_out.weight"], W[p + ".to_out.bias"])
        return ffn(x0, m0, W, p), ffn(x1, m1, W, p)

    saved = ref_mod._softmax_attention, ref_mod.cross_block
    ref_mod._softmax_attention, ref_mod.cross_block = softmax_attention, cross_block
    try:
        yield
    finally:
        ref_mod._softmax_attention, ref_mod.cross_block = saved


def lightglue_forward_flash(W, data, conf, variant):
    """The CPU oracle with half-precision attention: ``variant`` "upstream" or "tiled"."""
    with _flash_oracle(variant), torch.no_grad():
        return ref_mod.lightglue_forward(W, data, conf)


# ---------------------------------------------------------------- the model-level case
# B = 2, M = 300, N = 257 (neither a multiple of 64), 9 layers, the sharpened synthetic weights
MODEL_CONF = {"filter_threshold": 0.1}
MODEL_SHAPE = dict(B=2, M=300, N=257)
MODEL_SEED = 5  # synthetic_pair seed; weights seed 1 (the n300x257_b2 golden's inputs)
NEAR_TIE_CAP = 0.05


@functools.lru_cache(maxsize=None)
def model_case():
    """(weights, data, A, F1, F2): the fp32 oracle and the two flash oracles, computed once per
    process and shared (never modified) by the tests that need them."""
    from lightglue_amd.weights import synthetic_pair, synthetic_state_dict

    sd = synthetic_state_dict(MODEL_CONF, seed=1)
    data = synthetic_pair(seed=MODEL_SEED, **MODEL_SHAPE)
    with torch.no_grad():
        A = ref_mod.lightglue_forward(sd, data, MODEL_CONF)
    F1 = lightglue_forward_flash(sd, data, MODEL_CONF, "upstream")
    F2 = lightglue_forward_flash(sd, data, MODEL_CONF, "tiled")
    return sd, data, A, F1, F2


def spreads(F1, F2):
    """(d_s, d_la): max |F1 - F2| over matching_scores0/1 and over the finite log-assignment entries."""
    d_s = max((F1[k] - F2[k]).abs().max().item() for k in ("matching_scores0", "matching_scores1"))
    la1, la2 = F1["log_assignment"], F2["log_assignment"]
    fin = torch.isfinite(la1) & torch.isfinite(la2)
    return d_s, (la1[fin] - la2[fin]).abs().max().item()


def near_tie_masks(F1, F2):
    """Boolean [B, M] / [B, N] masks of the rows excluded from the match comparison: F1 and F2
    disagree on the match, or the row's top-1 / top-2 margin in F1's log assignment (dustbin
    included) is below 4 d_la."""
    _, d_la = spreads(F1, F2)
    la = F1["log_assignment"].double()
    r = la[:, :-1, :].topk(2, dim=2).values
    c = la[:, :, :-1].topk(2, dim=1).values
    tie0 = (r[..., 0] - r[..., 1] < 4 * d_la) | (F1["matches0"] != F2["matches0"])
    tie1 = (c[:, 0] - c[:, 1] < 4 * d_la) | (F1["matches1"] != F2["matches1"])
    return tie0, tie1
