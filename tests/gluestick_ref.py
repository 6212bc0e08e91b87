"""Functional torch restatement of GlueStick's eval forward over a plain state dict
(reference ``gluefactory/models/matchers/gluestick.py``), fp32 and fp64 capable.

``gluestick_forward(sd, data, conf, dtype)`` takes numpy / torch inputs keyed like the matcher's
data (``image_size`` [B, 2] (w, h) per view, or ``image_hw`` for the image-shape fallback) and
returns the matcher's outputs plus ``gnn_descriptors0/1`` [B, n, D] and ``line_layer_x``: the residual
stream ``(x0, x1)`` after every line layer application.  Everything is row-major [B, n, D]; the
reference's channel-first layout and its ``view(b, dim, heads, n)`` head split are restated as
``channel = d * heads + h``.

The three new kernels have their own restatements: :func:`line_update`, :func:`double_softmax`,
:func:`line_scores`.
"""
import numpy as np
import torch

HEADS = 4


def _tensor(v, dtype, device=None):
    t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)
    t = t.to(dtype) if t.is_floating_point() else t
    return t.to(device) if device is not None else t


def _lin(sd, name, x):  # Conv1d(k = 1) on rows
    return x @ sd[name + ".weight"][:, :, 0].T + sd[name + ".bias"]


def _bn(sd, name, x, eps=1e-5):
    alpha = sd[name + ".weight"] / torch.sqrt(sd[name + ".running_var"] + eps)
    return (x - sd[name + ".running_mean"]) * alpha + sd[name + ".bias"]


def mlp(sd, prefix, x, n_linear):
    """``MLP(channels)``: linear, (BatchNorm, ReLU) between linears."""
    for i in range(n_linear):
        x = _lin(sd, f"{prefix}.{3 * i}", x)
        if i < n_linear - 1:
            x = torch.relu(_bn(sd, f"{prefix}.{3 * i + 1}", x))
    return x


def normalize(pts, size):
    """pts [B, n, 2], size [B, 2] (w, h): centre at the image middle, scale by 0.7 max(w, h)."""
    return (pts - size[:, None] / 2) / (size.max(1, keepdim=True).values * 0.7)[:, None]


def _attention_update(sd, p, x, src):
    """AttentionalPropagation: multi-head attention of x over src, merge, MLP([x, message])."""
    B, n, D = x.shape
    hd = D // HEADS

    def heads(t):  # channel d * HEADS + h -> [B, h, n, d]
        return t.view(B, -1, hd, HEADS).permute(0, 3, 1, 2)

    q = heads(_lin(sd, p + ".attn.proj.0", x))
    k = heads(_lin(sd, p + ".attn.proj.1", src))
    v = heads(_lin(sd, p + ".attn.proj.2", src))
    prob = torch.softmax(q @ k.transpose(-1, -2) / hd**0.5, -1)
    msg = (prob @ v).permute(0, 2, 3, 1).reshape(B, n, D)  # back to channel d * HEADS + h
    msg = _lin(sd, p + ".attn.merge", msg)
    return mlp(sd, p + ".mlp", torch.cat([x, msg], -1), 2)


def line_update(sd, prefix, x, line_enc, idx):
    """One ``LineLayer`` on one image set: x [B, n, D], line_enc [B, 2L, D], idx [B, 2L] (int64).
    Every endpoint sends MLP([x[own junction], x[the line's other junction], line_enc]); a junction
    adds the mean of what its endpoints sent (none: unchanged)."""
    B, n, D = x.shape
    own = torch.gather(x, 1, idx[..., None].expand(-1, -1, D))
    other = own.view(B, -1, 2, D).flip(2).reshape(B, -1, D)
    msg = mlp(sd, prefix + ".mlp", torch.cat([own, other, line_enc], -1), 2)
    pair = torch.arange(B, device=x.device)[:, None].expand_as(idx)
    total = torch.zeros_like(x).index_put_((pair, idx), msg, accumulate=True)
    count = torch.zeros(B, n, dtype=x.dtype, device=x.device).index_put_((pair, idx), torch.ones_like(idx, dtype=x.dtype),
                                                                          accumulate=True)
    return x + total / count.clamp(min=1)[..., None]


def double_softmax(scores, bin_score):
    """``log_double_softmax``: [B, M, N] -> [B, M+1, N+1]."""
    B, M, N = scores.shape
    bin_ = torch.as_tensor(bin_score, dtype=scores.dtype, device=scores.device)
    rows = torch.log_softmax(torch.cat([scores, bin_.expand(B, M, 1)], 2), 2)
    cols = torch.log_softmax(torch.cat([scores, bin_.expand(B, 1, N)], 1), 1)
    out = scores.new_zeros(B, M + 1, N + 1)
    out[:, :M, :N] = (rows[:, :, :N] + cols[:, :M]) / 2
    out[:, :M, N] = rows[:, :, N]
    out[:, M, :N] = cols[:, M]
    return out


def line_scores(md0, md1, idx0, idx1):
    """Projected descriptors [B, n, D] and endpoint junctions [B, L, 2] -> raw line scores [B, L0, L1]:
    the better of the two endpoint orientations, halved."""
    D = md0.shape[-1]
    e0 = torch.gather(md0, 1, idx0.reshape(idx0.shape[0], -1)[..., None].expand(-1, -1, D))
    e1 = torch.gather(md1, 1, idx1.reshape(idx1.shape[0], -1)[..., None].expand(-1, -1, D))
    s = (e0 @ e1.transpose(1, 2) / D**0.5).view(e0.shape[0], e0.shape[1] // 2, 2, e1.shape[1] // 2, 2)
    return 0.5 * torch.maximum(s[:, :, 0, :, 0] + s[:, :, 1, :, 1], s[:, :, 0, :, 1] + s[:, :, 1, :, 0])


def get_matches(la, th):
    """Mutual nearest neighbours of la[:, :-1, :-1] with exp(max) > th (the SuperGlue rule)."""
    inner = la[:, :-1, :-1]
    max0, max1 = inner.max(2), inner.max(1)
    m0, m1 = max0.indices, max1.indices
    ar0 = torch.arange(m0.shape[1], device=la.device)[None]
    ar1 = torch.arange(m1.shape[1], device=la.device)[None]
    mutual0 = ar0 == m1.gather(1, m0)
    mutual1 = ar1 == m0.gather(1, m1)
    zero = la.new_zeros(())
    s0 = torch.where(mutual0, max0.values.exp(), zero)
    s1 = torch.where(mutual1, s0.gather(1, m1), zero)
    valid0 = mutual0 & (s0 > th)
    valid1 = mutual1 & valid0.gather(1, m1)
    return torch.where(valid0, m0, -1), torch.where(valid1, m1, -1), s0, s1


def _size(data, v, B, dtype, device):
    if data.get(f"image_size{v}") is not None:
        return _tensor(data[f"image_size{v}"], dtype, device)
    h, w = data["image_hw"]
    return torch.tensor([[float(w), float(h)]], dtype=dtype, device=device).expand(B, 2)


def gluestick_forward(sd, data, conf, dtype=torch.float64, device=None):
    """``device``: where to compute (default: the CPU; the benchmark runs it on the GPU)."""
    def _t(v, dt):
        return _tensor(v, dt, device)

    sd = {k: _t(v, dtype) for k, v in sd.items()}
    layers = list(conf.get("GNN_layers", ["self", "cross"] * 9))
    iters = int(conf.get("num_line_iterations", 1))
    th = float(conf.get("filter_threshold", 0.2))
    n_enc = len(conf.get("keypoint_encoder", [32, 64, 128, 256])) + 1
    k = [_t(data[f"keypoints{v}"], dtype) for v in "01"]
    B = k[0].shape[0]
    size = [_size(data, v, B, dtype, device) for v in "01"]
    x = []
    for v in range(2):
        kn = normalize(k[v], size[v])
        inp = torch.cat([kn, _t(data[f"keypoint_scores{v}"], dtype)[..., None]], -1)
        x.append(_t(data[f"descriptors{v}"], dtype) + mlp(sd, "kenc.encoder", inp, n_enc))
    idx = [_t(data[f"lines_junc_idx{v}"], dtype).long().reshape(B, -1) for v in "01"]
    L = [data[f"lines{v}"].shape[1] for v in "01"]
    with_lines = L[0] > 0 and L[1] > 0
    enc = [None, None]
    if with_lines:
        for v in range(2):
            ends = normalize(_t(data[f"lines{v}"], dtype).reshape(B, -1, 2), size[v]).view(B, L[v], 2, 2)
            off = ends[:, :, 1] - ends[:, :, 0]
            off = torch.stack([off, -off], 2).reshape(B, 2 * L[v], 2)
            # the reference tiles the scores (scores.repeat(1, 2)): endpoint column c reads line c mod L
            sc = _t(data[f"line_scores{v}"], dtype).repeat(1, 2)
            enc[v] = mlp(sd, "lenc.encoder", torch.cat([ends.reshape(B, 2 * L[v], 2), off, sc[..., None]], -1), n_enc)
    after_lines = []
    for i, kind in enumerate(layers):
        p = f"gnn.layers.{i}.update"
        s0, s1 = (x[1], x[0]) if kind == "cross" else (x[0], x[1])
        x = [x[0] + _attention_update(sd, p, x[0], s0), x[1] + _attention_update(sd, p, x[1], s1)]
        if kind == "self" and with_lines:
            for _ in range(iters):
                x = [line_update(sd, f"gnn.line_layers.{i // 2}", x[v], enc[v], idx[v]) for v in range(2)]
                after_lines.append((x[0], x[1]))
    md = [_lin(sd, "final_proj", x[v]) for v in range(2)]
    la = double_softmax(md[0] @ md[1].transpose(1, 2) / 256**0.5, sd["bin_score"])
    m0, m1, ms0, ms1 = get_matches(la, th)
    out = {"log_assignment": la, "matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1,
           "gnn_descriptors0": x[0], "gnn_descriptors1": x[1], "line_layer_x": after_lines}
    if with_lines:
        mdl = [_lin(sd, "final_line_proj", x[v]) for v in range(2)]
        raw = line_scores(mdl[0], mdl[1], idx[0].view(B, L[0], 2), idx[1].view(B, L[1], 2))
        lla = double_softmax(raw, sd["line_bin_score"])
        lm0, lm1, ls0, ls1 = get_matches(lla, th)
    else:
        raw = torch.zeros(B, L[0], L[1], dtype=dtype, device=device)
        lla = torch.zeros(B, L[0], L[1], dtype=dtype, device=device)
        lm0, lm1 = torch.full((B, L[0]), -1, device=device), torch.full((B, L[1]), -1, device=device)
        ls0 = torch.zeros(B, L[0], dtype=dtype, device=device)
        ls1 = torch.zeros(B, L[1], dtype=dtype, device=device)
    out.update({"line_log_assignment": lla, "line_matches0": lm0, "line_matches1": lm1, "line_matching_scores0": ls0,
                "line_matching_scores1": ls1, "raw_line_scores": raw})
    return out


def nll(la, gta, gt0, gt1, balancing=0.5):
    """``sub_loss`` values: (nll, num_matchable, num_unmatchable) per pair, in the dtype of la."""
    pos = gta.to(la.dtype)
    num_pos = pos.sum((1, 2)).clamp(min=1)
    neg0, neg1 = (gt0 == -1).to(la.dtype), (gt1 == -1).to(la.dtype)
    num_neg = (neg0.sum(1) + neg1.sum(1)).clamp(min=1)
    nll_pos = -(la[:, :-1, :-1] * pos).sum((1, 2)) / num_pos
    nll_neg = (-(la[:, :-1, -1] * neg0).sum(1) - (la[:, -1, :-1] * neg1).sum(1)) / num_neg
    return balancing * nll_pos + (1 - balancing) * nll_neg, num_pos, num_neg
