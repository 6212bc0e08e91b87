"""Pure-torch CPU restatement of ALIKED's eval forward (reference
``gluefactory/models/extractors/aliked.py``), fp32 and fp64 capable, functional over a state dict.
Includes ``deform_conv2d`` by torchvision's definition (torchvision is not a dependency):

* offset channel ``2k`` is dy and ``2k+1`` dx of tap ``k`` (taps row-major);
* the sample position of tap ``(i, j)`` at output ``(y, x)`` is ``(y - pad + i + dy, x - pad + j + dx)``;
* the value there is bilinear; a position with ``y <= -1``, ``y >= H``, ``x <= -1`` or ``x >= W``
  contributes 0, and so does every corner outside ``[0, H-1] x [0, W-1]``.

The tests compare the HIP extractor against this in fp64; ``test_aliked_golden.py`` pins this
restatement to fixtures made by the real reference.
"""
import numpy as np
import torch
import torch.nn.functional as F

from lightglue_amd.aliked_weights import ALIKED_CFGS

BN_EPS = 1e-5
TEMPERATURE = 0.1
N_LIMIT_MAX = 20000


def deform_conv2d(input, offset, weight, bias=None, padding=(1, 1), mask=None):
    """torchvision.ops.deform_conv2d for stride 1, dilation 1, one offset group, no mask."""
    assert mask is None
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    B, C, H, W = input.shape
    Co, Ci, kh, kw = weight.shape
    assert Ci == C and offset.shape[1] == 2 * kh * kw
    Ho, Wo = H + 2 * ph - kh + 1, W + 2 * pw - kw + 1
    assert offset.shape[2:] == (Ho, Wo)
    ys = torch.arange(Ho, dtype=input.dtype).view(1, Ho, 1)
    xs = torch.arange(Wo, dtype=input.dtype).view(1, 1, Wo)
    flat = input.reshape(B, C, H * W)
    cols = []
    for k in range(kh * kw):
        i, j = divmod(k, kw)
        py = ys - ph + i + offset[:, 2 * k]
        px = xs - pw + j + offset[:, 2 * k + 1]
        inside = (py > -1) & (py < H) & (px > -1) & (px < W)
        y0, x0 = torch.floor(py), torch.floor(px)
        ly, lx = py - y0, px - x0
        val = torch.zeros((B, C, Ho, Wo), dtype=input.dtype)
        for dy, dx, wgt in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
            yy, xx = y0 + dy, x0 + dx
            ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(B, 1, Ho * Wo).expand(B, C, Ho * Wo)
            g = torch.gather(flat, 2, idx).view(B, C, Ho, Wo)
            val = val + g * (wgt * ok.to(input.dtype)).unsqueeze(1)
        cols.append(val)
    col = torch.stack(cols, 2).reshape(B, C * kh * kw, Ho * Wo)  # (c, k) as the weight's (ci, i, j)
    out = torch.matmul(weight.reshape(Co, -1), col).view(B, Co, Ho, Wo)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def _bn(sd, n, x):
    s = sd[f"{n}.weight"] / torch.sqrt(sd[f"{n}.running_var"] + BN_EPS)
    return (x - sd[f"{n}.running_mean"].view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + sd[f"{n}.bias"].view(1, -1, 1, 1)


def _conv(sd, n, x, dcn):
    if not dcn:
        return F.conv2d(x, sd[f"{n}.weight"], None, padding=1)
    lim = max(x.shape[2:]) / 4.0
    off = F.conv2d(x, sd[f"{n}.offset_conv.weight"], sd[f"{n}.offset_conv.bias"], padding=1).clamp(-lim, lim)
    return deform_conv2d(x, off, sd[f"{n}.regular_conv.weight"], None, padding=1)


def _block(sd, n, x, dcn, residual):
    y = F.selu(_bn(sd, f"{n}.bn1", _conv(sd, f"{n}.conv1", x, dcn)))
    y = _bn(sd, f"{n}.bn2", _conv(sd, f"{n}.conv2", y, dcn))
    if residual:
        y = y + F.conv2d(x, sd[f"{n}.downsample.weight"], sd[f"{n}.downsample.bias"])
    return F.selu(y)


def dense_maps(sd, image):
    """(normalised feature map [B,dim,H,W], score map [B,1,H,W]), both unpadded."""
    H, W = image.shape[-2:]
    ph, pw = (-H) % 32, (-W) % 32
    pads = [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]
    x = F.pad(image, pads, mode="replicate")
    x1 = _block(sd, "block1", x, False, False)
    x2 = _block(sd, "block2", F.avg_pool2d(x1, 2), False, True)
    x3 = _block(sd, "block3", F.avg_pool2d(x2, 4), True, True)
    x4 = _block(sd, "block4", F.avg_pool2d(x3, 4), True, True)
    levels = []
    for i, (xl, scale) in enumerate(((x1, 1), (x2, 2), (x3, 8), (x4, 32)), 1):
        a = F.selu(F.conv2d(xl, sd[f"conv{i}.weight"]))
        levels.append(a if scale == 1 else F.interpolate(a, scale_factor=scale, mode="bilinear", align_corners=True))
    cat = torch.cat(levels, 1)
    s = F.selu(F.conv2d(cat, sd["score_head.0.weight"]))
    s = F.selu(F.conv2d(s, sd["score_head.2.weight"], padding=1))
    s = F.selu(F.conv2d(s, sd["score_head.4.weight"], padding=1))
    s = torch.sigmoid(F.conv2d(s, sd["score_head.6.weight"], padding=1))
    feat = F.normalize(cat, p=2, dim=1)
    crop = (slice(None), slice(None), slice(pads[2], pads[2] + H), slice(pads[0], pads[0] + W))
    return feat[crop], s[crop]


def nms_map(scores, radius):
    """simple_nms (aliked.py:47-70) on [B,1,H,W]."""
    k = 2 * radius + 1
    pool = lambda t: F.max_pool2d(t, k, 1, radius)  # noqa: E731
    keep = scores == pool(scores)
    for _ in range(2):
        near = pool(keep.to(scores.dtype)) > 0
        rest = torch.where(near, torch.zeros_like(scores), scores)
        keep = keep | ((rest == pool(rest)) & ~near)
    return torch.where(keep, scores, torch.zeros_like(scores))


def candidate_map(score_map, radius, image_size=None):
    """The NMS map with the borders at 0 (aliked.py:120-132)."""
    nms = nms_map(score_map, radius).clone()
    B, _, H, W = nms.shape
    nms[:, :, :radius] = 0
    nms[:, :, :, :radius] = 0
    for b in range(B):
        w, h = (int(image_size[b][0]), int(image_size[b][1])) if image_size is not None else (W, H)
        nms[b, :, max(h - radius, 0):] = 0
        nms[b, :, :, max(w - radius, 0):] = 0
    return nms


def select(nms, score_map, top_k, threshold, n_limit):
    """Per image pixel indices: top-k over the NMS map (ties: lower index first), or the threshold
    mode (aliked.py:135-158)."""
    B = nms.shape[0]
    flat = nms.reshape(B, -1)
    if top_k > 0:
        return [torch.sort(flat[b], descending=True, stable=True).indices[:top_k] for b in range(B)]
    mean = score_map.reshape(B, -1).mean(1).view(B, 1)
    mask = flat > threshold if threshold > 0 else flat > mean
    if threshold > 0 and mask.sum() == 0:
        mask = flat > mean
    out = []
    for b in range(B):
        idx = mask[b].nonzero()[:, 0]
        if len(idx) > n_limit:
            idx = idx[torch.sort(score_map.reshape(B, -1)[b][idx], descending=True, stable=True).indices[:n_limit]]
        out.append(idx)
    return out


def refine(score_map_b, idx, radius):
    """Soft-argmax position in [-1, 1], dispersity and sampled score of the pixels idx of one image
    (aliked.py:167-216); score_map_b [1,H,W]."""
    _, H, W = score_map_b.shape
    dt = score_map_b.dtype
    k = 2 * radius + 1
    win = F.unfold(score_map_b[None], k, padding=radius)[0].t()[idx]  # [N, k*k], rows dy-major
    r = torch.arange(-radius, radius + 1, dtype=dt)
    grid = torch.stack([r.repeat(k), r.repeat_interleave(k)], 1)  # (dx, dy)
    e = torch.exp((win - win.max(1, keepdim=True).values) / TEMPERATURE)
    tot = e.sum(1, keepdim=True)
    res = e @ grid / tot
    d2 = (((grid[None] - res[:, None]) / radius) ** 2).sum(-1)
    disp = (e * d2).sum(1) / tot[:, 0]
    xy = torch.stack([idx % W, idx // W], 1).to(dt) + res
    kn = xy / torch.tensor([W - 1, H - 1], dtype=dt) * 2 - 1
    samp = F.grid_sample(score_map_b[None], kn.view(1, 1, -1, 2), mode="bilinear", align_corners=True)[0, 0, 0]
    return kn, disp, samp


def describe(sd, feat_b, kn, M):
    """SDDH (aliked.py:513-588) for one image: feat_b [dim,H,W] normalised, kn [N,2] in [-1,1]."""
    C, H, W = feat_b.shape
    dt = feat_b.dtype
    N = kn.shape[0]
    wh = torch.tensor([W - 1, H - 1], dtype=dt)
    kp = (kn / 2 + 0.5) * wh
    corner = (kp.long().to(dt) - 3 / 2 + 1).long()  # get_patches: truncation twice
    cx = corner[:, 0].clamp(0, W - 1 - 3)
    cy = corner[:, 1].clamp(0, H - 1 - 3)
    d = torch.arange(3)
    yy = (cy[:, None, None] + d[None, :, None]).expand(N, 3, 3)
    xx = (cx[:, None, None] + d[None, None, :]).expand(N, 3, 3)
    patch = feat_b[:, yy, xx].permute(1, 0, 2, 3)  # [N, C, 3, 3]
    lim = max(H, W) / 4.0
    o = F.conv2d(patch, sd["desc_head.offset_conv.0.weight"], sd["desc_head.offset_conv.0.bias"])
    o = F.conv2d(F.selu(o), sd["desc_head.offset_conv.2.weight"], sd["desc_head.offset_conv.2.bias"]).clamp(-lim, lim)
    off = o[:, :, 0, 0].view(N, 2, M).permute(0, 2, 1)  # [N, M, (x, y)]
    pos = 2.0 * (kp[:, None] + off) / wh - 1
    f = F.grid_sample(feat_b[None], pos.reshape(1, N * M, 1, 2), mode="bilinear", align_corners=True)
    f = f.reshape(C, N, M).permute(1, 0, 2)  # [N, C, M]
    f = F.selu(torch.einsum("dc,ncp->ndp", sd["desc_head.sf_conv.weight"][:, :, 0, 0], f))
    return F.normalize(torch.einsum("ncp,pcd->nd", f, sd["desc_head.agg_weights"]), p=2.0, dim=1)


def aliked_forward(sd, data, conf, dtype=torch.float64):
    """The reference's output dict (lists per image where counts differ are returned as lists).
    ``keypoint_scores`` is the dispersity and ``score_dispersity`` the sampled score: the reference's
    swapped unpacking (aliked.py:768 against :240)."""
    g = ALIKED_CFGS[conf.get("model_name", "aliked-n16")]
    radius = int(conf.get("nms_radius", 2))
    k = int(conf.get("max_num_keypoints", -1))
    thr = float(conf.get("detection_threshold", 0.2))
    sd = {n: torch.as_tensor(np.asarray(v)).to(dtype) for n, v in sd.items() if not n.endswith("num_batches_tracked")}
    image = torch.as_tensor(np.asarray(data["image"])).to(dtype)
    isz = data.get("image_size")
    isz = None if isz is None else np.asarray(isz)
    with torch.no_grad():
        feat, score = dense_maps(sd, image)
        nms = candidate_map(score, radius, isz)
        idx = select(nms, score, -1 if thr > 0 else k, thr, k if k > 0 else N_LIMIT_MAX)
        B, _, H, W = image.shape
        wh = torch.tensor([W, H], dtype=dtype)
        kpts, desc, disp, samp = [], [], [], []
        for b in range(B):
            kn, d, s = refine(score[b], idx[b], radius)
            desc.append(describe(sd, feat[b], kn, g["M"]))
            kpts.append(wh * (kn + 1) / 2.0)
            disp.append(d)
            samp.append(s)
    same = len({len(i) for i in idx}) == 1
    pack = (lambda v: torch.stack(v)) if same else (lambda v: v)
    return {"keypoints": pack(kpts), "descriptors": pack(desc), "keypoint_scores": pack(disp),
            "score_dispersity": pack(samp), "score_map": score, "nms_map": nms, "indices": idx}
