"""Torch-CPU restatement of the open SuperPoint (reference
``gluefactory/models/extractors/superpoint_open.py:18-207``) as plain functions over its state dict.

The reference is not available where the GPU tests run; ``tests/test_sp_open_golden.py`` holds this
restatement to the reference's own outputs (``tests/golden/sp_open/spo_*.npz``), and the GPU tests
use it for seeded cases beyond the fixtures.  Line numbers refer to ``superpoint_open.py``.
"""
import torch
import torch.nn.functional as F

POOLED = ("backbone.0.1", "backbone.1.1", "backbone.2.1")
BACKBONE = ("backbone.0.0", "backbone.0.1", "backbone.1.0", "backbone.1.1", "backbone.2.0", "backbone.2.1",
            "backbone.3.0", "backbone.3.1")
DEFAULT_CONF = {"descriptor_dim": 256, "nms_radius": 4, "max_num_keypoints": None, "force_num_keypoints": False,
                "detection_threshold": 0.005, "remove_borders": 4, "dense_outputs": None}


def _t(sd, name, dtype):
    v = sd[name]
    return (v if torch.is_tensor(v) else torch.from_numpy(v)).to(dtype)


def vgg_block(x, sd, name, relu=True):
    """:57-73: conv -> ReLU -> BatchNorm(eps 1e-3, running statistics)."""
    dt = x.dtype
    w = _t(sd, f"{name}.conv.weight", dt)
    x = F.conv2d(x, w, _t(sd, f"{name}.conv.bias", dt), stride=1, padding=(w.shape[-1] - 1) // 2)
    if relu:
        x = F.relu(x)
    return F.batch_norm(x, _t(sd, f"{name}.bn.running_mean", dt), _t(sd, f"{name}.bn.running_var", dt),
                        _t(sd, f"{name}.bn.weight", dt), _t(sd, f"{name}.bn.bias", dt), training=False, eps=0.001)


def dense_maps(sd, image):
    """:118-134: (scores [B, 8Hc, 8Wc] before the NMS, descriptors_dense [B, 256, Hc, Wc])."""
    if image.shape[1] == 3:
        scale = image.new_tensor([0.299, 0.587, 0.114]).view(1, 3, 1, 1)
        image = (image * scale).sum(1, keepdim=True)
    x = image
    for name in BACKBONE:
        x = vgg_block(x, sd, name)
        if name in POOLED:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
    desc = F.normalize(vgg_block(vgg_block(x, sd, "descriptor.0"), sd, "descriptor.1", relu=False), p=2, dim=1)
    scores = vgg_block(vgg_block(x, sd, "detector.0"), sd, "detector.1", relu=False)
    scores = F.softmax(scores, 1)[:, :-1]
    b, _, h, w = scores.shape
    scores = scores.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8)
    scores = scores.permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
    return scores, desc


def batched_nms(scores, nms_radius):
    """:32-47."""
    def max_pool(x):
        return F.max_pool2d(x, kernel_size=nms_radius * 2 + 1, stride=1, padding=nms_radius)

    zeros = torch.zeros_like(scores)
    max_mask = scores == max_pool(scores)
    for _ in range(2):
        supp_mask = max_pool(max_mask.to(scores.dtype)) > 0
        supp_scores = torch.where(supp_mask, zeros, scores)
        new_max_mask = supp_scores == max_pool(supp_scores)
        max_mask = max_mask | (new_max_mask & (~supp_mask))
    return torch.where(max_mask, scores, zeros)


def candidate_map(scores, conf):
    """:135-143: the NMS'd scores with the borders at -1."""
    scores = batched_nms(scores, conf["nms_radius"])
    pad = conf["remove_borders"]
    if pad:
        scores[:, :pad] = -1
        scores[:, :, :pad] = -1
        scores[:, -pad:] = -1
        scores[:, :, -pad:] = -1
    return scores


def sample_descriptors(keypoints, descriptors, s=8):
    """:18-29; keypoints [B, N, 2] (x, y) without the +0.5, descriptors [B, C, Hc, Wc] -> [B, C, N]."""
    b, c, h, w = descriptors.shape
    keypoints = keypoints.to(descriptors.dtype)
    keypoints = (keypoints + 0.5) / (keypoints.new_tensor([w, h]) * s)
    keypoints = keypoints * 2 - 1
    d = F.grid_sample(descriptors, keypoints.view(b, 1, -1, 2), mode="bilinear", align_corners=False)
    return F.normalize(d.reshape(b, c, -1), p=2, dim=1)


def spo_forward(sd, data, conf=None, dtype=torch.float32):
    """:117-207 in eval mode.  Per-image keypoints are stacked (B > 1 needs equal counts, as the
    reference's ``torch.stack``; its list-``transpose`` failure at :193-202 is not reproduced) and
    ``force_num_keypoints`` needs every image to fill the budget (the pads are random)."""
    conf = dict(DEFAULT_CONF, **(conf or {}))
    image = data["image"]
    image = (image if torch.is_tensor(image) else torch.from_numpy(image)).to(dtype)
    dense_scores, desc_dense = dense_maps(sd, image)
    cand = candidate_map(dense_scores.clone(), conf)
    kps, scs = [], []
    for i in range(image.shape[0]):
        idx = torch.where(cand[i] > conf["detection_threshold"])
        k = torch.stack(idx, -1).flip(1).float()
        s = cand[i][idx]
        kmax = conf["max_num_keypoints"]
        if kmax is not None and kmax < len(k):
            s, ind = torch.topk(s, kmax, dim=0, sorted=True)
            k = k[ind]
        if conf["force_num_keypoints"]:
            assert len(k) == kmax, "spo_ref: force_num_keypoints with fewer candidates draws random pads"
        kps.append(k)
        scs.append(s)
    keypoints, scores = torch.stack(kps, 0), torch.stack(scs, 0)
    desc = sample_descriptors(keypoints, desc_dense)
    pred = {"keypoints": keypoints + 0.5, "keypoint_scores": scores, "descriptors": desc.transpose(-1, -2)}
    if conf["dense_outputs"]:
        pred["dense_descriptors"] = desc_dense
    return pred


def reference_with_margins(sd, data, conf=None):
    """(fp32 outputs, meta) for a seeded case without a fixture.  The meta is what
    tests/golden/make_sp_open_golden.py stores, from a float64 run of the same functions:
    ``e_scores`` / ``e_desc`` (max |fp32 - fp64| over matched keypoints and the dense map),
    per-image ``kth_gap``, ``positive`` and ``thr_gap``.  ``thr_gap`` is taken over the pixels whose
    crossing of the threshold could change the output: every positive pixel the NMS kept, or, where
    more than k candidates pass, the best k + 1 of them (one below that can cross the threshold
    without entering the top k).  Asserts that fp32 and fp64 select the same keypoint set."""
    conf = dict(DEFAULT_CONF, **(conf or {}))
    p32 = spo_forward(sd, data, conf)
    p64 = spo_forward(sd, data, conf, dtype=torch.float64)
    e_scores = e_desc = 0.0
    for b in range(p32["keypoints"].shape[0]):
        where = {tuple(p): i for i, p in enumerate(p64["keypoints"][b].numpy())}
        idx = [where.get(tuple(p), -1) for p in p32["keypoints"][b].numpy()]
        assert -1 not in idx and sorted(idx) == list(range(len(idx))), "fp32 and fp64 keypoint sets differ"
        if idx:
            e_scores = max(e_scores, float((p32["keypoint_scores"][b].double() - p64["keypoint_scores"][b][idx]).abs().max()))
            e_desc = max(e_desc, float((p32["descriptors"][b].double() - p64["descriptors"][b][idx]).abs().max()))
    if "dense_descriptors" in p32:
        e_desc = max(e_desc, float((p32["dense_descriptors"].double() - p64["dense_descriptors"]).abs().max()))
    image = data["image"]
    image = (image if torch.is_tensor(image) else torch.from_numpy(image)).double()
    cand = candidate_map(dense_maps(sd, image)[0].clone(), conf)
    thr, k, pad = conf["detection_threshold"], conf["max_num_keypoints"], conf["remove_borders"]
    gaps, positive, thr_gap = [], [], []
    for b in range(cand.shape[0]):
        v = torch.sort(cand[b][cand[b] > thr], descending=True).values
        gaps.append(float(v[k - 1] - v[k]) if k is not None and k < len(v) else float("inf"))
        positive.append(int((cand[b] > 0).sum()))
        kept = v[:k + 1] if k is not None and k < len(v) else cand[b][cand[b] > 0]
        thr_gap.append(float((kept - thr).abs().min()) if len(kept) else float("inf"))
    return p32, {"e_scores": e_scores, "e_desc": e_desc, "kth_gap": gaps, "positive": positive, "thr_gap": thr_gap,
                 "remove_borders": pad}
