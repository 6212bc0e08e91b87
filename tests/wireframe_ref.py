"""numpy statement of the wireframe step (lightglue_amd.wireframe), written from its definition:
DBSCAN(eps, min_samples=1) is the connected components of "distance <= eps" numbered by lowest member
(union-find here), junctions are index-order means of their members, a keypoint goes when it is
strictly closer than the radius to an endpoint, descriptors are a zero-padded bilinear sample of the
dense map at x / s - 0.5 followed by an L2 normalisation, and the associativity is the identity plus
every line's junction pair."""
import numpy as np


def cluster_labels(pts, eps):
    """pts [E, 2] -> labels [E] (component numbered by its lowest index), count."""
    p = np.asarray(pts).astype(np.float64)
    n = len(p)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    if n:
        dx, dy = p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]
        adj = dx * dx + dy * dy <= float(eps) * float(eps)
        for i, j in zip(*np.nonzero(np.triu(adj, 1))):
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    roots = [find(i) for i in range(n)]
    order = {r: k for k, r in enumerate(sorted(set(roots)))}
    return np.asarray([order[r] for r in roots], np.int64), len(order)


def ordered_mean(values, labels, n, dtype):
    """Mean per label, summed in index order in ``dtype`` then divided once."""
    v = np.asarray(values).astype(dtype)
    acc = np.zeros((n,) + v.shape[1:], dtype)
    cnt = np.zeros(n, dtype)
    for i, lab in enumerate(labels):
        acc[lab] = acc[lab] + v[i]
        cnt[lab] += 1
    return (acc / cnt.reshape((n,) + (1,) * (v.ndim - 1))).astype(dtype)


def removed_mask(kp, ep, radius):
    """float32, strict: sqrt(dx*dx + dy*dy) < radius for any endpoint."""
    kp, ep = np.asarray(kp, np.float32), np.asarray(ep, np.float32)
    if not len(ep):
        return np.zeros(len(kp), bool)
    d = kp[:, None] - ep[None]
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    return (dist < np.float32(radius)).any(1)


def sample_descriptors(dense_hwc, pts, s, dtype=np.float64):
    """dense_hwc [Hc, Wc, D], pts [P, 2] pixels -> [P, D]."""
    g = np.asarray(dense_hwc).astype(dtype)
    Hc, Wc, D = g.shape
    p = np.asarray(pts).astype(dtype)
    out = np.zeros((len(p), D), dtype)
    fx, fy = p[:, 0] / dtype(s) - dtype(0.5), p[:, 1] / dtype(s) - dtype(0.5)
    x0, y0 = np.floor(fx), np.floor(fy)
    for ox in (0, 1):
        for oy in (0, 1):
            x, y = x0 + ox, y0 + oy
            w = (1 - np.abs(fx - x)) * (1 - np.abs(fy - y))
            ok = (x >= 0) & (x < Wc) & (y >= 0) & (y < Hc) & np.isfinite(fx) & np.isfinite(fy)
            xi, yi = np.where(ok, x, 0).astype(np.int64), np.where(ok, y, 0).astype(np.int64)
            out += np.where(ok, w, 0)[:, None] * g[yi, xi]
    nrm = np.sqrt((out * out).sum(1, keepdims=True))
    return out / np.maximum(nrm, dtype(1e-12))


def associativity(pairs, n):
    a = np.eye(n, dtype=bool)
    if len(pairs):
        a[pairs[:, 0], pairs[:, 1]] = True
        a[pairs[:, 1], pairs[:, 0]] = True
    return a


def wireframe(inp, conf, fill_junctions=None, fill_keypoints=None, s=8, dtype=np.float64):
    """The extractor's outputs for one batch.  ``inp``: lines [B, L, 2, 2], line_scores [B, L] (as the
    line extractor returns them), keypoints, keypoint_scores, descriptors, dense_descriptors [B, D, Hc, Wc].
    ``conf``: nms_radius, merge_points, merge_line_endpoints, force_num_keypoints, force_num_lines,
    max_num_lines.  Returns lists per image where the sizes can differ."""
    lines = np.asarray(inp["lines"], np.float32)
    B, L = lines.shape[:2]
    r = conf.get("nms_radius", 3)
    scores = np.asarray(inp["line_scores"], np.float32)
    if L:
        scores = (scores / (scores.max(1)[:, None] + np.float32(1e-8))).astype(np.float32)
    merge_ep = conf.get("merge_line_endpoints", True) and L > 0
    out = {k: [] for k in ("keypoints", "keypoint_scores", "descriptors", "lines", "lines_junc_idx", "pl_associativity",
                           "num_junctions", "labels", "removed")}
    out["line_scores"], out["orig_lines"] = scores, lines
    for b in range(B):
        dense = np.transpose(np.asarray(inp["dense_descriptors"][b]), (1, 2, 0))
        ep = lines[b].reshape(-1, 2)
        kp = np.asarray(inp["keypoints"][b], np.float32).astype(dtype)
        ks = np.asarray(inp["keypoint_scores"][b], np.float32).astype(dtype)
        kd = np.asarray(inp["descriptors"][b], np.float32).astype(dtype)
        rem = removed_mask(inp["keypoints"][b], ep, r) if conf.get("merge_points", True) else np.zeros(len(kp), bool)
        if rem.any() and conf.get("force_num_keypoints", False):
            kp[rem] = np.asarray(fill_keypoints[b], dtype)[rem]
            ks[rem] = 0
            kd[rem] = sample_descriptors(dense, kp[rem], s, dtype)
        elif rem.any():
            kp, ks, kd = kp[~rem], ks[~rem], kd[~rem]
        if merge_ep:
            labels, n_true = cluster_labels(ep, r)
            junc = ordered_mean(ep, labels, n_true, dtype)
            jsc = ordered_mean(np.repeat(scores[b], 2), labels, n_true, dtype)
            if conf.get("force_num_lines", False):
                J = 2 * conf["max_num_lines"]
                junc = np.concatenate([junc, np.asarray(fill_junctions[b], dtype)[: J - n_true]])
                jsc = np.concatenate([jsc, np.zeros(J - n_true, dtype)])
        else:
            labels, n_true = np.arange(2 * L, dtype=np.int64), 2 * L
            junc, jsc = ep.astype(dtype), np.repeat(scores[b], 2).astype(dtype)
        pairs = labels.reshape(-1, 2)
        out["labels"].append(labels)
        out["removed"].append(rem)
        out["lines"].append(junc[labels].reshape(-1, 2, 2))
        out["lines_junc_idx"].append(pairs)
        out["keypoints"].append(np.concatenate([junc, kp]))
        out["keypoint_scores"].append(np.concatenate([jsc, ks]))
        out["descriptors"].append(np.concatenate([sample_descriptors(dense, junc, s, dtype), kd]))
        out["pl_associativity"].append(associativity(pairs if merge_ep else pairs[:0], len(junc) + len(kp)))
        out["num_junctions"].append(n_true)
    return out
