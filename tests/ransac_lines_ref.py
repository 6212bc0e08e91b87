"""Float64 numpy restatement of the hybrid point-and-line LO-RANSAC for homographies,
written from the specification: live points and lines, the one fixed normalising frame per image, the
line of an image-1 segment, the counter-based sampler over points and lines together with the 2+2
rejection, the 8x9 minimal solver by Gauss-Jordan with complete pivoting, rounds of 256 hypotheses,
the 8-step local optimisation by an unweighted DLT in the fixed frame (through ``eigh`` here), the
stopping rule and the fp32 result whose two masks are its own classification in pixels.

``ransac_homography_lines`` returns every field of the kernel's ``info`` row and the case's ``margin``
as tests/ransac_ref.py does: the smallest ``|lhs - rhs| / |rhs|`` over every comparison that steers the
run (each residual against ``th_n`` or ``m * th_n``, each pivot against the floor, each segment length
against ``min_line_length``, the stop rule, the final residuals against ``th``).
"""
import math

import numpy as np

from ransac_ref import LO_MULTIPLIERS, ROUND, _Margin, corner_error, live_matches, sample

PIVOT_FLOOR = 1e-12
INFO_FIELDS = ("success", "num_point_matches", "num_line_matches", "num_point_inliers", "num_line_inliers", "best_t",
               "best_minimal_count", "rounds", "valid_hypotheses")


def live_lines(lines0, lines1, line_matches0=None, num0=None, num1=None, min_line_length=1.0, margin=None):
    """(rows [Kl, 8] float64 of a0 b0 a1 b1, their slots) under the kernel's rules."""
    lines0 = np.asarray(lines0, dtype=np.float32).reshape(-1, 2, 2).astype(np.float64)
    lines1 = np.asarray(lines1, dtype=np.float32).reshape(-1, 2, 2).astype(np.float64)
    n0 = len(lines0) if num0 is None else min(max(int(num0), 0), len(lines0))
    n1 = len(lines1) if num1 is None else min(max(int(num1), 0), len(lines1))
    m = np.arange(len(lines0)) if line_matches0 is None else np.asarray(line_matches0).astype(np.int64)
    sq = lambda s: float(((s[0] - s[1]) ** 2).sum())  # noqa: E731
    mll2 = float(min_line_length) ** 2
    slots = []
    for i in range(n0):
        if not 0 <= m[i] < n1:
            continue
        d0, d1 = sq(lines0[i]), sq(lines1[m[i]])
        if margin is not None and mll2 > 0:
            margin.note(np.array([d0, d1]), mll2)
        if d0 >= mll2 and d1 >= mll2:
            slots.append(i)
    slots = np.array(slots, dtype=np.int64)
    if len(slots) == 0:
        return np.zeros((0, 8)), slots
    return np.concatenate([lines0[slots].reshape(-1, 4), lines1[m[slots]].reshape(-1, 4)], 1), slots


def frame(xy):
    """(mean, scale) of the similarity x -> s (x - mean) over coordinates [n, 2]."""
    mean = xy.mean(0)
    return mean, math.sqrt(2.0) / (np.linalg.norm(xy - mean, axis=1).mean() + 1e-8)


def segment_line(seg):
    """(a, b, c) of segments [n, 4] (xa ya xb yb), unit normal.  The endpoints are taken in
    lexicographic (x, y) order, so that their order in the input cannot move a bit."""
    seg = np.asarray(seg, dtype=np.float64).reshape(-1, 4)
    swap = (seg[:, 0] > seg[:, 2]) | ((seg[:, 0] == seg[:, 2]) & (seg[:, 1] > seg[:, 3]))
    seg = np.where(swap[:, None], seg[:, [2, 3, 0, 1]], seg)
    nx, ny = seg[:, 1] - seg[:, 3], seg[:, 2] - seg[:, 0]
    with np.errstate(all="ignore"):
        n = np.sqrt(nx * nx + ny * ny)
        a, b = nx / n, ny / n
    return np.stack([a, b, -(a * seg[:, 0] + b * seg[:, 1])], 1)


def point_ratio(H, pts):
    """Forward transfer distances [..., Kp] of models [..., 3, 3] in the division-free form's terms:
    sqrt(ex^2 + ey^2) / |w|; non-finite where w is 0."""
    H = np.asarray(H, dtype=np.float64)
    x, y, u, v = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    with np.errstate(all="ignore"):
        X = H[..., 0, 0, None] * x + H[..., 0, 1, None] * y + H[..., 0, 2, None]
        Y = H[..., 1, 0, None] * x + H[..., 1, 1, None] * y + H[..., 1, 2, None]
        w = H[..., 2, 0, None] * x + H[..., 2, 1, None] * y + H[..., 2, 2, None]
        return np.sqrt((X - u * w) ** 2 + (Y - v * w) ** 2) / np.abs(w)


def line_ratio(H, ends, abc):
    """|a X + b Y + c w| / |w| of both mapped image-0 endpoints: [..., Kl, 2]."""
    H = np.asarray(H, dtype=np.float64)
    out = []
    with np.errstate(all="ignore"):
        for k in (0, 2):
            x, y = ends[:, k], ends[:, k + 1]
            X = H[..., 0, 0, None] * x + H[..., 0, 1, None] * y + H[..., 0, 2, None]
            Y = H[..., 1, 0, None] * x + H[..., 1, 1, None] * y + H[..., 1, 2, None]
            w = H[..., 2, 0, None] * x + H[..., 2, 1, None] * y + H[..., 2, 2, None]
            out.append(np.abs(abc[:, 0] * X + abc[:, 1] * Y + abc[:, 2] * w) / np.abs(w))
    return np.stack(out, -1)


def classify(H, pts, ends, abc, th, margin):
    """(point mask [..., Kp], line mask [..., Kl]) under models [..., 3, 3]; non-finite is an outlier."""
    rp, rl = point_ratio(H, pts), line_ratio(H, ends, abc)
    margin.note(rp, th), margin.note(rl, th)
    with np.errstate(invalid="ignore"):
        return np.isfinite(rp) & (rp < th), (np.isfinite(rl) & (rl < th)).all(-1)


def point_rows(P):
    """The two DLT rows of points [..., 4]: [..., 2, 9]."""
    x, y, u, v = P[..., 0], P[..., 1], P[..., 2], P[..., 3]
    z, o = np.zeros_like(x), np.ones_like(x)
    return np.stack([np.stack([z, z, z, -x, -y, -o, v * x, v * y, v], -1),
                     np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], -1)], -2)


def line_rows(E, L):
    """One row per image-0 endpoint of lines (ends [..., 4], (a, b, c) [..., 3]): [..., 2, 9]."""
    a, b, c = L[..., 0], L[..., 1], L[..., 2]
    return np.stack([np.stack([a * E[..., k], a * E[..., k + 1], a, b * E[..., k], b * E[..., k + 1], b,
                               c * E[..., k], c * E[..., k + 1], c], -1) for k in (0, 2)], -2)


def minimal_solver(A, margin):
    """The null vector of an 8x9 system by Gauss-Jordan with complete pivoting, or None."""
    A = np.array(A, dtype=np.float64)
    scale = np.abs(A).max()
    used, pc = np.zeros(9, dtype=bool), []
    for s in range(8):
        mag = np.abs(A[s:]).copy()
        mag[:, used] = -1.0
        r, c = np.unravel_index(np.argmax(mag), mag.shape)  # the first maximum in row-major order
        piv = A[s + r, c]
        margin.note(np.array([abs(piv)]), PIVOT_FLOOR * scale)
        if not abs(piv) > PIVOT_FLOOR * scale:
            return None
        A[[s, s + r]] = A[[s + r, s]]
        A[s] = A[s] / piv
        for i in range(8):
            if i != s:
                A[i] = A[i] - A[i, c] * A[s]
        used[c] = True
        pc.append(c)
    free = int(np.flatnonzero(~used)[0])
    h = np.zeros(9)
    h[free] = 1.0
    h[pc] = -A[:, free]
    return h.reshape(3, 3)


def dlt(pts, ends, abc):
    """Unweighted DLT in the fixed frame: two rows per point and two per line."""
    R = np.concatenate([point_rows(pts).reshape(-1, 9), line_rows(ends, abc).reshape(-1, 9)])
    return np.linalg.eigh(R.T @ R)[1][:, 0].reshape(3, 3)


def local_optimisation(H, count, pts, ends, abc, th, margin):
    for m in LO_MULTIPLIERS:
        sp, sl = classify(H, pts, ends, abc, m * th, margin)
        if sp.sum() + sl.sum() < 4:
            break
        fit = dlt(pts[sp], ends[sl], abc[sl])
        ip, il = classify(fit, pts, ends, abc, th, margin)
        c = int(ip.sum() + il.sum())
        if c >= count:
            H, count = fit, c
    return H, count


def ransac_homography_lines(pts, lns, th, max_iters=3000, confidence=0.995, seed=0):
    """pts [Kp, 4] (x0 y0 x1 y1), lns [Kl, 8] (a0 b0 a1 b1), both live and in pixels.  Returns success, H
    (fp32 [3, 3]), the two masks, the info fields and the margin."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    lns = np.asarray(lns, dtype=np.float64).reshape(-1, 8)
    th = float(np.float32(th))
    Kp, Kl = len(pts), len(lns)
    K = Kp + Kl
    margin = _Margin()
    out = {"success": 0, "num_point_matches": Kp, "num_line_matches": Kl, "num_point_inliers": 0, "num_line_inliers": 0,
           "best_t": -1, "best_minimal_count": 0, "rounds": 0, "valid_hypotheses": 0, "H": np.eye(3, dtype=np.float32),
           "inliers": np.zeros(Kp, dtype=bool), "line_inliers": np.zeros(Kl, dtype=bool), "margin": math.inf}
    if K < 4:
        return out
    m0, s0 = frame(np.concatenate([pts[:, :2], lns[:, 0:2], lns[:, 2:4]]))
    m1, s1 = frame(np.concatenate([pts[:, 2:], lns[:, 4:6], lns[:, 6:8]]))
    npts = np.concatenate([s0 * (pts[:, :2] - m0), s1 * (pts[:, 2:] - m1)], 1)
    ends = s0 * (lns[:, :4] - np.tile(m0, 2))
    abc = segment_line(s1 * (lns[:, 4:] - np.tile(m1, 2)))
    th_n = s1 * th
    best_min, best_lo, H_lo = -1, -1, None
    done = 0
    while done < max_iters:
        ts = range(done, min(done + ROUND, max_iters))
        done = ts[-1] + 1
        out["rounds"] += 1
        models, ids = [], []
        for t in ts:
            idx = sample(seed, t, K)
            if idx is None or sum(i < Kp for i in idx) == 2:
                continue
            A = np.concatenate([point_rows(npts[i]) if i < Kp else line_rows(ends[i - Kp], abc[i - Kp]) for i in idx])
            H = minimal_solver(A, margin)
            if H is not None:
                models.append(H), ids.append(t)
        out["valid_hypotheses"] += len(ids)
        if ids:
            ip, il = classify(np.stack(models), npts, ends, abc, th_n, margin)
            counts = ip.sum(1) + il.sum(1)
            k = int(np.argmax(counts))  # the first of equal counts: the lowest t
            if counts[k] > best_min:
                best_min, out["best_t"] = int(counts[k]), ids[k]
                H, c = local_optimisation(models[k], best_min, npts, ends, abc, th_n, margin)
                if c > best_lo:
                    best_lo, H_lo = c, H
        if best_lo >= 4:
            with np.errstate(divide="ignore"):
                lhs, rhs = done * np.log1p(-((best_lo / K) ** 4)), math.log1p(-confidence)
            margin.note(lhs, rhs)
            if lhs <= rhs:
                break
    out["best_minimal_count"] = max(best_min, 0)
    out["margin"] = margin.value
    if H_lo is None:
        return out
    T0 = np.array([[s0, 0, -s0 * m0[0]], [0, s0, -s0 * m0[1]], [0, 0, 1.0]])
    T1inv = np.array([[1 / s1, 0, m1[0]], [0, 1 / s1, m1[1]], [0, 0, 1.0]])
    Hp = T1inv @ H_lo @ T0
    if not np.isfinite(Hp).all() or not abs(Hp[2, 2]) > 1e-12 * np.abs(Hp).max():
        return out
    H32 = (Hp / Hp[2, 2]).astype(np.float32)
    ip, il = classify(H32.astype(np.float64), pts, lns[:, :4], segment_line(lns[:, 4:]), th, margin)
    out["margin"] = margin.value
    if ip.sum() + il.sum() < 4:
        return out
    out.update(success=1, num_point_inliers=int(ip.sum()), num_line_inliers=int(il.sum()), H=H32, inliers=ip,
               line_inliers=il)
    return out


def info_row(out):
    return np.array([out[k] for k in INFO_FIELDS] + [0, 0, 0], dtype=np.int32)


def estimate_pair(kpts0, kpts1, matches0, lines0, lines1, line_matches0, th, num0=None, num1=None, num_lines0=None,
                  num_lines1=None, min_line_length=1.0, H_gt=None, size=None, **options):
    """One pair in keypoint / line-slot form: the restatement's outputs in slot order.  Either set may
    be empty ([0, 2] keypoints, [0, 2, 2] lines)."""
    margin = _Margin()
    pts, slots = live_matches(np.asarray(kpts0).reshape(-1, 2), np.asarray(kpts1).reshape(-1, 2), matches0, num0, num1)
    lns, lslots = live_lines(lines0, lines1, line_matches0, num_lines0, num_lines1, min_line_length, margin)
    out = ransac_homography_lines(pts, lns, th, **options)
    out["margin"] = min(out["margin"], margin.value)
    mask = np.zeros(len(np.asarray(kpts0).reshape(-1, 2)), dtype=bool)
    lmask = np.zeros(len(np.asarray(lines0).reshape(-1, 2, 2)), dtype=bool)
    mask[slots], lmask[lslots] = out["inliers"], out["line_inliers"]
    out["inliers_slots"], out["line_inliers_slots"] = mask, lmask
    out["m_kpts"], out["m_lines"] = pts.astype(np.float32), lns.astype(np.float32)
    if H_gt is not None:
        out["H_error"] = corner_error(out["H"], H_gt, size) if out["success"] else math.inf
    return out
